/*
 * tests/cpp/test_host_core.cpp -- the engine's HIP-free host core (ol_dsp_amd/csrc/olfx_host.h) on
 * the CPU: note-event folding, the event section and packet layout, the reference setters'
 * coefficient words, validation ("a rejected call changes nothing") and the rack's CC routing.
 * Links olfx_host.cpp directly (no libolfx.so, no GPU); also built under ASan + UBSan
 * (tests/test_sanitizers.py).
 */
#include <map>
#include <utility>

#include "../../ol_dsp_amd/csrc/olfx_host.h"
#include "harness.h"

using namespace olfx;
using host::Shadow;

namespace {

uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

/* daisysp::mtof through libm at run time, as fold_events' table is made */
float mtof(int note) {
    volatile float k = (float)note;
    return powf(2.f, (k - 69.0f) / 12.0f) * 440.0f;
}

/* A shadow whose first (all-instances) packet has gone out: nothing dirty. */
Shadow fresh(int kind, uint32_t n, float sr = 48000.f) {
    Shadow s;
    s.init(kind, n, sr);
    s.reset();
    const host::PacketPlan pl = s.plan(false);
    std::vector<uint32_t> buf(pl.words);
    s.fill_records(pl, buf.data());
    return s;
}

std::vector<uint32_t> record(const Shadow &s, uint32_t i) {
    std::vector<uint32_t> w(host::coef_segments(s.kind).total());
    s.derive_record(i, w.data());
    return w;
}

olfx_voice_event vev(uint32_t inst, int type, int note = 0, float value = 0.f) {
    return olfx_voice_event{inst, (uint8_t)type, (uint8_t)note, 0, 0, value};
}

/* The event section as voice.hip's voice_event reads it: workgroup g takes its kVevCap fixed
 * slots, or -- slot 0 marked VEV_MORE -- `count` records of the overflow list from slot 0's y;
 * a record with ops lands on voice x & 63 of the group.  voice -> (ops, frequency bits). */
std::map<uint32_t, std::pair<uint32_t, uint32_t>> decode_events(const uint32_t *fix, uint32_t n) {
    const uint32_t groups = (n + 63u) / 64u;
    const uint32_t *more = fix + (size_t)groups * kVevCap * 2;
    std::map<uint32_t, std::pair<uint32_t, uint32_t>> out;
    for (uint32_t g = 0; g < groups; ++g) {
        const uint32_t *rec = fix + 2 * (size_t)g * kVevCap;
        uint32_t cnt = kVevCap;
        if ((rec[0] >> 8) & VEV_MORE) {
            cnt = rec[0] >> 16;
            rec = more + 2 * (size_t)rec[1];
        }
        for (uint32_t k = 0; k < cnt; ++k)
            if (rec[2 * k] >> 8) out[g * 64u + (rec[2 * k] & 63u)] = {rec[2 * k] >> 8, rec[2 * k + 1]};
    }
    return out;
}

struct Snapshot {
    std::vector<float> params;
    std::vector<uint8_t> configured;
    std::vector<uint32_t> dirty;
    int64_t components;
    explicit Snapshot(const Shadow &s)
        : params(s.params), configured(s.configured), dirty(s.dirty_list), components(s.n_components) {}
    bool same(const Shadow &s) const {
        return std::memcmp(params.data(), s.params.data(), params.size() * 4) == 0 && configured == s.configured &&
               dirty == s.dirty_list && components == s.n_components;
    }
};

}  // namespace

TEST(HostCore, FoldComposesPerVoice) {
    Shadow s = fresh(OLFX_KIND_VOICE, 130);
    const olfx_voice_event ev[] = {
        vev(7, OLFX_EV_NOTE_ON, 60), vev(8, OLFX_EV_GATE_ON), vev(9, OLFX_EV_NOTE_ON, 60),
        vev(7, OLFX_EV_NOTE_OFF), vev(8, OLFX_EV_SET_FREQUENCY, 0, 123.5f),
        vev(9, OLFX_EV_SET_FREQUENCY, 0, 100.f), vev(9, OLFX_EV_NOTE_ON, 72), vev(10, OLFX_EV_NOTE_ON, 69)};
    EXPECT_EQ(s.voice_events(ev, 8), OLFX_OK);
    s.fold_events();
    EXPECT_TRUE(s.events.empty());
    EXPECT_EQ(s.folded.size(), (size_t)4);          /* one record per voice, by first appearance */
    if (s.folded.size() != 4) return;
    for (uint32_t k = 0; k < 4; ++k) EXPECT_EQ(s.folded[k].inst, 7u + k);
    EXPECT_EQ(s.folded[0].op, VEV_GATE_SET | VEV_RETRIGGER | VEV_FREQ);   /* GATE_ON clear */
    EXPECT_EQ(s.folded[0].freq, bits(mtof(60)));
    EXPECT_EQ(s.folded[1].op, VEV_GATE_SET | VEV_GATE_ON | VEV_FREQ);
    EXPECT_EQ(s.folded[1].freq, bits(123.5f));
    EXPECT_EQ(s.folded[2].op, VEV_GATE_SET | VEV_GATE_ON | VEV_RETRIGGER | VEV_FREQ);
    EXPECT_EQ(s.folded[2].freq, bits(mtof(72)));
    EXPECT_EQ(s.folded[3].freq, bits(440.0f));
    /* the queue's two entry points refuse what they always refused, and queue nothing */
    const olfx_event bad = {130, OLFX_EV_NOTE_ON, 60, 0, 0};
    EXPECT_EQ(s.note_events(&bad, 1), OLFX_E_ARG);
    EXPECT_EQ(std::string(s.msg), std::string("olfx_note_events: bad event 0"));
    EXPECT_TRUE(s.events.empty());
}

TEST(HostCore, EventSectionFixedSlotsAndOverflow) {
    const uint32_t n = 130, groups = 3;
    Shadow s = fresh(OLFX_KIND_VOICE, n);
    std::vector<olfx_voice_event> ev;
    for (uint32_t v = 0; v < kVevCap; ++v) ev.push_back(vev(v * 5, OLFX_EV_NOTE_ON, 40 + (int)v));   /* group 0: full */
    const uint32_t crowd[kVevCap + 1] = {64 + 5, 64 + 1, 64 + 63, 64 + 3, 64 + 7};                  /* group 1: one too many */
    for (uint32_t k = 0; k <= kVevCap; ++k) ev.push_back(vev(crowd[k], OLFX_EV_SET_FREQUENCY, 0, 100.f + (float)k));
    ev.push_back(vev(129, OLFX_EV_GATE_OFF));                                                         /* group 2: one */
    EXPECT_EQ(s.voice_events(ev.data(), (uint32_t)ev.size()), OLFX_OK);
    s.fold_events();
    EXPECT_EQ(s.n_more, kVevCap + 1);
    const host::PacketPlan pl = s.plan(true);
    EXPECT_EQ(pl.words, pl.o_ev + 2 * ((size_t)groups * kVevCap + kVevCap + 1));
    std::vector<uint32_t> buf(pl.words, 0xFFFFFFFFu);
    s.write_events(buf.data() + pl.o_ev);
    const uint32_t *fix = buf.data() + pl.o_ev, *more = fix + 2 * groups * kVevCap;
    for (uint32_t k = 0; k < kVevCap; ++k) {            /* group 0: all in its fixed slots */
        EXPECT_EQ(fix[2 * k], (k * 5) | (VEV_GATE_SET | VEV_GATE_ON | VEV_RETRIGGER | VEV_FREQ) << 8);
        EXPECT_EQ(fix[2 * k + 1], bits(mtof(40 + (int)k)));
    }
    EXPECT_EQ(fix[2 * kVevCap], VEV_MORE << 8 | 5u << 16);   /* group 1: slot 0 points at its run */
    EXPECT_EQ(fix[2 * kVevCap + 1], 0u);
    for (uint32_t k = 1; k < kVevCap; ++k) {
        EXPECT_EQ(fix[2 * (kVevCap + k)], 0u);
        EXPECT_EQ(fix[2 * (kVevCap + k) + 1], 0u);
    }
    for (uint32_t k = 0; k <= kVevCap; ++k) {           /* the five records, in fold order */
        EXPECT_EQ(more[2 * k], ((crowd[k] & 63u) | VEV_FREQ << 8));
        EXPECT_EQ(more[2 * k + 1], bits(100.f + (float)k));
    }
    EXPECT_EQ(fix[2 * 2 * kVevCap], (129u & 63u) | VEV_GATE_SET << 8);   /* group 2: one record, then empty slots */
    for (uint32_t w = 2 * 2 * kVevCap + 2; w < 2 * groups * kVevCap; ++w) EXPECT_EQ(fix[w], 0u);
    /* what the kernel decodes is the folded set */
    const auto got = decode_events(fix, n);
    EXPECT_EQ(got.size(), s.folded.size());
    for (const host::Folded &r : s.folded) {
        const auto it = got.find(r.inst);
        EXPECT_TRUE(it != got.end() && it->second.first == r.op && it->second.second == r.freq);
    }

    /* a block with events in one group only: every fixed slot of the other groups is zero */
    const olfx_voice_event one = vev(70, OLFX_EV_GATE_ON);
    EXPECT_EQ(s.voice_events(&one, 1), OLFX_OK);
    s.fold_events();
    EXPECT_EQ(s.n_more, 0u);
    std::vector<uint32_t> sec(2 * groups * kVevCap, 0xFFFFFFFFu);
    s.write_events(sec.data());
    for (uint32_t w = 0; w < sec.size(); ++w)
        EXPECT_EQ(sec[w], w == 2 * kVevCap ? ((70u & 63u) | (VEV_GATE_SET | VEV_GATE_ON) << 8) : 0u);
}

TEST(HostCore, PacketPlanAndRecords) {
    const int kinds[2] = {OLFX_KIND_CHAIN, OLFX_KIND_VOICE};
    const uint32_t pick[5] = {4, 1, 2, 0, 3};           /* the order the instances are touched in */
    for (const int kind : kinds) {
        const host::Segments sg = host::coef_segments(kind);
        EXPECT_EQ(sg.nseg, kind == OLFX_KIND_CHAIN ? 3u : 1u);
        const uint32_t W = sg.total();
        EXPECT_EQ(W, kind == OLFX_KIND_CHAIN ? (uint32_t)(2 * CHC_N + DTC_N) : (uint32_t)VCC_N);
        for (const uint32_t m : {1u, 3u, 5u}) {
            Shadow s = fresh(kind, 5);
            for (uint32_t k = 0; k < m; ++k) {          /* distinct parameters, so records differ */
                const float v = 0.1f + 0.1f * (float)pick[k];
                EXPECT_EQ(s.set_range(pick[k], 1, kind == OLFX_KIND_CHAIN ? OLFX_CN_VERB0 + OLFX_DT_DECAY : OLFX_VC_AMP_SUSTAIN, 1, &v), OLFX_OK);
            }
            const host::PacketPlan pl = s.plan(false);
            EXPECT_EQ(pl.dense, m == 5);
            EXPECT_EQ(pl.o_inst, (size_t)0);
            EXPECT_EQ(pl.o_val, m == 5 ? (size_t)0 : (size_t)4);   /* dense: no instance list */
            EXPECT_TRUE(pl.o_val % 4 == 0 && pl.o_ev % 4 == 0);
            EXPECT_EQ(pl.o_ev, (pl.o_val + (size_t)W * m + 3) / 4 * 4);
            EXPECT_EQ(pl.words, pl.o_ev);
            std::vector<std::vector<uint32_t>> want;
            for (uint32_t r = 0; r < m; ++r) want.push_back(record(s, m == 5 ? r : pick[r]));
            std::vector<uint32_t> buf(pl.words, 0xFFFFFFFFu);
            s.fill_records(pl, buf.data());
            EXPECT_TRUE(s.dirty_list.empty());
            for (uint32_t r = 0; r < m; ++r) {
                if (!pl.dense) EXPECT_EQ(buf[pl.o_inst + r], pick[r]);
                for (uint32_t w = 0; w < W; ++w) EXPECT_EQ(buf[pl.o_val + (size_t)w * m + r], want[r][w]);   /* [W][m] */
            }
        }
    }
    /* the sections of a listed packet with events: 4-word aligned, in order */
    const host::PacketPlan pl = host::plan_packet(130, 3, VCC_N, true, 7);
    EXPECT_TRUE(!pl.dense && pl.o_inst == 0 && pl.o_val == 4 && pl.o_ev == (4 + 3 * VCC_N + 3) / 4 * 4);
    EXPECT_EQ(pl.words, pl.o_ev + 2 * (3 * kVevCap + 7));

    /* the largest voice packet: every voice changed and with an event, two crowded workgroups */
    Shadow s;
    s.init(OLFX_KIND_VOICE, 130, 48000.f);
    s.reset();
    std::vector<olfx_voice_event> ev;
    for (uint32_t v = 0; v < 130; ++v) ev.push_back(vev(v, OLFX_EV_NOTE_ON, (int)(v % 128)));
    EXPECT_EQ(s.voice_events(ev.data(), 130), OLFX_OK);
    s.fold_events();
    EXPECT_EQ(s.n_more, 128u);
    const host::PacketPlan big = s.plan(true);
    EXPECT_TRUE(big.dense);
    EXPECT_TRUE(big.words <= host::max_packet_words(OLFX_KIND_VOICE, 130));
    std::vector<uint32_t> buf(big.words);
    s.fill_records(big, buf.data());
    s.write_events(buf.data() + big.o_ev);
    EXPECT_EQ(decode_events(buf.data() + big.o_ev, 130).size(), (size_t)130);
}

TEST(HostCore, Coefficients) {
    {   /* reverb: the pre-delay in samples and decay diffusion 2 */
        Shadow s = fresh(OLFX_KIND_DATTORRO, 4);
        const float pre[4] = {2.0f, 13.0f, 0.0f, -0.0f};
        EXPECT_EQ(s.set_range(0, 4, OLFX_DT_PREDELAY, 1, pre), OLFX_OK);
        EXPECT_EQ(record(s, 0)[DTC_PREDELAY], bits(1408.f));      /* 9600 mod 8192 */
        EXPECT_EQ(record(s, 1)[DTC_PREDELAY], bits(5056.f));      /* 62400 mod 8192 */
        EXPECT_EQ(record(s, 2)[DTC_PREDELAY], bits(0.f));
        EXPECT_EQ(record(s, 3)[DTC_PREDELAY], bits(0.f));
        EXPECT_TRUE(!s.uniform_predelay());
        const float decay[2] = {0.05f, 0.9f};
        EXPECT_EQ(s.set_range(0, 2, OLFX_DT_DECAY, 1, decay), OLFX_OK);
        EXPECT_EQ(record(s, 0)[DTC_DD2], bits(0.25f));
        EXPECT_EQ(record(s, 1)[DTC_DD2], bits(0.5f));
        EXPECT_EQ(record(s, 1)[DTC_DECAY], bits(0.9f));
    }
    Shadow ch = fresh(OLFX_KIND_CHORUS, 2), ps = fresh(OLFX_KIND_PITCHSHIFT, 2), dt = fresh(OLFX_KIND_DATTORRO, 2);
    {   /* chorus: the LFO's phase offset as a 64-bit fraction of a cycle; 1.0 wraps to 0 */
        EXPECT_EQ(record(ch, 0)[CHC_LFO_OFF], 0u);                /* the default phase, 1.0 */
        EXPECT_EQ(record(ch, 0)[CHC_LFO_OFF_LO], 0u);
        EXPECT_EQ(ch.set_range(0, 1, OLFX_CH_PHASE, 1, std::vector<float>{0.5f}.data()), OLFX_OK);
        EXPECT_EQ(record(ch, 0)[CHC_LFO_OFF], 0x80000000u);
        EXPECT_EQ(record(ch, 0)[CHC_LFO_OFF_LO], 0u);
    }
    {   /* pitch-shift = the default chorus with pitch and window replaced */
        const float sw[2] = {1.5f, 6.0f};
        EXPECT_EQ(ps.set_range(1, 1, OLFX_PS_SHIFT, 2, sw), OLFX_OK);
        EXPECT_EQ(ch.set_range(1, 1, OLFX_CH_PITCH, 1, &sw[0]), OLFX_OK);
        EXPECT_EQ(ch.set_range(1, 1, OLFX_CH_WINDOW, 1, &sw[1]), OLFX_OK);
        EXPECT_TRUE(record(ps, 1) == record(ch, 1));
        EXPECT_TRUE(record(ps, 1) != record(ps, 0));
    }
    {   /* chain = chorus | pitch-shift | reverb, word for word */
        Shadow cn = fresh(OLFX_KIND_CHAIN, 2);
        const float cp[OLFX_CH_NPARAMS] = {2.f, 0.3f, 0.7f, 0.6f, 0.25f, 0.4f, 0.9f, 5.f};
        const float pp[OLFX_PS_NPARAMS] = {0.75f, 8.f};
        const float vp[OLFX_DT_NPARAMS] = {0.5f, 0.8f, 0.7f, 0.6f, 0.65f, 0.3f, 0.9f};
        EXPECT_EQ(cn.set_range(1, 1, OLFX_CN_CHORUS0, OLFX_CH_NPARAMS, cp), OLFX_OK);
        EXPECT_EQ(cn.set_range(1, 1, OLFX_CN_PITCH0, OLFX_PS_NPARAMS, pp), OLFX_OK);
        EXPECT_EQ(cn.set_range(1, 1, OLFX_CN_VERB0, OLFX_DT_NPARAMS, vp), OLFX_OK);
        EXPECT_EQ(ch.set_range(0, 1, 0, OLFX_CH_NPARAMS, cp), OLFX_OK);
        EXPECT_EQ(ps.set_range(0, 1, 0, OLFX_PS_NPARAMS, pp), OLFX_OK);
        EXPECT_EQ(dt.set_range(0, 1, 0, OLFX_DT_NPARAMS, vp), OLFX_OK);
        std::vector<uint32_t> want = record(ch, 0);
        const std::vector<uint32_t> b = record(ps, 0), c = record(dt, 0);
        want.insert(want.end(), b.begin(), b.end());
        want.insert(want.end(), c.begin(), c.end());
        EXPECT_TRUE(record(cn, 1) == want);
    }
    {   /* rack: the longest delay stays inside the ring; a component has no master volume */
        Shadow fr = fresh(OLFX_KIND_FXRACK, 2);
        const float one = 1.0f, topo = 3.0f;
        EXPECT_EQ(fr.set_range(0, 1, OLFX_FR_DELAY_TIME, 1, &one), OLFX_OK);
        EXPECT_EQ(record(fr, 0)[FRC_DELAY], 47999u);
        EXPECT_EQ(record(fr, 0)[FRC_FRAC], bits(0.f));
        EXPECT_EQ(record(fr, 0)[FRC_MASTER], bits(0.8f));
        EXPECT_EQ(fr.set_range(0, 1, OLFX_FR_TOPOLOGY, 1, &topo), OLFX_OK);
        EXPECT_EQ(record(fr, 0)[FRC_MASTER], bits(1.0f));
        EXPECT_EQ(record(fr, 0)[FRC_TOPO], 3u);
    }
    for (const int kind : {OLFX_KIND_VOICE, OLFX_KIND_VOICE_MOOG}) {
        /* an unconfigured voice: daisysp Adsr::Init / Svf::Init (LadderFilter::Init) constants */
        Shadow vc = fresh(kind, 2);
        EXPECT_EQ(vc.update(1, 1), OLFX_OK);
        const std::vector<uint32_t> w = record(vc, 0), u = record(vc, 1);
        EXPECT_EQ(w[VCC_SUS_A], bits(0.7f));
        EXPECT_EQ(w[VCC_SUS_F], bits(0.7f));
        EXPECT_EQ(w[VCC_ATK_TGT_A], bits(1.01f));       /* shape 0 */
        EXPECT_EQ(w[VCC_ATK_TGT_F], bits(1.01f));
        EXPECT_TRUE(w[VCC_ATK_D0F] == w[VCC_ATK_D0A] && w[VCC_DEC_D0F] == w[VCC_DEC_D0A] && w[VCC_REL_D0F] == w[VCC_REL_D0A]);
        EXPECT_EQ(w[VCC_DEC_D0A], w[VCC_REL_D0A]);      /* both 0.1 s */
        /* 0.1 s at 48 kHz: d0 = 1 - exp(-1 / 4800) = 2.0831e-4.  expf's one ulp near 1 (6e-8) is
           3e-4 of that difference, so the bound is 1e-3 relative, not a few ulps */
        float d0;
        std::memcpy(&d0, &w[VCC_DEC_D0A], 4);
        EXPECT_TRUE(std::fabs(d0 - 2.0831165e-4) <= 1e-3 * 2.0831165e-4);
        if (kind == OLFX_KIND_VOICE) {
            EXPECT_EQ(w[VCC_DRIVE], bits(0.5f));
            EXPECT_EQ(w[VCC_DAMP_RES], bits(2.0f * (1.0f - powf(0.5f, 0.25f))));
        } else {
            EXPECT_EQ(w[VCC_LADDER_K], bits(4.0f * 0.2f));
            EXPECT_EQ(w[VCC_LADDER_DRIVE], bits(0.5f));
        }
        /* Update() ends the Init constants: the members' defaults (sustain 1 / 0 -> -0.01) */
        EXPECT_EQ(u[VCC_SUS_A], bits(1.0f));
        EXPECT_EQ(u[VCC_SUS_F], bits(-0.01f));
        EXPECT_EQ(u[VCC_AMP_AMT], w[VCC_AMP_AMT]);
    }
}

TEST(HostCore, RejectedCallsChangeNothing) {
    {
        Shadow s = fresh(OLFX_KIND_VOICE, 4);
        const Snapshot before(s);
        const float v[4] = {0.1f, 0.2f, NAN, 0.4f};
        EXPECT_EQ(s.set_range(0, 4, OLFX_VC_FILTER_CUTOFF, 1, v), OLFX_E_ARG);
        EXPECT_EQ(std::string(s.msg), std::string("olfx_set_params: non-finite value"));
        EXPECT_TRUE(before.same(s));
        const uint32_t inst[2] = {1, 2};
        EXPECT_EQ(s.set_list(OLFX_VC_FILTER_CUTOFF, inst, v + 1, 2), OLFX_E_ARG);
        EXPECT_EQ(std::string(s.msg), std::string("olfx_set_param_list: non-finite value"));
        EXPECT_TRUE(before.same(s));
        EXPECT_EQ(s.set_range(2, 3, 0, 1, v), OLFX_E_ARG);
        EXPECT_EQ(std::string(s.msg), std::string("olfx_set_params: range out of bounds"));
        EXPECT_TRUE(before.same(s));
    }
    {
        Shadow s = fresh(OLFX_KIND_DATTORRO, 4);
        s.pre_changed = false;
        const Snapshot before(s);
        const float v[2] = {0.5f, 14.0f};               /* 14 x 4800 >= 65536 */
        EXPECT_EQ(s.set_range(1, 2, OLFX_DT_PREDELAY, 1, v), OLFX_E_ARG);
        EXPECT_EQ(std::string(s.msg), std::string("olfx_set_params: pre-delay outside [0, 65536/4800)"));
        EXPECT_TRUE(before.same(s) && !s.pre_changed);
        EXPECT_TRUE(s.uniform_predelay());
        EXPECT_EQ(s.set_range(1, 1, OLFX_DT_PREDELAY, 1, v), OLFX_OK);
        EXPECT_TRUE(s.pre_changed && !s.uniform_predelay());
    }
    {
        Shadow s = fresh(OLFX_KIND_FXRACK, 4);
        const Snapshot before(s);
        const float v = 2.5f;
        EXPECT_EQ(s.set_range(0, 1, OLFX_FR_TOPOLOGY, 1, &v), OLFX_E_ARG);
        EXPECT_EQ(std::string(s.msg), std::string("olfx_set_params: rack topology must be 0, 1, 2, 3 or 4"));
        EXPECT_TRUE(before.same(s));
        /* the count of standalone components follows one instance's topology 0 -> 2 -> 3 -> 1 */
        const float topo[3] = {2.f, 3.f, 1.f};
        const int64_t want[3] = {1, 1, 0};
        for (int k = 0; k < 3; ++k) {
            EXPECT_EQ(s.set_range(2, 1, OLFX_FR_TOPOLOGY, 1, &topo[k]), OLFX_OK);
            EXPECT_EQ(s.n_components, want[k]);
        }
        EXPECT_EQ(s.dirty_list.size(), (size_t)1);      /* three changes, listed once */
    }
}

TEST(HostCore, DirtyListAndSetMember) {
    Shadow s = fresh(OLFX_KIND_VOICE, 4);
    EXPECT_EQ(s.update(2, 1), OLFX_OK);
    EXPECT_EQ(s.update(2, 1), OLFX_OK);
    EXPECT_TRUE(s.dirty_list == std::vector<uint32_t>{2});
    EXPECT_TRUE(s.configured == (std::vector<uint8_t>{0, 0, 1, 0}));
    /* before the first Update() every member may be written, and stays un-Update()d */
    EXPECT_EQ(s.set_member(0, OLFX_VC_AMP_ATTACK, 0.25f), OLFX_OK);
    EXPECT_EQ(s.configured[0], 0);
    EXPECT_EQ(s.params[(size_t)OLFX_VC_AMP_ATTACK * 4 + 0], 0.25f);
    EXPECT_TRUE(s.dirty_list == (std::vector<uint32_t>{2, 0}));
    /* on an Update()d voice: an envelope member is refused, what Process reads itself is taken */
    const Snapshot before(s);
    EXPECT_EQ(s.set_member(2, OLFX_VC_AMP_ATTACK, 0.25f), OLFX_E_STATE);
    EXPECT_EQ(std::string(s.msg), std::string("olfx_set_member: instance 2 is already Update()d (use olfx_set_params)"));
    EXPECT_TRUE(before.same(s));
    EXPECT_EQ(s.set_member(2, OLFX_VC_FILTER_CUTOFF, 1234.f), OLFX_OK);
    EXPECT_EQ(s.params[(size_t)OLFX_VC_FILTER_CUTOFF * 4 + 2], 1234.f);
    EXPECT_TRUE(s.configured == before.configured);
    EXPECT_EQ(s.set_member(4, OLFX_VC_FILTER_CUTOFF, 1.f), OLFX_E_ARG);
}

TEST(HostCore, RackControlRouting) {
    Shadow s = fresh(OLFX_KIND_FXRACK, 5);
    const float topo[5] = {0.f, 1.f, 2.f, 3.f, 4.f};   /* instance i has topology i */
    EXPECT_EQ(s.set_range(0, 5, OLFX_FR_TOPOLOGY, 1, topo), OLFX_OK);
    EXPECT_EQ(s.n_components, (int64_t)3);
    { const host::PacketPlan pl = s.plan(false); std::vector<uint32_t> b(pl.words); s.fill_records(pl, b.data()); }
    auto cc = [&](uint32_t inst, int control) {
        const olfx_control_event ev = {inst, (uint8_t)control, OLFX_CTL_MIDI, 0, 64.f};
        return s.control(&ev, 1);
    };
    auto param = [&](uint32_t field, uint32_t inst) { return s.params[(size_t)field * 5 + inst]; };
    const float unit = host::core_scale(64.f, 0.f, 127.f, 0.f, 1.f, 1.f);
    const float hz = host::core_scale(64.f, 0.f, 127.f, 0.f, 20000.f, 1.f);
    const Snapshot start(s);
    /* a DelayFx alone: its own CC 36, not the filter's 41 nor the reverb's 34 */
    EXPECT_EQ(cc(2, 41), OLFX_OK);
    EXPECT_EQ(cc(2, 34), OLFX_OK);
    EXPECT_TRUE(start.same(s));
    EXPECT_EQ(cc(2, 36), OLFX_OK);
    EXPECT_EQ(param(OLFX_FR_DELAY_FEEDBACK, 2), unit);
    EXPECT_TRUE(s.dirty_list == std::vector<uint32_t>{2});
    /* a FilterFx alone: the voice-filter CC 41 drives its cutoff */
    EXPECT_EQ(cc(4, 41), OLFX_OK);
    EXPECT_EQ(param(OLFX_FR_FILTER_CUTOFF, 4), hz);
    /* the firmware's callback: no FxRack, so no master volume */
    const Snapshot mid(s);
    EXPECT_EQ(cc(1, 7), OLFX_OK);
    EXPECT_TRUE(mid.same(s));
    /* FxRack: its own CC 45, not the voice filter's 41 */
    EXPECT_EQ(cc(0, 41), OLFX_OK);
    EXPECT_TRUE(mid.same(s));
    EXPECT_EQ(cc(0, 45), OLFX_OK);
    EXPECT_EQ(param(OLFX_FR_FILTER_CUTOFF, 0), hz);
    EXPECT_TRUE(s.dirty_list == (std::vector<uint32_t>{2, 4, 0}));
    EXPECT_EQ(cc(5, 45), OLFX_E_ARG);
    EXPECT_EQ(std::string(s.msg), std::string("olfx_control: event 0: instance out of range"));
}

int main() { return run_all_tests(); }
