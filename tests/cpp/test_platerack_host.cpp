/*
 * tests/cpp/test_platerack_host.cpp -- OLFX_KIND_PLATERACK in the engine's HIP-free host core
 * (ol_dsp_amd/csrc/olfx_host.h) on the CPU: the kind tables, the defaults, the coefficient record
 * (rack record, then plate record), the reverb CC table for both sources, the refused topologies and
 * the plate's validation.  Links olfx_host.cpp directly (no libolfx.so, no GPU); built by
 * tests/test_platerack_host.py with its own build line.
 */
#include "../../ol_dsp_amd/csrc/olfx_host.h"
#include "harness.h"

using namespace olfx;
using host::Shadow;

namespace {

constexpr int K = OLFX_KIND_PLATERACK;
constexpr uint32_t V = OLFX_PR_VERB0;
enum : uint8_t {
    CC_VOLUME = 7, CC_REVERB_TIME = 32, CC_REVERB_CUTOFF = 33, CC_REVERB_BALANCE = 34, CC_DELAY_TIME = 35,
    CC_FILTER_CUTOFF = 41, CC_FX_FILTER_CUTOFF = 45, CC_EARLY_PREDELAY = 50, CC_REVERB_PREDELAY = 52,
    CC_REVERB_PREFILTER = 53, CC_REVERB_INPUT_DIFFUSION_1 = 54, CC_REVERB_INPUT_DIFFUSION_2 = 55,
    CC_REVERB_DECAY_DIFFUSION = 56,
};

Shadow fresh(int kind, uint32_t n) {
    Shadow s;
    s.init(kind, n, 48000.f);
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

float param(const Shadow &s, uint32_t field, uint32_t inst) { return s.params[(size_t)field * s.n + inst]; }

/* ol::core::scale(value, 0, 127, 0, 1, 1), as UpdateMidiControl's `scaled` */
float midi_unit(float v) { return host::core_scale(v, 0.f, 127.f, 0.f, 1.f, 1.f); }

}  // namespace

TEST(PlateRack, TablesAndDefaults) {
    EXPECT_EQ(OLFX_KIND_PLATERACK, 8);
    EXPECT_EQ(OLFX_ABI_VERSION, 2);
    EXPECT_EQ(OLFX_PR_RACK0, 0);
    EXPECT_EQ((uint32_t)OLFX_PR_VERB0, (uint32_t)OLFX_FR_NPARAMS);
    EXPECT_EQ(host::n_params_of(K), (uint32_t)(OLFX_FR_NPARAMS + OLFX_DT_NPARAMS));
    EXPECT_EQ(host::in_channels(K), 2u);
    EXPECT_EQ(host::out_channels(K), 2u);

    float p[OLFX_PR_NPARAMS], fr[OLFX_FR_NPARAMS], dt[OLFX_DT_NPARAMS];
    host::default_params(K, p);
    host::default_params(OLFX_KIND_FXRACK, fr);
    host::default_params(OLFX_KIND_DATTORRO, dt);
    EXPECT_TRUE(std::memcmp(p, fr, sizeof fr) == 0);                   /* rack fields: as the rack */
    /* the five members the glue forwards inside their setter's domain (Fx.h:274-281) */
    EXPECT_EQ(p[V + OLFX_DT_DECAY], 0.5f);
    EXPECT_EQ(p[V + OLFX_DT_PREFILTER], 0.5f);
    EXPECT_EQ(p[V + OLFX_DT_INPUT_DIFFUSION1], 0.5f);
    EXPECT_EQ(p[V + OLFX_DT_INPUT_DIFFUSION2], 0.5f);
    EXPECT_EQ(p[V + OLFX_DT_DECAY_DIFFUSION], 0.5f);
    /* DattorroVerb_create's own (verb.cpp:215-221) */
    EXPECT_EQ(p[V + OLFX_DT_DAMPING], dt[OLFX_DT_DAMPING]);
    EXPECT_EQ(p[V + OLFX_DT_DAMPING], (float)0.95);
    EXPECT_EQ(p[V + OLFX_DT_PREDELAY], dt[OLFX_DT_PREDELAY]);
    EXPECT_EQ(p[V + OLFX_DT_PREDELAY], (float)0.1);

    /* the rack's state, plus the plate's with its instances rounded up to 64 */
    for (uint32_t n : {1u, 64u, 65u, 130u}) {
        const uint64_t pad = (n + 63u) & ~63u;
        EXPECT_EQ(host::state_bytes(K, n, 48000.f),
                  host::state_bytes(OLFX_KIND_FXRACK, n, 48000.f) + host::state_bytes(OLFX_KIND_DATTORRO, (uint32_t)pad, 48000.f));
    }
    const host::Segments sg = host::coef_segments(K);
    EXPECT_EQ(sg.nseg, 2u);
    EXPECT_EQ(sg.words[0], (uint32_t)FRC_N);
    EXPECT_EQ(sg.words[1], (uint32_t)DTC_N);
    EXPECT_TRUE(std::fabs(host::algorithmic_bytes_per_frame(K) - 180.6) < 1e-9);
    EXPECT_TRUE(std::fabs(host::algorithmic_read_bytes_per_frame(K) - (16.0 + 6445.0 * 4.0 / 256.0)) < 1e-9);
}

TEST(PlateRack, RecordIsRackThenPlate) {
    const uint32_t n = 3;
    Shadow pr = fresh(K, n), fr = fresh(OLFX_KIND_FXRACK, n), dt = fresh(OLFX_KIND_DATTORRO, n);
    Lcg rng(11);
    for (uint32_t i = 0; i < n; ++i) {
        float rack[OLFX_FR_NPARAMS], plate[OLFX_DT_NPARAMS];
        for (float &v : rack) v = rng.uni(0.f, 1.f);
        rack[OLFX_FR_DELAY_CUTOFF] = rng.uni(100.f, 12000.f);
        rack[OLFX_FR_FILTER_CUTOFF] = rng.uni(100.f, 12000.f);
        rack[OLFX_FR_FILTER_TYPE] = (float)(i % 5);
        rack[OLFX_FR_TOPOLOGY] = (float)(i % 2);
        for (float &v : plate) v = rng.uni(0.f, 1.f);
        EXPECT_EQ(pr.set_range(i, 1, OLFX_PR_RACK0, OLFX_FR_NPARAMS, rack), OLFX_OK);
        EXPECT_EQ(pr.set_range(i, 1, OLFX_PR_VERB0, OLFX_DT_NPARAMS, plate), OLFX_OK);
        EXPECT_EQ(fr.set_range(i, 1, 0, OLFX_FR_NPARAMS, rack), OLFX_OK);
        EXPECT_EQ(dt.set_range(i, 1, 0, OLFX_DT_NPARAMS, plate), OLFX_OK);
    }
    for (uint32_t i = 0; i < n; ++i) {
        const std::vector<uint32_t> w = record(pr, i), wr = record(fr, i), wd = record(dt, i);
        EXPECT_EQ(w.size(), wr.size() + wd.size());
        EXPECT_TRUE(std::equal(wr.begin(), wr.end(), w.begin()));
        EXPECT_TRUE(std::equal(wd.begin(), wd.end(), w.begin() + (long)wr.size()));
    }
    /* the defaults too */
    Shadow d = fresh(K, 1), dr = fresh(OLFX_KIND_FXRACK, 1);
    const std::vector<uint32_t> w = record(d, 0), wr = record(dr, 0);
    EXPECT_TRUE(std::equal(wr.begin(), wr.end(), w.begin()));
}

TEST(PlateRack, ReverbControlTable) {
    struct Row { uint8_t cc; uint32_t field; };
    const Row rows[] = {
        {CC_REVERB_TIME, V + OLFX_DT_DECAY},
        {CC_REVERB_PREFILTER, V + OLFX_DT_PREFILTER},
        {CC_REVERB_INPUT_DIFFUSION_1, V + OLFX_DT_INPUT_DIFFUSION1},
        {CC_REVERB_DECAY_DIFFUSION, V + OLFX_DT_DECAY_DIFFUSION},
        {CC_REVERB_INPUT_DIFFUSION_2, V + OLFX_DT_DECAY_DIFFUSION},   /* the reference's quirk, Fx.h:323-324 */
        {CC_REVERB_BALANCE, OLFX_FR_REVERB_BALANCE},
        {CC_REVERB_CUTOFF, V + OLFX_DT_DAMPING},                      /* the 0..1 form */
        {CC_REVERB_PREDELAY, OLFX_FIELD_UPDATE_ONLY},
        {CC_EARLY_PREDELAY, OLFX_FIELD_UPDATE_ONLY},
    };
    for (const Row &r : rows) {
        for (float mv : {0.f, 1.f, 37.f, 64.f, 127.f}) {              /* MIDI: scaled 0..1 */
            uint32_t field = 12345;
            float v = -1.f;
            EXPECT_EQ(olfx_control_map(K, r.cc, OLFX_CTL_MIDI, mv, &field, &v), OLFX_OK);
            EXPECT_EQ(field, r.field);
            EXPECT_EQ(v, midi_unit(mv));
        }
        for (float hv : {0.f, 0.25f, 0.8125f, 1.f}) {                 /* hardware: as given */
            uint32_t field = 12345;
            float v = -1.f;
            EXPECT_EQ(olfx_control_map(K, r.cc, OLFX_CTL_HARDWARE, hv, &field, &v), OLFX_OK);
            EXPECT_EQ(field, r.field);
            EXPECT_EQ(v, hv);
        }
        /* the plain rack still ignores every reverb CC but the balance */
        uint32_t field;
        float v;
        EXPECT_EQ(olfx_control_map(OLFX_KIND_FXRACK, r.cc, OLFX_CTL_MIDI, 64.f, &field, &v),
                  r.cc == CC_REVERB_BALANCE ? OLFX_OK : OLFX_IGNORED);
    }
    /* delay, filter and volume controls: as the rack maps them */
    for (int cc = 0; cc < 128; ++cc) {
        bool reverb = false;
        for (const Row &r : rows) reverb = reverb || r.cc == cc;
        if (reverb) continue;
        for (int src : {OLFX_CTL_MIDI, OLFX_CTL_HARDWARE}) {
            uint32_t f1 = 1, f2 = 2;
            float v1 = 1.f, v2 = 2.f;
            const int r1 = olfx_control_map(K, (uint8_t)cc, src, 0.3f, &f1, &v1);
            const int r2 = olfx_control_map(OLFX_KIND_FXRACK, (uint8_t)cc, src, 0.3f, &f2, &v2);
            EXPECT_EQ(r1, r2);
            if (r1 == OLFX_OK) { EXPECT_EQ(f1, f2); EXPECT_EQ(v1, v2); }
        }
    }
}

TEST(PlateRack, ControlThroughTheShadow) {
    Shadow s = fresh(K, 4);
    const olfx_control_event evs[] = {
        {0, CC_REVERB_TIME, OLFX_CTL_MIDI, 0, 100.f},
        {1, CC_REVERB_INPUT_DIFFUSION_2, OLFX_CTL_HARDWARE, 0, 0.3f},
        {2, CC_REVERB_CUTOFF, OLFX_CTL_MIDI, 0, 20.f},
        {3, CC_REVERB_BALANCE, OLFX_CTL_HARDWARE, 0, 0.75f},
    };
    EXPECT_EQ(s.control(evs, 4), OLFX_OK);
    EXPECT_EQ(param(s, V + OLFX_DT_DECAY, 0), midi_unit(100.f));
    EXPECT_EQ(param(s, V + OLFX_DT_DECAY_DIFFUSION, 1), 0.3f);
    EXPECT_EQ(param(s, V + OLFX_DT_INPUT_DIFFUSION2, 1), 0.5f);        /* untouched: the quirk */
    EXPECT_EQ(param(s, V + OLFX_DT_DAMPING, 2), midi_unit(20.f));
    EXPECT_EQ(param(s, OLFX_FR_REVERB_BALANCE, 3), 0.75f);
    EXPECT_EQ(s.dirty_list.size(), (size_t)4);

    /* the two update-only controls: Update() with unchanged members */
    Shadow u = fresh(K, 2);
    const std::vector<float> before = u.params;
    const olfx_control_event upd[] = {{1, CC_REVERB_PREDELAY, OLFX_CTL_MIDI, 0, 90.f},
                                      {1, CC_EARLY_PREDELAY, OLFX_CTL_HARDWARE, 0, 0.9f}};
    EXPECT_EQ(u.control(upd, 2), OLFX_OK);
    EXPECT_TRUE(u.params == before);
    EXPECT_EQ(u.dirty_list.size(), (size_t)1);
    EXPECT_EQ(u.dirty_list[0], 1u);

    /* topology 1 (the firmware: every CC goes to delay_fx, reverb_fx and filter_fx directly): the
       reverb CCs reach the plate, the voice-filter CCs drive FILTER_*, CCs 45-48 and 7 reach nothing */
    Shadow f = fresh(K, 1);
    const float one = 1.f;
    EXPECT_EQ(f.set_range(0, 1, OLFX_FR_TOPOLOGY, 1, &one), OLFX_OK);
    const olfx_control_event fw[] = {
        {0, CC_REVERB_PREFILTER, OLFX_CTL_MIDI, 0, 10.f},
        {0, CC_FILTER_CUTOFF, OLFX_CTL_MIDI, 0, 64.f},
        {0, CC_FX_FILTER_CUTOFF, OLFX_CTL_MIDI, 0, 1.f},
        {0, CC_VOLUME, OLFX_CTL_MIDI, 0, 1.f},
        {0, CC_DELAY_TIME, OLFX_CTL_MIDI, 0, 127.f},
    };
    EXPECT_EQ(f.control(fw, 5), OLFX_OK);
    EXPECT_EQ(param(f, V + OLFX_DT_PREFILTER, 0), midi_unit(10.f));
    EXPECT_EQ(param(f, OLFX_FR_FILTER_CUTOFF, 0), host::core_scale(64.f, 0.f, 127.f, 0.f, 20000.f, 1.f));
    EXPECT_EQ(param(f, OLFX_FR_MASTER_VOLUME, 0), 0.8f);
    EXPECT_EQ(param(f, OLFX_FR_DELAY_TIME, 0), midi_unit(127.f));
}

TEST(PlateRack, RefusedValuesChangeNothing) {
    Shadow s = fresh(K, 3);
    const std::vector<float> before = s.params;
    for (float t : {2.f, 3.f, 4.f, 5.f, -1.f, 0.5f}) {
        EXPECT_EQ(s.set_range(1, 1, OLFX_FR_TOPOLOGY, 1, &t), OLFX_E_ARG);
        const uint32_t inst = 2;
        EXPECT_EQ(s.set_list(OLFX_FR_TOPOLOGY, &inst, &t, 1), OLFX_E_ARG);
    }
    /* a whole-row write with one bad value: nothing of it lands */
    float row[OLFX_PR_NPARAMS];
    host::default_params(K, row);
    row[OLFX_FR_DELAY_TIME] = 0.9f;
    row[OLFX_FR_TOPOLOGY] = 2.f;
    EXPECT_EQ(s.set_range(0, 1, 0, OLFX_PR_NPARAMS, row), OLFX_E_ARG);
    /* the plate's fields, as OLFX_KIND_DATTORRO validates them */
    const float nan = std::nanf(""), big = 65536.0f / 4800.0f, neg = -0.01f, inf = INFINITY;
    EXPECT_EQ(s.set_range(0, 1, V + OLFX_DT_DECAY, 1, &nan), OLFX_E_ARG);
    EXPECT_EQ(s.set_range(0, 1, V + OLFX_DT_DAMPING, 1, &inf), OLFX_E_ARG);
    EXPECT_EQ(s.set_range(0, 1, V + OLFX_DT_PREDELAY, 1, &big), OLFX_E_ARG);
    EXPECT_EQ(s.set_range(0, 1, V + OLFX_DT_PREDELAY, 1, &neg), OLFX_E_ARG);
    EXPECT_EQ(s.set_range(0, 1, OLFX_PR_NPARAMS, 1, &neg), OLFX_E_ARG);      /* past the last field */
    Shadow d = fresh(OLFX_KIND_DATTORRO, 1);
    EXPECT_EQ(d.set_range(0, 1, OLFX_DT_PREDELAY, 1, &big), OLFX_E_ARG);
    EXPECT_TRUE(s.params == before);
    EXPECT_TRUE(s.dirty_list.empty());
    /* the accepted ones land */
    const float ok = 13.0f;                                                   /* 62,400 samples: < 65,536 */
    EXPECT_EQ(s.set_range(0, 1, V + OLFX_DT_PREDELAY, 1, &ok), OLFX_OK);
    const float t1 = 1.f;
    EXPECT_EQ(s.set_range(1, 1, OLFX_FR_TOPOLOGY, 1, &t1), OLFX_OK);
    EXPECT_EQ(param(s, OLFX_FR_TOPOLOGY, 1), 1.f);
}

int main() { return run_all_tests(); }
