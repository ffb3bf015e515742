/*
 * tests/cpp/test_synth_svf_host.cpp -- OLFX_KIND_SYNTH_SVF in the engine's HIP-free host core
 * (ol_dsp_amd/csrc/olfx_host.h) on the CPU: the kind tables and defaults, the coefficient record (the Svf
 * voice's record, then the rack's at the instrument's topology), topology 0 / 1 accepted and everything
 * else refused, the Polyvoice router shared with OLFX_KIND_SYNTH, the control fan-out by topology and
 * olfx_synth_control_map_at.  Links olfx_host.cpp directly (no libolfx.so, no GPU); built by
 * tests/test_synth_svf_host.py with its own build line.
 */
#include "../../ol_dsp_amd/csrc/olfx_host.h"
#include "harness.h"

using namespace olfx;
using host::Shadow;

namespace {

constexpr int K = OLFX_KIND_SYNTH_SVF;
constexpr uint32_t V0 = OLFX_SY_VOICE0, R0 = OLFX_SY_RACK0;
enum : uint8_t {
    CC_VOLUME = 7, CC_REVERB_TIME = 32, CC_REVERB_BALANCE = 34, CC_DELAY_TIME = 35, CC_DELAY_CUTOFF = 37,
    CC_FILTER_CUTOFF = 41, CC_FILTER_DRIVE = 44, CC_FX_FILTER_CUTOFF = 45, CC_FX_FILTER_TYPE = 47, CC_ENV_FILT_D = 75,
    CC_OSC_1_VOLUME = 114,
};

Shadow fresh(uint32_t n, uint32_t voices = 4, int kind = K) {
    Shadow s;
    s.init(kind, n, 48000.f, voices);
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

std::vector<uint8_t> playing(Shadow &s, uint32_t inst) {
    std::vector<uint8_t> p(s.voices, 0xEE);
    EXPECT_EQ(s.synth_playing(inst, p.data()), OLFX_OK);
    return p;
}

int note(Shadow &s, uint32_t inst, uint8_t type, uint8_t n) {
    const olfx_event e{inst, type, n, 100, 0};
    return s.note_events(&e, 1);
}

}  // namespace

TEST(SynthSvf, TablesAndDefaults) {
    EXPECT_EQ(OLFX_KIND_SYNTH_SVF, 12);
    EXPECT_EQ(OLFX_ABI_VERSION, 2);
    EXPECT_TRUE(is_synth_kind(K) && is_synth_kind(OLFX_KIND_SYNTH) && !is_synth_kind(OLFX_KIND_VOICE));
    EXPECT_EQ(host::n_params_of(K), 28u);
    EXPECT_EQ(host::in_channels(K), 0u);
    EXPECT_EQ(host::out_channels(K), 2u);
    EXPECT_TRUE(!is_voice_kind(K));
    EXPECT_TRUE(host::takes_note_events(K));
    EXPECT_EQ(host::n_params_of(13), 0u);

    float p[OLFX_SY_NPARAMS], vc[OLFX_VC_NPARAMS], fr[OLFX_FR_NPARAMS];
    host::default_params(K, p);
    host::default_params(OLFX_KIND_VOICE, vc);
    host::default_params(OLFX_KIND_FXRACK, fr);
    EXPECT_TRUE(std::memcmp(p + V0, vc, sizeof vc) == 0);
    fr[OLFX_FR_TOPOLOGY] = 1.f;
    EXPECT_TRUE(std::memcmp(p + R0, fr, sizeof fr) == 0);

    /* the synth's formula with OLFX_KIND_VOICE's per-voice figures */
    const uint64_t rack = host::state_bytes(OLFX_KIND_FXRACK, 1, 48000.f);
    EXPECT_EQ(host::state_bytes(K, 1, 48000.f), rack + VCC_N * 4 + 4ull * VCS_N * 4);
    EXPECT_EQ(host::state_bytes(K, 1, 48000.f),
              rack + VCC_N * 4 + 4ull * (host::state_bytes(OLFX_KIND_VOICE, 1, 48000.f) - VCC_N * 4));
    EXPECT_EQ(host::state_bytes(K, 7, 48000.f), 7 * host::state_bytes(K, 1, 48000.f));
    EXPECT_EQ(voice_state_slots(K), (uint32_t)VCS_N);
    EXPECT_EQ(voice_state_slots(OLFX_KIND_SYNTH), (uint32_t)VCS_N_MOOG);
    const host::Segments sg = host::coef_segments(K);
    EXPECT_EQ(sg.nseg, 2u);
    EXPECT_EQ(sg.words[0], (uint32_t)VCC_N);
    EXPECT_EQ(sg.words[1], (uint32_t)FRC_N);
    EXPECT_TRUE(std::fabs(host::algorithmic_bytes_per_frame(K) - 24.0) < 1e-9);
    EXPECT_TRUE(std::fabs(host::algorithmic_read_bytes_per_frame(K) - 8.0) < 1e-9);

    Shadow s = fresh(65, 5);
    EXPECT_EQ(s.voices, 5u);
    EXPECT_EQ(s.npad, 128u);
    EXPECT_EQ(s.n_ev(), 640u);
    EXPECT_TRUE(host::max_packet_words(K, 65, s.n_ev()) == host::max_packet_words(OLFX_KIND_SYNTH, 65, s.n_ev()));
}

TEST(SynthSvf, RecordIsSvfVoiceThenRackAtTheTopology) {
    const uint32_t n = 4;
    Shadow sy = fresh(n), vc = fresh(n, 4, OLFX_KIND_VOICE), fr = fresh(n, 4, OLFX_KIND_FXRACK);
    const float one = 1.f;
    for (uint32_t i = 0; i < n; ++i) EXPECT_EQ(fr.set_range(i, 1, OLFX_FR_TOPOLOGY, 1, &one), OLFX_OK);
    {
        const std::vector<uint32_t> w = record(sy, 0), wv = record(vc, 0), wr = record(fr, 0);
        EXPECT_EQ(w.size(), wv.size() + wr.size());
        EXPECT_TRUE(std::equal(wv.begin(), wv.end(), w.begin()));
        EXPECT_TRUE(std::equal(wr.begin(), wr.end(), w.begin() + (long)wv.size()));
    }
    Lcg rng(9);
    for (uint32_t i = 0; i < n; ++i) {
        float v[OLFX_VC_NPARAMS], r[OLFX_FR_NPARAMS];
        for (float &x : v) x = rng.uni(0.01f, 0.9f);
        v[OLFX_VC_FILTER_CUTOFF] = rng.uni(100.f, 8000.f);
        for (float &x : r) x = rng.uni(0.f, 1.f);
        r[OLFX_FR_DELAY_CUTOFF] = rng.uni(100.f, 12000.f);
        r[OLFX_FR_FILTER_CUTOFF] = rng.uni(100.f, 12000.f);
        r[OLFX_FR_FILTER_TYPE] = (float)(i % 5);
        r[OLFX_FR_MASTER_VOLUME] = 0.3f + 0.1f * (float)i;
        r[OLFX_FR_TOPOLOGY] = (float)(i & 1u);
        EXPECT_EQ(sy.set_range(i, 1, V0, OLFX_VC_NPARAMS, v), OLFX_OK);
        EXPECT_EQ(sy.set_range(i, 1, R0, OLFX_FR_NPARAMS, r), OLFX_OK);
        EXPECT_EQ(vc.set_range(i, 1, 0, OLFX_VC_NPARAMS, v), OLFX_OK);
        EXPECT_EQ(fr.set_range(i, 1, 0, OLFX_FR_NPARAMS, r), OLFX_OK);
    }
    for (uint32_t i = 0; i < n; ++i) {
        const std::vector<uint32_t> w = record(sy, i), wv = record(vc, i), wr = record(fr, i);
        EXPECT_TRUE(std::equal(wv.begin(), wv.end(), w.begin()));
        EXPECT_TRUE(std::equal(wr.begin(), wr.end(), w.begin() + (long)wv.size()));
        float master;
        std::memcpy(&master, &w[VCC_N + FRC_MASTER], 4);
        EXPECT_EQ(w[VCC_N + FRC_TOPO], i & 1u);
        /* MASTER_VOLUME: live at topology 0, stored and ignored (x 1.0f) at topology 1 */
        EXPECT_EQ(master, (i & 1u) ? 1.0f : 0.3f + 0.1f * (float)i);
        EXPECT_EQ(param(sy, R0 + OLFX_FR_MASTER_VOLUME, i), 0.3f + 0.1f * (float)i);
    }
    /* FILTER_DRIVE is live (SvfFilter::SetDrive): it moves the record, which the Moog synth's ignores */
    Shadow a = fresh(1), m = fresh(1, 4, OLFX_KIND_SYNTH);
    const float res = 0.5f, d0 = 0.f, d1 = 0.8f;
    for (Shadow *s : {&a, &m}) {
        EXPECT_EQ(s->set_range(0, 1, V0 + OLFX_VC_FILTER_RESONANCE, 1, &res), OLFX_OK);
        EXPECT_EQ(s->set_range(0, 1, V0 + OLFX_VC_FILTER_DRIVE, 1, &d0), OLFX_OK);
    }
    const std::vector<uint32_t> a0 = record(a, 0), m0 = record(m, 0);
    EXPECT_EQ(a.set_range(0, 1, V0 + OLFX_VC_FILTER_DRIVE, 1, &d1), OLFX_OK);
    EXPECT_EQ(m.set_range(0, 1, V0 + OLFX_VC_FILTER_DRIVE, 1, &d1), OLFX_OK);
    EXPECT_TRUE(record(a, 0) != a0);
    EXPECT_TRUE(record(m, 0) == m0);
}

TEST(SynthSvf, TopologyZeroAndOneAcceptedOthersRefused) {
    Shadow s = fresh(3);
    const float zero = 0.f, one = 1.f;
    EXPECT_EQ(s.set_range(1, 1, R0 + OLFX_FR_TOPOLOGY, 1, &zero), OLFX_OK);
    EXPECT_EQ(param(s, R0 + OLFX_FR_TOPOLOGY, 1), 0.f);
    EXPECT_EQ(param(s, R0 + OLFX_FR_TOPOLOGY, 0), 1.f);                 /* per instrument */
    EXPECT_EQ(s.n_components, 0);
    EXPECT_EQ(s.set_member(1, R0 + OLFX_FR_TOPOLOGY, 1.f), OLFX_OK);
    const uint32_t inst = 2;
    EXPECT_EQ(s.set_list(R0 + OLFX_FR_TOPOLOGY, &inst, &zero, 1), OLFX_OK);
    EXPECT_EQ(s.set_list(R0 + OLFX_FR_TOPOLOGY, &inst, &one, 1), OLFX_OK);
    {
        const host::PacketPlan pl = s.plan(false);
        std::vector<uint32_t> buf(pl.words);
        s.fill_records(pl, buf.data());
    }
    const std::vector<float> before = s.params;
    for (float t : {2.f, -1.f, 0.5f, 3.f, 4.f, 5.f}) {
        EXPECT_EQ(s.set_range(1, 1, R0 + OLFX_FR_TOPOLOGY, 1, &t), OLFX_E_ARG);
        EXPECT_EQ(s.set_list(R0 + OLFX_FR_TOPOLOGY, &inst, &t, 1), OLFX_E_ARG);
        EXPECT_EQ(s.set_member(0, R0 + OLFX_FR_TOPOLOGY, t), OLFX_E_ARG);
    }
    float row[OLFX_SY_NPARAMS];
    host::default_params(K, row);
    row[V0 + OLFX_VC_FILTER_CUTOFF] = 900.f;
    row[R0 + OLFX_FR_TOPOLOGY] = 2.f;
    EXPECT_EQ(s.set_range(0, 1, 0, OLFX_SY_NPARAMS, row), OLFX_E_ARG);   /* nothing of the row lands */
    EXPECT_TRUE(s.params == before);
    EXPECT_TRUE(s.dirty_list.empty());
    row[R0 + OLFX_FR_TOPOLOGY] = 0.f;
    EXPECT_EQ(s.set_range(0, 1, 0, OLFX_SY_NPARAMS, row), OLFX_OK);
    EXPECT_EQ(param(s, V0 + OLFX_VC_FILTER_CUTOFF, 0), 900.f);
    /* OLFX_KIND_SYNTH itself still refuses 0 */
    Shadow m = fresh(2, 4, OLFX_KIND_SYNTH);
    EXPECT_EQ(m.set_range(0, 1, R0 + OLFX_FR_TOPOLOGY, 1, &zero), OLFX_E_ARG);
    EXPECT_EQ(param(m, R0 + OLFX_FR_TOPOLOGY, 0), 1.f);
}

TEST(SynthSvf, RouterAndPlayingAsTheSynth) {
    const uint32_t n = 70;
    Shadow s = fresh(n), m = fresh(n, 4, OLFX_KIND_SYNTH);
    const uint32_t i = 65;
    for (Shadow *e : {&s, &m}) {
        for (uint8_t k : {60, 64, 67, 70, 72}) EXPECT_EQ(note(*e, i, OLFX_EV_NOTE_ON, k), OLFX_OK);   /* the fifth: dropped */
        EXPECT_EQ(note(*e, i, OLFX_EV_NOTE_OFF, 64), OLFX_OK);
        EXPECT_EQ(note(*e, i, OLFX_EV_NOTE_ON, 0), OLFX_OK);            /* gates voice 1, which stays free */
        EXPECT_EQ(note(*e, i, OLFX_EV_NOTE_ON, 71), OLFX_OK);
        EXPECT_EQ(note(*e, 3, OLFX_EV_GATE_ON, 0), OLFX_OK);
    }
    EXPECT_TRUE((playing(s, i) == std::vector<uint8_t>{60, 71, 67, 70}));
    EXPECT_TRUE(playing(s, i) == playing(m, i));
    EXPECT_EQ(s.events.size(), m.events.size());
    EXPECT_EQ(s.events.size(), (size_t)(4 + 1 + 1 + 1 + 4));
    for (size_t k = 0; k < s.events.size() && k < m.events.size(); ++k) {
        EXPECT_EQ(s.events[k].inst, m.events[k].inst);
        EXPECT_EQ(s.events[k].type, m.events[k].type);
        EXPECT_EQ(s.events[k].note, m.events[k].note);
    }
    EXPECT_EQ(s.events[1].inst, 1u * 128u + i);                          /* voice slot p npad + inst */
    const olfx_voice_event sf{2, OLFX_EV_SET_FREQUENCY, 0, 0, 0, 440.f};
    const size_t nq = s.events.size();
    EXPECT_EQ(s.voice_events(&sf, 1), OLFX_OK);                          /* accepted, does nothing */
    EXPECT_EQ(s.events.size(), nq);
    s.fold_events();
    EXPECT_EQ(s.ev_count.size(), (size_t)(4 * 128 / 64));
    s.reset();
    EXPECT_TRUE((playing(s, i) == std::vector<uint8_t>{0, 0, 0, 0}));
    EXPECT_EQ(param(s, R0 + OLFX_FR_TOPOLOGY, 0), 1.f);
    /* the refused entry points */
    host::BankPlan plan;
    const uint64_t off[2] = {0, 4};
    const float pcm[4] = {0, 0, 0, 0};
    EXPECT_EQ(s.bank_plan(1, off, pcm, &plan), OLFX_E_STATE);
    const olfx_sample_voice rec{0, OLFX_NO_SAMPLE, 0, 0, 0, 0};
    EXPECT_EQ(s.sample_voices(&rec, 1), OLFX_E_STATE);
}

TEST(SynthSvf, ControlMapAtBothTopologies) {
    uint32_t f[2], g[2], f1;
    float v[2], w[2], v1;
    const uint8_t ccs[] = {3, 5, 7, 32, 34, 35, 36, 37, 38, 39, 41, 42, 44, 45, 46, 47, 48, 73, 75, 108, 114, 120};
    for (int source : {OLFX_CTL_MIDI, OLFX_CTL_HARDWARE})
        for (uint8_t cc : ccs) {
            const float val = source == OLFX_CTL_MIDI ? 77.f : 0.6f;
            /* kind 11 at topology 1 is olfx_synth_control_map */
            f[0] = f[1] = g[0] = g[1] = 99;
            v[0] = v[1] = w[0] = w[1] = -1.f;
            const int h11 = olfx_synth_control_map(cc, source, val, f, v);
            EXPECT_EQ(olfx_synth_control_map_at(OLFX_KIND_SYNTH, 1, cc, source, val, g, w), h11);
            EXPECT_TRUE(std::memcmp(f, g, sizeof f) == 0 && std::memcmp(v, w, sizeof v) == 0);
            /* kind 12: the voice's table (OLFX_KIND_VOICE), then the rack's at the topology */
            for (uint32_t topo : {0u, 1u}) {
                int want = 0;
                uint32_t wf[2] = {99, 99};
                float wv[2] = {-1.f, -1.f};
                if (olfx_control_map(OLFX_KIND_VOICE, cc, source, val, &f1, &v1) == OLFX_OK) {
                    wf[want] = f1 == OLFX_FIELD_UPDATE_ONLY ? f1 : V0 + f1;
                    wv[want++] = v1;
                }
                uint8_t as = cc;
                bool takes = true;
                if (topo == 1u) {                                      /* the firmware's direct routing */
                    const bool filter_cc = cc >= 41 && cc <= 44;
                    takes = filter_cc || (cc >= 35 && cc <= 39) || cc == 34;
                    if (filter_cc) as = (uint8_t)(cc + 4);
                }
                if (takes && olfx_control_map(OLFX_KIND_FXRACK, as, source, val, &f1, &v1) == OLFX_OK) {
                    wf[want] = R0 + f1;
                    wv[want++] = v1;
                }
                f[0] = f[1] = 99;
                v[0] = v[1] = -1.f;
                EXPECT_EQ(olfx_synth_control_map_at(K, topo, cc, source, val, f, v), want);
                EXPECT_TRUE(std::memcmp(f, wf, sizeof f) == 0 && std::memcmp(v, wv, sizeof v) == 0);
            }
        }
    /* the cases by hand: CC 41 hits both filters at topology 1 and the voice's alone at topology 0 ... */
    EXPECT_EQ(olfx_synth_control_map_at(K, 1, CC_FILTER_CUTOFF, OLFX_CTL_MIDI, 64.f, f, v), 2);
    EXPECT_EQ(f[0], V0 + OLFX_VC_FILTER_CUTOFF);
    EXPECT_EQ(f[1], R0 + OLFX_FR_FILTER_CUTOFF);
    EXPECT_EQ(olfx_synth_control_map_at(K, 0, CC_FILTER_CUTOFF, OLFX_CTL_MIDI, 64.f, f, v), 1);
    EXPECT_EQ(f[0], V0 + OLFX_VC_FILTER_CUTOFF);
    /* ... CC 44 is SvfFilter's drive, live on this kind */
    EXPECT_EQ(olfx_synth_control_map_at(K, 0, CC_FILTER_DRIVE, OLFX_CTL_HARDWARE, 0.4f, f, v), 1);
    EXPECT_EQ(f[0], V0 + OLFX_VC_FILTER_DRIVE);
    /* ... the rack's own filter CCs and the volume reach FxRack's handlers at topology 0 only */
    EXPECT_EQ(olfx_synth_control_map_at(K, 0, CC_FX_FILTER_CUTOFF, OLFX_CTL_MIDI, 64.f, f, v), 1);
    EXPECT_EQ(f[0], R0 + OLFX_FR_FILTER_CUTOFF);
    EXPECT_EQ(olfx_synth_control_map_at(K, 1, CC_FX_FILTER_CUTOFF, OLFX_CTL_MIDI, 64.f, f, v), 0);
    EXPECT_EQ(olfx_synth_control_map_at(K, 0, CC_VOLUME, OLFX_CTL_MIDI, 80.f, f, v), 2);
    EXPECT_EQ(f[0], V0 + OLFX_VC_AMP_ENV_AMOUNT);
    EXPECT_EQ(f[1], R0 + OLFX_FR_MASTER_VOLUME);
    EXPECT_EQ(olfx_synth_control_map_at(K, 1, CC_VOLUME, OLFX_CTL_MIDI, 80.f, f, v), 1);
    /* refusals */
    EXPECT_EQ(olfx_synth_control_map_at(OLFX_KIND_SYNTH, 0, CC_DELAY_TIME, OLFX_CTL_MIDI, 64.f, f, v), OLFX_E_ARG);
    EXPECT_EQ(olfx_synth_control_map_at(K, 2, CC_DELAY_TIME, OLFX_CTL_MIDI, 64.f, f, v), OLFX_E_ARG);
    EXPECT_EQ(olfx_synth_control_map_at(K, 0, CC_DELAY_TIME, 7, 64.f, f, v), OLFX_E_ARG);
    EXPECT_EQ(olfx_synth_control_map_at(K, 0, CC_DELAY_TIME, OLFX_CTL_MIDI, 64.f, nullptr, v), OLFX_E_ARG);
    EXPECT_EQ(olfx_synth_control_map_at(OLFX_KIND_FXRACK, 0, CC_DELAY_TIME, OLFX_CTL_MIDI, 64.f, f, v), OLFX_E_KIND);
    EXPECT_EQ(olfx_control_map(K, CC_FILTER_CUTOFF, OLFX_CTL_MIDI, 64.f, &f1, &v1), OLFX_E_KIND);
    EXPECT_EQ(olfx_control_map(OLFX_KIND_SYNTH, CC_FILTER_CUTOFF, OLFX_CTL_MIDI, 64.f, &f1, &v1), OLFX_E_KIND);
}

TEST(SynthSvf, ControlThroughTheShadowFollowsTheInstanceTopology) {
    Shadow s = fresh(4);
    const float zero = 0.f;
    EXPECT_EQ(s.set_range(0, 1, R0 + OLFX_FR_TOPOLOGY, 1, &zero), OLFX_OK);
    EXPECT_EQ(s.set_range(2, 1, R0 + OLFX_FR_TOPOLOGY, 1, &zero), OLFX_OK);
    const olfx_control_event evs[] = {
        {0, CC_FILTER_CUTOFF, OLFX_CTL_MIDI, 0, 50.f},                  /* topology 0: the voice filter only */
        {1, CC_FILTER_CUTOFF, OLFX_CTL_MIDI, 0, 50.f},                  /* topology 1: both filters */
        {2, CC_FX_FILTER_CUTOFF, OLFX_CTL_MIDI, 0, 30.f},               /* topology 0: filter1 */
        {3, CC_FX_FILTER_CUTOFF, OLFX_CTL_MIDI, 0, 30.f},               /* topology 1: nothing */
        {2, CC_VOLUME, OLFX_CTL_MIDI, 0, 90.f},                         /* topology 0: voices and master */
        {3, CC_VOLUME, OLFX_CTL_MIDI, 0, 90.f},                         /* topology 1: voices only */
        {0, CC_FX_FILTER_TYPE, OLFX_CTL_HARDWARE, 0, 0.5f},
    };
    EXPECT_EQ(s.control(evs, 7), OLFX_OK);
    const float vcut = host::core_scale(50.f, 0.f, 127.f, 0.f, 20000.f, 2.5f);
    EXPECT_EQ(param(s, V0 + OLFX_VC_FILTER_CUTOFF, 0), vcut);
    EXPECT_EQ(param(s, R0 + OLFX_FR_FILTER_CUTOFF, 0), 20000.f);
    EXPECT_EQ(param(s, V0 + OLFX_VC_FILTER_CUTOFF, 1), vcut);
    EXPECT_EQ(param(s, R0 + OLFX_FR_FILTER_CUTOFF, 1), host::core_scale(50.f, 0.f, 127.f, 0.f, 20000.f, 1.f));
    EXPECT_EQ(param(s, R0 + OLFX_FR_FILTER_CUTOFF, 2), host::core_scale(30.f, 0.f, 127.f, 0.f, 20000.f, 1.f));
    EXPECT_EQ(param(s, R0 + OLFX_FR_FILTER_CUTOFF, 3), 20000.f);
    const float unit = host::core_scale(90.f, 0.f, 127.f, 0.f, 1.f, 1.f);
    EXPECT_EQ(param(s, V0 + OLFX_VC_AMP_ENV_AMOUNT, 2), unit);
    EXPECT_EQ(param(s, R0 + OLFX_FR_MASTER_VOLUME, 2), unit);
    EXPECT_EQ(param(s, V0 + OLFX_VC_AMP_ENV_AMOUNT, 3), unit);
    EXPECT_EQ(param(s, R0 + OLFX_FR_MASTER_VOLUME, 3), 0.8f);
    uint32_t f1;
    float v1;
    EXPECT_EQ(olfx_control_map(OLFX_KIND_FXRACK, CC_FX_FILTER_TYPE, OLFX_CTL_HARDWARE, 0.5f, &f1, &v1), OLFX_OK);
    EXPECT_EQ(param(s, R0 + OLFX_FR_FILTER_TYPE, 0), v1);
    /* a topology change moves the routing of the next event */
    const float one = 1.f;
    EXPECT_EQ(s.set_range(2, 1, R0 + OLFX_FR_TOPOLOGY, 1, &one), OLFX_OK);
    const olfx_control_event again = {2, CC_FX_FILTER_CUTOFF, OLFX_CTL_MIDI, 0, 99.f};
    EXPECT_EQ(s.control(&again, 1), OLFX_OK);
    EXPECT_EQ(param(s, R0 + OLFX_FR_FILTER_CUTOFF, 2), host::core_scale(30.f, 0.f, 127.f, 0.f, 20000.f, 1.f));
    const olfx_control_event bad = {4, CC_DELAY_TIME, OLFX_CTL_MIDI, 0, 1.f};
    EXPECT_EQ(s.control(&bad, 1), OLFX_E_ARG);
}

int main() { return run_all_tests(); }
