/*
 * tests/cpp/test_synth_host.cpp -- OLFX_KIND_SYNTH in the engine's HIP-free host core
 * (ol_dsp_amd/csrc/olfx_host.h) on the CPU: the kind tables, the 16 + 12 field split with its defaults
 * and validation, the coefficient record (voice record, then rack record), the Polyvoice router with
 * the reference's quirks, the control fan-out and the refused entry points.  Links olfx_host.cpp
 * directly (no libolfx.so, no GPU); built by tests/test_synth_host.py with its own build line.
 */
#include "../../ol_dsp_amd/csrc/olfx_host.h"
#include "harness.h"

using namespace olfx;
using host::Shadow;

namespace {

constexpr int K = OLFX_KIND_SYNTH;
constexpr uint32_t V0 = OLFX_SY_VOICE0, R0 = OLFX_SY_RACK0;
enum : uint8_t {
    CC_PORTAMENTO = 5, CC_VOLUME = 7, CC_REVERB_TIME = 32, CC_REVERB_BALANCE = 34, CC_DELAY_TIME = 35,
    CC_DELAY_CUTOFF = 37, CC_FILTER_CUTOFF = 41, CC_FILTER_RESONANCE = 42, CC_FX_FILTER_CUTOFF = 45,
    CC_ENV_FILT_D = 75, CC_OSC_1_VOLUME = 114,
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

/* the queued per-voice events as (voice slot, type, note) */
struct Q { uint32_t slot; uint8_t type, note; };
std::vector<Q> queued(const Shadow &s) {
    std::vector<Q> q;
    for (const olfx_voice_event &e : s.events) q.push_back({e.inst, e.type, e.note});
    return q;
}

int note(Shadow &s, uint32_t inst, uint8_t type, uint8_t n) {
    const olfx_event e{inst, type, n, 100, 0};
    return s.note_events(&e, 1);
}

float midi_unit(float v) { return host::core_scale(v, 0.f, 127.f, 0.f, 1.f, 1.f); }

}  // namespace

TEST(Synth, TablesAndDefaults) {
    EXPECT_EQ(OLFX_KIND_SYNTH, 11);
    EXPECT_EQ(OLFX_ABI_VERSION, 2);
    EXPECT_EQ(OLFX_SY_VOICE0, 0);
    EXPECT_EQ((uint32_t)OLFX_SY_RACK0, (uint32_t)OLFX_VC_NPARAMS);
    EXPECT_EQ((uint32_t)OLFX_SY_NPARAMS, 28u);
    EXPECT_EQ(host::n_params_of(K), 28u);
    EXPECT_EQ(host::in_channels(K), 0u);
    EXPECT_EQ(host::out_channels(K), 2u);
    EXPECT_TRUE(!is_voice_kind(K));
    EXPECT_TRUE(host::takes_note_events(K));
    EXPECT_EQ(host::n_params_of(9), 0u);                               /* still unassigned */

    float p[OLFX_SY_NPARAMS], vc[OLFX_VC_NPARAMS], fr[OLFX_FR_NPARAMS];
    host::default_params(K, p);
    host::default_params(OLFX_KIND_VOICE_MOOG, vc);
    host::default_params(OLFX_KIND_FXRACK, fr);
    EXPECT_TRUE(std::memcmp(p + V0, vc, sizeof vc) == 0);
    fr[OLFX_FR_TOPOLOGY] = 1.f;                                         /* the firmware's callback */
    EXPECT_TRUE(std::memcmp(p + R0, fr, sizeof fr) == 0);

    /* kind info: the rack's state, one set of voice coefficients, four Moog voices' state */
    const uint64_t rack = host::state_bytes(OLFX_KIND_FXRACK, 1, 48000.f);
    EXPECT_EQ(host::state_bytes(K, 1, 48000.f), rack + VCC_N * 4 + 4ull * VCS_N_MOOG * 4);
    EXPECT_EQ(host::state_bytes(K, 7, 48000.f), 7 * host::state_bytes(K, 1, 48000.f));
    const host::Segments sg = host::coef_segments(K);
    EXPECT_EQ(sg.nseg, 2u);
    EXPECT_EQ(sg.words[0], (uint32_t)VCC_N);
    EXPECT_EQ(sg.words[1], (uint32_t)FRC_N);
    /* the rack's figure for topology 1 with no input read */
    EXPECT_TRUE(std::fabs(host::algorithmic_bytes_per_frame(K) - (host::algorithmic_bytes_per_frame(OLFX_KIND_FXRACK) - 8.0)) < 1e-9);
    EXPECT_TRUE(std::fabs(host::algorithmic_read_bytes_per_frame(K) - 8.0) < 1e-9);

    /* voice slots: voices x n rounded up to 64 */
    Shadow s = fresh(65, 5);
    EXPECT_EQ(s.voices, 5u);
    EXPECT_EQ(s.npad, 128u);
    EXPECT_EQ(s.n_ev(), 640u);
    EXPECT_EQ(fresh(3, 4, OLFX_KIND_VOICE_MOOG).n_ev(), 3u);
    EXPECT_EQ(fresh(3, 4, OLFX_KIND_VOICE_MOOG).voices, 0u);
}

TEST(Synth, RecordIsVoiceThenRack) {
    const uint32_t n = 3;
    Shadow sy = fresh(n), vc = fresh(n, 4, OLFX_KIND_VOICE_MOOG), fr = fresh(n, 4, OLFX_KIND_FXRACK);
    /* defaults: the unconfigured voice (SynthVoice::Init without Update), the rack at topology 1 */
    const float one = 1.f;
    for (uint32_t i = 0; i < n; ++i) EXPECT_EQ(fr.set_range(i, 1, OLFX_FR_TOPOLOGY, 1, &one), OLFX_OK);
    {
        const std::vector<uint32_t> w = record(sy, 0), wv = record(vc, 0), wr = record(fr, 0);
        EXPECT_EQ(w.size(), wv.size() + wr.size());
        EXPECT_TRUE(std::equal(wv.begin(), wv.end(), w.begin()));
        EXPECT_TRUE(std::equal(wr.begin(), wr.end(), w.begin() + (long)wv.size()));
    }
    Lcg rng(7);
    for (uint32_t i = 0; i < n; ++i) {
        float v[OLFX_VC_NPARAMS], r[OLFX_FR_NPARAMS];
        for (float &x : v) x = rng.uni(0.01f, 0.9f);
        v[OLFX_VC_FILTER_CUTOFF] = rng.uni(100.f, 8000.f);
        for (float &x : r) x = rng.uni(0.f, 1.f);
        r[OLFX_FR_DELAY_CUTOFF] = rng.uni(100.f, 12000.f);
        r[OLFX_FR_FILTER_CUTOFF] = rng.uni(100.f, 12000.f);
        r[OLFX_FR_FILTER_TYPE] = (float)(i % 5);
        r[OLFX_FR_TOPOLOGY] = 1.f;
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
        EXPECT_EQ(master, 1.0f);                                        /* MASTER_VOLUME: stored, ignored */
    }
    /* a rack-only write is no Update() of the voices; a voice write is */
    Shadow a = fresh(2);
    const float t = 0.25f;
    EXPECT_EQ(a.set_range(0, 1, R0 + OLFX_FR_DELAY_TIME, 1, &t), OLFX_OK);
    EXPECT_EQ(a.configured[0], 0);
    EXPECT_EQ(a.set_range(1, 1, V0 + OLFX_VC_AMP_DECAY, 1, &t), OLFX_OK);
    EXPECT_EQ(a.configured[1], 1);
    const uint32_t inst = 0;
    EXPECT_EQ(a.set_list(R0 + OLFX_FR_DELAY_FEEDBACK, &inst, &t, 1), OLFX_OK);
    EXPECT_EQ(a.configured[0], 0);
    EXPECT_EQ(a.set_list(V0 + OLFX_VC_AMP_DECAY, &inst, &t, 1), OLFX_OK);
    EXPECT_EQ(a.configured[0], 1);
}

TEST(Synth, TopologyOtherThanOneIsRefusedAndChangesNothing) {
    Shadow s = fresh(3);
    const std::vector<float> before = s.params;
    for (float t : {0.f, 2.f, 3.f, 4.f, 5.f, -1.f, 0.5f}) {
        EXPECT_EQ(s.set_range(1, 1, R0 + OLFX_FR_TOPOLOGY, 1, &t), OLFX_E_ARG);
        const uint32_t inst = 2;
        EXPECT_EQ(s.set_list(R0 + OLFX_FR_TOPOLOGY, &inst, &t, 1), OLFX_E_ARG);
        EXPECT_EQ(s.set_member(0, R0 + OLFX_FR_TOPOLOGY, t), OLFX_E_ARG);
    }
    float row[OLFX_SY_NPARAMS];
    host::default_params(K, row);
    row[V0 + OLFX_VC_FILTER_CUTOFF] = 900.f;
    row[R0 + OLFX_FR_TOPOLOGY] = 0.f;
    EXPECT_EQ(s.set_range(0, 1, 0, OLFX_SY_NPARAMS, row), OLFX_E_ARG);   /* nothing of the row lands */
    const float nan = std::nanf("");
    EXPECT_EQ(s.set_range(0, 1, V0 + OLFX_VC_AMP_DECAY, 1, &nan), OLFX_E_ARG);
    EXPECT_EQ(s.set_range(0, 1, OLFX_SY_NPARAMS, 1, &row[0]), OLFX_E_ARG);   /* past the last field */
    EXPECT_TRUE(s.params == before);
    EXPECT_TRUE(s.dirty_list.empty());
    const float one = 1.f, vol = 0.3f;
    EXPECT_EQ(s.set_range(1, 1, R0 + OLFX_FR_TOPOLOGY, 1, &one), OLFX_OK);
    EXPECT_EQ(s.set_range(1, 1, R0 + OLFX_FR_MASTER_VOLUME, 1, &vol), OLFX_OK);   /* stored */
    EXPECT_EQ(param(s, R0 + OLFX_FR_MASTER_VOLUME, 1), 0.3f);
}

TEST(Synth, SetMemberAndUpdate) {
    Shadow s = fresh(2);
    /* a voice field before Update(): the member of all voices, no Update() */
    EXPECT_EQ(s.set_member(0, V0 + OLFX_VC_FILTER_RESONANCE, 0.4f), OLFX_OK);
    EXPECT_EQ(param(s, V0 + OLFX_VC_FILTER_RESONANCE, 0), 0.4f);
    EXPECT_EQ(s.configured[0], 0);
    /* a rack field: olfx_set_param */
    EXPECT_EQ(s.set_member(0, R0 + OLFX_FR_DELAY_TIME, 0.125f), OLFX_OK);
    EXPECT_EQ(param(s, R0 + OLFX_FR_DELAY_TIME, 0), 0.125f);
    EXPECT_EQ(s.configured[0], 0);
    EXPECT_EQ(s.update(0, 1), OLFX_OK);                                 /* Polyvoice::Update */
    EXPECT_EQ(s.configured[0], 1);
    EXPECT_EQ(s.configured[1], 0);
    /* after Update(): only the members Process reads, as the voice kind */
    EXPECT_EQ(s.set_member(0, V0 + OLFX_VC_FILTER_RESONANCE, 0.9f), OLFX_E_STATE);
    EXPECT_EQ(param(s, V0 + OLFX_VC_FILTER_RESONANCE, 0), 0.4f);
    EXPECT_EQ(s.set_member(0, V0 + OLFX_VC_FILTER_CUTOFF, 777.f), OLFX_OK);
    EXPECT_EQ(s.set_member(0, R0 + OLFX_FR_DELAY_TIME, 0.5f), OLFX_OK);
    /* the unconfigured record differs from the configured one (DaisySP's Init defaults) */
    EXPECT_TRUE(record(s, 0) != record(s, 1));
}

TEST(Synth, PolyvoiceRouter) {
    const uint32_t n = 70;                                              /* npad 128 */
    Shadow s = fresh(n);
    EXPECT_EQ(s.npad, 128u);
    const uint32_t i = 65;
    for (uint8_t k : {60, 64, 67, 70}) EXPECT_EQ(note(s, i, OLFX_EV_NOTE_ON, k), OLFX_OK);
    EXPECT_TRUE((playing(s, i) == std::vector<uint8_t>{60, 64, 67, 70}));
    EXPECT_TRUE((playing(s, 0) == std::vector<uint8_t>{0, 0, 0, 0}));
    std::vector<Q> q = queued(s);
    EXPECT_EQ(q.size(), (size_t)4);
    for (uint32_t p = 0; p < 4 && p < q.size(); ++p) {
        EXPECT_EQ(q[p].slot, p * 128u + i);                             /* voice slot p npad + inst */
        EXPECT_EQ(q[p].type, OLFX_EV_NOTE_ON);
    }
    /* a full instrument drops the fifth note */
    EXPECT_EQ(note(s, i, OLFX_EV_NOTE_ON, 72), OLFX_OK);
    EXPECT_EQ(s.events.size(), (size_t)4);
    EXPECT_TRUE((playing(s, i) == std::vector<uint8_t>{60, 64, 67, 70}));
    /* NoteOff frees the first match; the next NoteOn takes that voice */
    EXPECT_EQ(note(s, i, OLFX_EV_NOTE_OFF, 64), OLFX_OK);
    EXPECT_TRUE((playing(s, i) == std::vector<uint8_t>{60, 0, 67, 70}));
    EXPECT_EQ(s.events.back().inst, 1u * 128u + i);
    EXPECT_EQ(s.events.back().type, OLFX_EV_NOTE_OFF);
    EXPECT_EQ(note(s, i, OLFX_EV_NOTE_OFF, 99), OLFX_OK);               /* nobody plays 99: nothing */
    EXPECT_EQ(s.events.size(), (size_t)5);
    EXPECT_EQ(note(s, i, OLFX_EV_NOTE_ON, 72), OLFX_OK);
    EXPECT_TRUE((playing(s, i) == std::vector<uint8_t>{60, 72, 67, 70}));
    /* two voices on one note: NoteOff takes the first */
    Shadow d = fresh(2);
    EXPECT_EQ(note(d, 1, OLFX_EV_NOTE_ON, 50), OLFX_OK);
    EXPECT_EQ(note(d, 1, OLFX_EV_NOTE_ON, 50), OLFX_OK);
    EXPECT_EQ(note(d, 1, OLFX_EV_NOTE_OFF, 50), OLFX_OK);
    EXPECT_TRUE((playing(d, 1) == std::vector<uint8_t>{0, 50, 0, 0}));

    /* the note-0 quirks: NoteOn(0) gates a voice that stays free; NoteOff(0) hits the first free voice */
    Shadow z = fresh(1);
    EXPECT_EQ(note(z, 0, OLFX_EV_NOTE_ON, 61), OLFX_OK);
    EXPECT_EQ(note(z, 0, OLFX_EV_NOTE_ON, 0), OLFX_OK);
    EXPECT_EQ(z.events.back().inst, 1u * 64u + 0u);
    EXPECT_EQ(z.events.back().type, OLFX_EV_NOTE_ON);
    EXPECT_TRUE((playing(z, 0) == std::vector<uint8_t>{61, 0, 0, 0}));
    EXPECT_EQ(note(z, 0, OLFX_EV_NOTE_ON, 62), OLFX_OK);                /* takes voice 1 again */
    EXPECT_EQ(z.events.back().inst, 64u);
    EXPECT_TRUE((playing(z, 0) == std::vector<uint8_t>{61, 62, 0, 0}));
    EXPECT_EQ(note(z, 0, OLFX_EV_NOTE_OFF, 0), OLFX_OK);                /* voice 2: the first with Playing() == 0 */
    EXPECT_EQ(z.events.back().inst, 2u * 64u);
    EXPECT_EQ(z.events.back().type, OLFX_EV_NOTE_OFF);
    EXPECT_TRUE((playing(z, 0) == std::vector<uint8_t>{61, 62, 0, 0}));

    /* GATE_* fan out to every voice; SET_FREQUENCY is accepted and does nothing */
    Shadow g = fresh(3, 5);
    const olfx_voice_event ge[] = {{2, OLFX_EV_GATE_ON, 0, 0, 0, 0.f}, {2, OLFX_EV_SET_FREQUENCY, 0, 0, 0, 440.f},
                                   {1, OLFX_EV_GATE_OFF, 0, 0, 0, 0.f}};
    EXPECT_EQ(g.voice_events(ge, 3), OLFX_OK);
    q = queued(g);
    EXPECT_EQ(q.size(), (size_t)10);
    for (uint32_t p = 0; p < 5 && q.size() == 10; ++p) {
        EXPECT_EQ(q[p].slot, p * 64u + 2u);
        EXPECT_EQ(q[p].type, OLFX_EV_GATE_ON);
        EXPECT_EQ(q[5 + p].slot, p * 64u + 1u);
        EXPECT_EQ(q[5 + p].type, OLFX_EV_GATE_OFF);
    }
    EXPECT_TRUE((playing(g, 2) == std::vector<uint8_t>{0, 0, 0, 0, 0}));
    /* bad events are refused whole */
    const olfx_voice_event bad[] = {{0, OLFX_EV_NOTE_ON, 60, 0, 0, 0.f}, {3, OLFX_EV_NOTE_ON, 60, 0, 0, 0.f}};
    const size_t nq = g.events.size();
    EXPECT_EQ(g.voice_events(bad, 2), OLFX_E_ARG);
    EXPECT_EQ(g.events.size(), nq);
    EXPECT_TRUE((playing(g, 0) == std::vector<uint8_t>{0, 0, 0, 0, 0}));
    uint8_t buf[8];
    EXPECT_EQ(g.synth_playing(3, buf), OLFX_E_ARG);
    EXPECT_EQ(fresh(2, 4, OLFX_KIND_VOICE_MOOG).synth_playing(0, buf), OLFX_E_STATE);

    /* the routed events fold per voice slot into the slots' groups; reset clears Playing() */
    s.fold_events();
    EXPECT_EQ(s.ev_count.size(), (size_t)(4 * 128 / 64));
    EXPECT_EQ(s.ev_count[(0 * 128 + 65) >> 6], 1u);
    EXPECT_EQ(s.ev_count[(1 * 128 + 65) >> 6], 1u);
    const host::PacketPlan pl = s.plan(true);
    EXPECT_TRUE(pl.words <= host::max_packet_words(K, n, s.n_ev()));
    EXPECT_EQ(pl.words - pl.o_ev, (size_t)2 * (8 * kVevCap + s.n_more));
    s.reset();
    EXPECT_TRUE((playing(s, i) == std::vector<uint8_t>{0, 0, 0, 0}));
    EXPECT_TRUE(s.events.empty());
}

TEST(Synth, ControlMapFanOut) {
    uint32_t f[2] = {99, 99}, f1;
    float v[2] = {-1.f, -1.f}, v1;
    /* CC 41 hits the voice filter and FILTER_CUTOFF, each with its own handler's scaling */
    EXPECT_EQ(olfx_synth_control_map(CC_FILTER_CUTOFF, OLFX_CTL_MIDI, 64.f, f, v), 2);
    EXPECT_EQ(f[0], V0 + OLFX_VC_FILTER_CUTOFF);
    EXPECT_EQ(v[0], host::core_scale(64.f, 0.f, 127.f, 0.f, 20000.f, 2.5f));
    EXPECT_EQ(f[1], R0 + OLFX_FR_FILTER_CUTOFF);
    EXPECT_EQ(v[1], host::core_scale(64.f, 0.f, 127.f, 0.f, 20000.f, 1.f));
    /* MIDI scaling against hardware values */
    EXPECT_EQ(olfx_synth_control_map(CC_FILTER_CUTOFF, OLFX_CTL_HARDWARE, 0.5f, f, v), 2);
    EXPECT_EQ(v[0], host::core_scale(0.5f, 0.f, 1.f, 0.f, 20000.f, 2.5f));
    EXPECT_EQ(v[1], host::core_scale(0.5f, 0.f, 1.f, 0.f, 20000.f, 1.02f));
    EXPECT_EQ(olfx_synth_control_map(CC_FILTER_RESONANCE, OLFX_CTL_MIDI, 100.f, f, v), 2);
    EXPECT_EQ(f[0], V0 + OLFX_VC_FILTER_RESONANCE);
    EXPECT_EQ(f[1], R0 + OLFX_FR_FILTER_RESONANCE);
    EXPECT_EQ(v[0], midi_unit(100.f));
    EXPECT_EQ(v[1], midi_unit(100.f));
    EXPECT_EQ(olfx_synth_control_map(CC_FILTER_RESONANCE, OLFX_CTL_HARDWARE, 0.3f, f, v), 2);
    EXPECT_EQ(v[0], 0.3f);
    /* a delay CC hits one field, as the rack maps it */
    EXPECT_EQ(olfx_synth_control_map(CC_DELAY_TIME, OLFX_CTL_MIDI, 90.f, f, v), 1);
    EXPECT_EQ(olfx_control_map(OLFX_KIND_FXRACK, CC_DELAY_TIME, OLFX_CTL_MIDI, 90.f, &f1, &v1), OLFX_OK);
    EXPECT_EQ(f[0], R0 + f1);
    EXPECT_EQ(v[0], v1);
    EXPECT_EQ(olfx_synth_control_map(CC_DELAY_CUTOFF, OLFX_CTL_HARDWARE, 0.5f, f, v), 0);   /* MIDI only (Fx.h:253-260) */
    EXPECT_EQ(olfx_synth_control_map(CC_REVERB_BALANCE, OLFX_CTL_HARDWARE, 0.75f, f, v), 1);
    EXPECT_EQ(f[0], R0 + OLFX_FR_REVERB_BALANCE);
    /* voice-only controls: one field, as the voice maps it; CC 7 is the voices' volume, never the master */
    EXPECT_EQ(olfx_synth_control_map(CC_ENV_FILT_D, OLFX_CTL_MIDI, 100.f, f, v), 1);
    EXPECT_EQ(olfx_control_map(OLFX_KIND_VOICE_MOOG, CC_ENV_FILT_D, OLFX_CTL_MIDI, 100.f, &f1, &v1), OLFX_OK);
    EXPECT_EQ(f[0], V0 + f1);
    EXPECT_EQ(v[0], v1);
    EXPECT_EQ(olfx_synth_control_map(CC_VOLUME, OLFX_CTL_MIDI, 80.f, f, v), 1);
    EXPECT_EQ(f[0], V0 + OLFX_VC_AMP_ENV_AMOUNT);
    EXPECT_EQ(olfx_synth_control_map(CC_OSC_1_VOLUME, OLFX_CTL_MIDI, 100.f, f, v), 1);
    EXPECT_EQ(f[0], OLFX_FIELD_UPDATE_ONLY);
    /* unknown CCs, the rack's own filter CCs and the stub-only reverb CCs hit nothing */
    for (int cc : {3, 120, (int)CC_FX_FILTER_CUTOFF, (int)CC_REVERB_TIME})
        EXPECT_EQ(olfx_synth_control_map((uint8_t)cc, OLFX_CTL_MIDI, 64.f, f, v), 0);
    EXPECT_EQ(olfx_synth_control_map(CC_DELAY_TIME, 7, 64.f, f, v), OLFX_E_ARG);
    EXPECT_EQ(olfx_synth_control_map(CC_DELAY_TIME, OLFX_CTL_MIDI, 64.f, nullptr, v), OLFX_E_ARG);
    /* the one-field map has nothing to say about this kind */
    EXPECT_EQ(olfx_control_map(K, CC_FILTER_CUTOFF, OLFX_CTL_MIDI, 64.f, &f1, &v1), OLFX_E_KIND);
    EXPECT_EQ(olfx_control_map(9, CC_FILTER_CUTOFF, OLFX_CTL_MIDI, 64.f, &f1, &v1), OLFX_E_KIND);
    EXPECT_EQ(olfx_control_map(OLFX_KIND_FXRACK, 3, OLFX_CTL_MIDI, 64.f, &f1, &v1), OLFX_IGNORED);
}

TEST(Synth, ControlThroughTheShadow) {
    Shadow s = fresh(3);
    const olfx_control_event evs[] = {
        {0, CC_FILTER_CUTOFF, OLFX_CTL_MIDI, 0, 50.f},
        {1, CC_DELAY_TIME, OLFX_CTL_HARDWARE, 0, 0.25f},
        {2, CC_OSC_1_VOLUME, OLFX_CTL_MIDI, 0, 100.f},
        {2, CC_FX_FILTER_CUTOFF, OLFX_CTL_MIDI, 0, 1.f},
    };
    EXPECT_EQ(s.control(evs, 4), OLFX_OK);
    EXPECT_EQ(param(s, V0 + OLFX_VC_FILTER_CUTOFF, 0), host::core_scale(50.f, 0.f, 127.f, 0.f, 20000.f, 2.5f));
    EXPECT_EQ(param(s, R0 + OLFX_FR_FILTER_CUTOFF, 0), host::core_scale(50.f, 0.f, 127.f, 0.f, 20000.f, 1.f));
    EXPECT_EQ(s.configured[0], 1);                                      /* the voices' handler Update()s */
    EXPECT_EQ(param(s, R0 + OLFX_FR_DELAY_TIME, 1), 0.25f);
    EXPECT_EQ(s.configured[1], 0);                                      /* delay_fx only */
    EXPECT_EQ(s.configured[2], 1);                                      /* update-only: Update() with unchanged members */
    EXPECT_EQ(param(s, R0 + OLFX_FR_FILTER_CUTOFF, 2), 20000.f);        /* CC 45 reaches nothing */
    EXPECT_EQ(s.dirty_list.size(), (size_t)3);
    const olfx_control_event bad = {3, CC_DELAY_TIME, OLFX_CTL_MIDI, 0, 1.f};
    EXPECT_EQ(s.control(&bad, 1), OLFX_E_ARG);
}

TEST(Synth, RefusedEntryPoints) {
    Shadow s = fresh(2);
    host::BankPlan plan;
    const uint64_t off[2] = {0, 4};
    const float pcm[4] = {0, 0, 0, 0};
    EXPECT_EQ(s.bank_plan(1, off, pcm, &plan), OLFX_E_STATE);
    const olfx_sample_voice rec{0, OLFX_NO_SAMPLE, 0, 0, 0, 0};
    EXPECT_EQ(s.sample_voices(&rec, 1), OLFX_E_STATE);
    /* ... while the kinds without voices still refuse note events */
    Shadow r = fresh(2, 4, OLFX_KIND_FXRACK);
    EXPECT_EQ(note(r, 0, OLFX_EV_NOTE_ON, 60), OLFX_E_STATE);
}

int main() { return run_all_tests(); }
