/*
 * tests/cpp/test_drumkit_host.cpp -- OLFX_KIND_DRUMKIT in the engine's HIP-free host core
 * (ol_dsp_amd/csrc/olfx_host.h) on the CPU: the field layout and defaults, validation per slot, the per-slot
 * Update() bookkeeping, the VoiceMap (displacement, clearing, the "leave alone" values, a swap in one call, a
 * voice at two notes refused with nothing changed, range errors), note routing and the playing table, refused
 * gate and frequency events, control routing by channel, the sum-order word, reset keeping map, bank and
 * assignments, and the packet's size at the worst case.  Links olfx_host.cpp directly (no libolfx.so, no GPU);
 * built by tests/test_drumkit_host.py with its own build line.
 */
#include "../../ol_dsp_amd/csrc/olfx_host.h"
#include "harness.h"

using namespace olfx;
using host::Shadow;

namespace {

constexpr int K = OLFX_KIND_DRUMKIT;
constexpr uint32_t R0 = OLFX_DK_RACK0, NONE = OLFX_DK_NO_VOICE;
constexpr uint8_t NO_NOTE = OLFX_DK_NO_NOTE, NO_CH = OLFX_DK_NO_CHANNEL;
enum : uint8_t { CC_VOLUME = 7, CC_FILTER_CUTOFF = 41, CC_FX_FILTER_CUTOFF = 45, CC_OSC_1_VOLUME = 114, CC_NOBODY = 3 };

void drain(Shadow &s) {
    const host::PacketPlan pl = s.plan(false);
    std::vector<uint32_t> buf(pl.words + 4);
    s.fill_records(pl, buf.data());
}

Shadow fresh(uint32_t n, uint32_t voices = 4) {
    Shadow s;
    s.init(K, n, 48000.f, voices);
    s.reset();
    drain(s);
    return s;
}

uint32_t slot_field(uint32_t p, uint32_t f) { return OLFX_DK_VOICE0 + 16 * p + f; }
float param(const Shadow &s, uint32_t field, uint32_t inst) { return s.params[(size_t)field * s.n + inst]; }
std::vector<uint32_t> sorted(std::vector<uint32_t> v) { std::sort(v.begin(), v.end()); return v; }

int map1(Shadow &s, uint32_t kit, uint32_t voice, uint8_t channel, uint8_t note) {
    const olfx_drumkit_voice r{kit, voice, channel, note, 0};
    return s.drumkit_map(&r, 1);
}
int note(Shadow &s, uint32_t kit, uint8_t type, uint8_t n) {
    const olfx_event e{kit, type, n, 100, 0};
    return s.note_events(&e, 1);
}
int control(Shadow &s, uint32_t kit, uint8_t cc, float value, uint16_t channel, uint8_t source = OLFX_CTL_MIDI) {
    const olfx_control_event e{kit, cc, source, channel, value};
    return s.control(&e, 1);
}
std::vector<uint8_t> playing(Shadow &s, uint32_t kit) {
    std::vector<uint8_t> p(s.voices, 0xEE);
    EXPECT_EQ(s.synth_playing(kit, p.data()), OLFX_OK);
    return p;
}

}  // namespace

TEST(DrumKit, LayoutAndDefaults) {
    EXPECT_EQ(OLFX_KIND_DRUMKIT, 14);
    EXPECT_EQ(OLFX_ABI_VERSION, 2);
    EXPECT_EQ(OLFX_DK_NPARAMS, 140);
    EXPECT_EQ(OLFX_DK_RACK0, 128);
    EXPECT_EQ(host::n_params_of(K), 140u);
    EXPECT_EQ(host::n_params_of(13), 0u);
    EXPECT_EQ(host::in_channels(K), 0u);
    EXPECT_EQ(host::out_channels(K), 2u);
    EXPECT_TRUE(host::takes_note_events(K) && !is_voice_kind(K) && !is_synth_kind(K));
    EXPECT_EQ(std::string(host::kind_desc(K).kernel), std::string("drumkit_block_v1"));

    float p[OLFX_DK_NPARAMS], vc[OLFX_VC_NPARAMS], fr[OLFX_FR_NPARAMS];
    host::default_params(K, p);
    host::default_params(OLFX_KIND_VOICE_SAMPLE, vc);
    host::default_params(OLFX_KIND_FXRACK, fr);
    for (uint32_t q = 0; q < 8; ++q) EXPECT_TRUE(std::memcmp(p + 16 * q, vc, sizeof vc) == 0);
    fr[OLFX_FR_TOPOLOGY] = 1.f;
    EXPECT_TRUE(std::memcmp(p + R0, fr, sizeof fr) == 0);

    /* the 4-voice figure: the rack, and four voices' state, coefficients and Sample words */
    const uint64_t rack = host::state_bytes(OLFX_KIND_FXRACK, 1, 48000.f);
    EXPECT_EQ(host::state_bytes(K, 1, 48000.f), rack + 4ull * (VCS_N + VCC_N + SMC_N) * 4);
    EXPECT_EQ(host::state_bytes(K, 1, 48000.f), rack + 4 * host::state_bytes(OLFX_KIND_VOICE_SAMPLE, 1, 48000.f));
    const host::Segments kit = host::coef_segments(K), slot = host::voice_segments(K);
    EXPECT_EQ(kit.nseg, 2u);
    EXPECT_EQ(kit.words[0], (uint32_t)FRC_N);
    EXPECT_EQ(kit.words[1], (uint32_t)DKC_N);
    EXPECT_EQ(slot.nseg, 2u);
    EXPECT_EQ(slot.words[0], (uint32_t)VCC_N);
    EXPECT_EQ(slot.words[1], (uint32_t)SMC_N);
    EXPECT_EQ(host::voice_segments(OLFX_KIND_SYNTH_SVF).nseg, 0u);

    Shadow s = fresh(65, 5);
    EXPECT_EQ(s.voices, 5u);
    EXPECT_EQ(s.npad, 128u);
    EXPECT_EQ(s.n_ev(), 640u);
    EXPECT_EQ(s.n_voices(), 325u);
    EXPECT_EQ(s.samples.size(), (size_t)325);
    EXPECT_EQ(s.configured.size(), (size_t)325);
    /* the slot record of a fresh engine is the sample voice's, unconfigured and unassigned */
    Shadow v;
    v.init(OLFX_KIND_VOICE_SAMPLE, 1, 48000.f);
    v.reset();
    std::vector<uint32_t> a(VCC_N + SMC_N), b(VCC_N + SMC_N);
    s.derive_voice_record(3 * 65 + 7, a.data());
    v.derive_record(0, b.data());
    EXPECT_TRUE(a == b);
    /* the kit record: the rack's at topology 1, then the empty map's order word */
    std::vector<uint32_t> w(FRC_N + DKC_N);
    s.derive_record(0, w.data());
    EXPECT_EQ(w[FRC_TOPO], 1u);
    EXPECT_EQ(w[FRC_N + DKC_ORDER], kDkOrderEmpty);
    uint32_t f = 0;
    float val = 0.f;
    EXPECT_EQ(olfx_control_map(K, CC_FILTER_CUTOFF, OLFX_CTL_MIDI, 64.f, &f, &val), OLFX_E_KIND);
    uint32_t f2[2];
    float v2[2];
    EXPECT_EQ(olfx_synth_control_map_at(K, 1, CC_FILTER_CUTOFF, OLFX_CTL_MIDI, 64.f, f2, v2), OLFX_E_KIND);
}

TEST(DrumKit, ValidationPerSlot) {
    Shadow s = fresh(3, 2);
    const float nan = std::nanf(""), two = 2.f, zero = 0.f, half = 0.5f;
    for (uint32_t q = 0; q < 8; ++q) {                      /* slots past the kit's voices are validated too */
        EXPECT_EQ(s.set_range(1, 1, slot_field(q, OLFX_VC_FILTER_CUTOFF), 1, &nan), OLFX_E_ARG);
        EXPECT_EQ(s.set_range(1, 1, slot_field(q, OLFX_VC_FILTER_CUTOFF), 1, &half), OLFX_OK);
        EXPECT_EQ(param(s, slot_field(q, OLFX_VC_FILTER_CUTOFF), 1), 0.5f);
    }
    EXPECT_EQ(s.set_range(1, 1, R0 + OLFX_FR_TOPOLOGY, 1, &two), OLFX_E_ARG);
    EXPECT_TRUE(std::strstr(s.msg, "drum kit rack topology must be 0 or 1") != nullptr);
    EXPECT_EQ(param(s, R0 + OLFX_FR_TOPOLOGY, 1), 1.f);
    EXPECT_EQ(s.set_range(1, 1, R0 + OLFX_FR_TOPOLOGY, 1, &zero), OLFX_OK);
    EXPECT_EQ(s.set_range(0, 3, OLFX_DK_NPARAMS, 1, &zero), OLFX_E_ARG);
    /* a [140][n] draw is one call, whatever P */
    std::vector<float> all(140 * 3);
    float d[140];
    host::default_params(K, d);
    for (uint32_t fld = 0; fld < 140; ++fld) for (uint32_t i = 0; i < 3; ++i) all[fld * 3 + i] = d[fld];
    EXPECT_EQ(s.set_range(0, 3, 0, 140, all.data()), OLFX_OK);
    all[139 * 3 + 2] = 3.f;                                  /* one bad value: nothing changes */
    all[0] = 99.f;
    EXPECT_EQ(s.set_range(0, 3, 0, 140, all.data()), OLFX_E_ARG);
    EXPECT_EQ(param(s, 0, 0), d[0]);
}

TEST(DrumKit, UpdateBookkeepingIsPerSlot) {
    const uint32_t n = 4;
    Shadow s = fresh(n, 3);
    EXPECT_TRUE(s.dirty_list.empty() && s.vdirty_list.empty());
    for (uint8_t c : s.configured) EXPECT_EQ(c, 0);
    const float v = 0.25f;
    /* one field of slot 1 of kit 2: that voice alone is Update()d, the rack is not re-derived */
    EXPECT_EQ(s.set_range(2, 1, slot_field(1, OLFX_VC_AMP_DECAY), 1, &v), OLFX_OK);
    EXPECT_TRUE(s.vdirty_list == std::vector<uint32_t>{1 * n + 2});
    EXPECT_TRUE(s.dirty_list.empty());
    EXPECT_EQ(s.configured[1 * n + 2], 1);
    EXPECT_EQ(s.configured[0 * n + 2] + s.configured[2 * n + 2] + s.configured[1 * n + 1], 0);
    drain(s);
    /* a rack field: the kit's record only */
    EXPECT_EQ(s.set_range(1, 1, R0 + OLFX_FR_DELAY_TIME, 1, &v), OLFX_OK);
    EXPECT_TRUE(s.vdirty_list.empty());
    EXPECT_TRUE(s.dirty_list == std::vector<uint32_t>{1});
    drain(s);
    /* a range from slot 0's last field to slot 2's first: slots 0, 1 and 2 of kits 0 and 1 */
    std::vector<float> vals(18 * 2, 0.5f);
    EXPECT_EQ(s.set_range(0, 2, slot_field(0, 15), 18, vals.data()), OLFX_OK);
    EXPECT_TRUE(sorted(s.vdirty_list) == (std::vector<uint32_t>{0, 1, n, n + 1, 2 * n, 2 * n + 1}));
    EXPECT_TRUE(s.dirty_list.empty());
    drain(s);
    /* a slot past the kit's voices: stored, nothing to derive */
    EXPECT_EQ(s.set_range(0, 1, slot_field(5, 0), 1, &v), OLFX_OK);
    EXPECT_TRUE(s.vdirty_list.empty() && s.dirty_list.empty());
    EXPECT_EQ(param(s, slot_field(5, 0), 0), 0.25f);
    /* a range over the last slot in use and the rack */
    std::vector<float> tail(140 - 47);
    float d[140];
    host::default_params(K, d);
    for (uint32_t fld = 47; fld < 140; ++fld) tail[fld - 47] = d[fld];
    EXPECT_EQ(s.set_range(3, 1, 47, 140 - 47, tail.data()), OLFX_OK);
    EXPECT_TRUE(s.vdirty_list == std::vector<uint32_t>{2 * n + 3});
    EXPECT_TRUE(s.dirty_list == std::vector<uint32_t>{3});
    drain(s);
    /* set_list */
    const uint32_t insts[2] = {3, 0};
    const float lv[2] = {0.1f, 0.2f};
    EXPECT_EQ(s.set_list(slot_field(2, OLFX_VC_FILTER_CUTOFF), insts, lv, 2), OLFX_OK);
    EXPECT_TRUE(s.vdirty_list == (std::vector<uint32_t>{2 * n + 3, 2 * n + 0}));
    EXPECT_EQ(s.configured[2 * n + 0], 1);
    drain(s);
    /* set_member stores without Update(); refused once that slot is Update()d, except what Process reads */
    EXPECT_EQ(s.configured[0 * n + 3], 0);
    EXPECT_EQ(s.set_member(3, slot_field(0, OLFX_VC_AMP_ATTACK), 0.3f), OLFX_OK);
    EXPECT_EQ(s.configured[0 * n + 3], 0);
    EXPECT_TRUE(s.vdirty_list == std::vector<uint32_t>{0 * n + 3});
    EXPECT_EQ(s.set_member(3, slot_field(2, OLFX_VC_AMP_ATTACK), 0.3f), OLFX_E_STATE);
    EXPECT_EQ(s.set_member(3, slot_field(2, OLFX_VC_FILTER_CUTOFF), 0.3f), OLFX_OK);
    EXPECT_EQ(s.set_member(3, slot_field(7, OLFX_VC_AMP_ATTACK), 0.3f), OLFX_OK);
    EXPECT_EQ(s.set_member(3, R0 + OLFX_FR_DELAY_TIME, 0.3f), OLFX_OK);          /* a rack field: olfx_set_param */
    drain(s);
    /* olfx_update: every voice of those kits, and their racks */
    EXPECT_EQ(s.update(1, 2), OLFX_OK);
    EXPECT_TRUE(sorted(s.vdirty_list) == (std::vector<uint32_t>{1, 2, n + 1, n + 2, 2 * n + 1, 2 * n + 2}));
    EXPECT_TRUE(s.dirty_list == (std::vector<uint32_t>{1, 2}));
    for (uint32_t q = 0; q < 3; ++q) EXPECT_EQ(s.configured[q * n + 1], 1);
    /* the record of a configured slot is the sample voice's for the same fields */
    Shadow vs;
    vs.init(OLFX_KIND_VOICE_SAMPLE, 1, 48000.f);
    vs.reset();
    float vf[16];
    for (uint32_t fld = 0; fld < 16; ++fld) vf[fld] = param(s, slot_field(2, fld), 3);
    EXPECT_EQ(vs.set_range(0, 1, 0, 16, vf), OLFX_OK);
    std::vector<uint32_t> a(VCC_N + SMC_N), b(VCC_N + SMC_N);
    s.derive_voice_record(2 * n + 3, a.data());
    vs.derive_record(0, b.data());
    EXPECT_TRUE(a == b);
}

TEST(DrumKit, Map) {
    const uint32_t n = 3;
    Shadow s = fresh(n, 4);
    EXPECT_EQ(s.order_word(1), kDkOrderEmpty);
    /* SetVoice(channel, note, voice) */
    EXPECT_EQ(map1(s, 1, 2, 5, 60), OLFX_OK);
    EXPECT_EQ(s.note2voice[60 * n + 1], 2);
    EXPECT_EQ(s.chan2voice[5 * n + 1], 2);
    EXPECT_EQ(s.note2voice[60 * n + 0], Shadow::kNoVoice);
    EXPECT_TRUE(s.dirty_list == std::vector<uint32_t>{1});
    EXPECT_EQ(s.order_word(1), 0xFFFFFFF2u);
    drain(s);
    EXPECT_EQ(map1(s, 1, 0, 6, 72), OLFX_OK);
    EXPECT_EQ(map1(s, 1, 3, 7, 36), OLFX_OK);
    EXPECT_EQ(s.order_word(1), 0xFFFFF023u);                 /* notes 36, 60, 72: voices 3, 2, 0 */
    /* displacement: voice 1 takes note 60 and channel 5; voice 2 sits nowhere */
    EXPECT_EQ(map1(s, 1, 1, 5, 60), OLFX_OK);
    EXPECT_EQ(s.order_word(1), 0xFFFFF013u);
    EXPECT_EQ(s.chan2voice[5 * n + 1], 1);
    /* the "leave alone" values */
    EXPECT_EQ(map1(s, 1, 2, NO_CH, 61), OLFX_OK);
    EXPECT_EQ(s.chan2voice[5 * n + 1], 1);
    EXPECT_EQ(s.order_word(1), 0xFFFF0213u);
    EXPECT_EQ(map1(s, 1, 2, 9, NO_NOTE), OLFX_OK);
    EXPECT_EQ(s.chan2voice[9 * n + 1], 2);
    EXPECT_EQ(s.order_word(1), 0xFFFF0213u);
    /* clearing */
    EXPECT_EQ(map1(s, 1, NONE, 9, 61), OLFX_OK);
    EXPECT_EQ(s.chan2voice[9 * n + 1], Shadow::kNoVoice);
    EXPECT_EQ(s.order_word(1), 0xFFFFF013u);
    /* a voice at two notes: refused, nothing changed (the channel write of the same record neither) */
    const std::vector<uint8_t> n2v = s.note2voice, c2v = s.chan2voice;
    drain(s);
    EXPECT_EQ(map1(s, 1, 1, 11, 90), OLFX_E_ARG);
    EXPECT_TRUE(std::strstr(s.msg, "two notes") != nullptr);
    const olfx_drumkit_voice bad[3] = {{0, 0, 0, 10, 0}, {2, 1, 1, 20, 0}, {2, 1, 2, 21, 0}};
    EXPECT_EQ(s.drumkit_map(bad, 3), OLFX_E_ARG);
    EXPECT_TRUE(s.note2voice == n2v && s.chan2voice == c2v && s.dirty_list.empty());
    /* a swap of two voices' notes in one call: voice 1 sits at two notes after the first record only */
    const olfx_drumkit_voice swap[2] = {{1, 1, NO_CH, 72, 0}, {1, 0, NO_CH, 60, 0}};
    EXPECT_EQ(s.drumkit_map(swap, 2), OLFX_OK);
    EXPECT_EQ(s.order_word(1), 0xFFFFF103u);
    /* the same voice on several channels is fine */
    EXPECT_EQ(map1(s, 1, 3, 0, NO_NOTE), OLFX_OK);
    EXPECT_EQ(map1(s, 1, 3, 1, NO_NOTE), OLFX_OK);
    /* range errors */
    EXPECT_EQ(map1(s, 3, 0, 0, 0), OLFX_E_ARG);
    EXPECT_EQ(map1(s, 0, 4, 0, 0), OLFX_E_ARG);
    EXPECT_EQ(map1(s, 0, 0, 0, 128), OLFX_E_ARG);
    EXPECT_EQ(map1(s, 0, 0, 0, 254), OLFX_E_ARG);
    EXPECT_EQ(map1(s, 0, 0, 16, 0), OLFX_E_ARG);
    EXPECT_EQ(map1(s, 0, 0, 254, 0), OLFX_E_ARG);
    EXPECT_EQ(s.drumkit_map(nullptr, 1), OLFX_E_ARG);
    EXPECT_EQ(s.drumkit_map(nullptr, 0), OLFX_OK);
    /* eight voices at eight notes fill the word */
    Shadow e8 = fresh(1, 8);
    for (uint32_t q = 0; q < 8; ++q) EXPECT_EQ(map1(e8, 0, 7 - q, NO_CH, (uint8_t)(10 + q)), OLFX_OK);
    EXPECT_EQ(e8.order_word(0), 0x01234567u);
    /* another kind */
    Shadow sy;
    sy.init(OLFX_KIND_SYNTH_SVF, 2, 48000.f);
    sy.reset();
    EXPECT_EQ(map1(sy, 0, 0, 0, 0), OLFX_E_STATE);
}

TEST(DrumKit, NoteRoutingAndPlaying) {
    const uint32_t n = 70;
    Shadow s = fresh(n, 3);
    EXPECT_EQ(s.npad, 128u);
    EXPECT_EQ(map1(s, 69, 2, 0, 40), OLFX_OK);
    EXPECT_EQ(map1(s, 69, 0, 1, 50), OLFX_OK);
    EXPECT_EQ(note(s, 69, OLFX_EV_NOTE_ON, 40), OLFX_OK);
    EXPECT_EQ(s.events.size(), (size_t)1);
    EXPECT_EQ(s.events[0].inst, 2 * 128u + 69u);             /* voice slot p * npad + kit */
    EXPECT_EQ(s.events[0].type, OLFX_EV_NOTE_ON);
    EXPECT_TRUE(playing(s, 69) == (std::vector<uint8_t>{0, 0, 40}));
    EXPECT_EQ(note(s, 69, OLFX_EV_NOTE_ON, 41), OLFX_OK);    /* nobody sits there: ignored */
    EXPECT_EQ(note(s, 68, OLFX_EV_NOTE_ON, 40), OLFX_OK);    /* another kit's map */
    EXPECT_EQ(s.events.size(), (size_t)1);
    EXPECT_EQ(note(s, 69, OLFX_EV_NOTE_ON, 50), OLFX_OK);
    EXPECT_TRUE(playing(s, 69) == (std::vector<uint8_t>{50, 0, 40}));
    EXPECT_EQ(note(s, 69, OLFX_EV_NOTE_OFF, 40), OLFX_OK);
    EXPECT_TRUE(playing(s, 69) == (std::vector<uint8_t>{50, 0, 0}));
    EXPECT_EQ(s.events.size(), (size_t)3);
    /* the map takes effect in call order: the queued events keep their voices */
    EXPECT_EQ(map1(s, 69, 1, NO_CH, 50), OLFX_OK);
    EXPECT_EQ(s.events[1].inst, 0 * 128u + 69u);
    EXPECT_EQ(note(s, 69, OLFX_EV_NOTE_OFF, 50), OLFX_OK);
    EXPECT_EQ(s.events[3].inst, 1 * 128u + 69u);
    /* the folded records carry the sample voice's seek */
    s.fold_events();
    EXPECT_EQ(s.folded.size(), (size_t)3);
    EXPECT_TRUE((s.folded[0].op & VEV_SEEK) != 0);
    /* gate and frequency events: VoiceMap has no such call; a refused call queues nothing */
    EXPECT_EQ(note(s, 69, OLFX_EV_GATE_ON, 40), OLFX_E_ARG);
    EXPECT_EQ(note(s, 69, OLFX_EV_GATE_OFF, 40), OLFX_E_ARG);
    const olfx_voice_event ve[2] = {{69, OLFX_EV_NOTE_ON, 40, 100, 0, 0.f}, {69, OLFX_EV_SET_FREQUENCY, 0, 0, 0, 440.f}};
    EXPECT_EQ(s.voice_events(ve, 2), OLFX_E_ARG);
    EXPECT_TRUE(s.events.empty());
    EXPECT_EQ(s.voice_events(ve, 1), OLFX_OK);
    EXPECT_EQ(s.events.size(), (size_t)1);
    EXPECT_EQ(note(s, 70, OLFX_EV_NOTE_ON, 40), OLFX_E_ARG);
    EXPECT_EQ(note(s, 0, OLFX_EV_NOTE_ON, 128), OLFX_E_ARG);
    uint8_t out[3];
    EXPECT_EQ(s.synth_playing(70, out), OLFX_E_ARG);
}

TEST(DrumKit, ControlRoutingByChannel) {
    const uint32_t n = 3;
    Shadow s = fresh(n, 4);
    EXPECT_EQ(map1(s, 1, 2, 5, 60), OLFX_OK);
    drain(s);
    const std::vector<float> before = s.params;
    uint32_t f = 0;
    float v = 0.f;
    /* channel 5 of kit 1 is voice 2: the voice kind's mapping lands on slot 2's field, that voice alone */
    EXPECT_EQ(olfx_control_map(OLFX_KIND_VOICE_SAMPLE, CC_FILTER_CUTOFF, OLFX_CTL_MIDI, 90.f, &f, &v), OLFX_OK);
    EXPECT_EQ(control(s, 1, CC_FILTER_CUTOFF, 90.f, 5), OLFX_OK);
    EXPECT_EQ(param(s, slot_field(2, f), 1), v);
    EXPECT_TRUE(s.vdirty_list == std::vector<uint32_t>{2 * n + 1});
    EXPECT_TRUE(s.dirty_list.empty());
    EXPECT_EQ(s.configured[2 * n + 1], 1);
    size_t changed = 0;
    for (size_t k = 0; k < before.size(); ++k) changed += std::memcmp(&before[k], &s.params[k], 4) != 0;
    EXPECT_EQ(changed, (size_t)1);
    drain(s);
    /* hardware source; an Update()-only control */
    EXPECT_EQ(olfx_control_map(OLFX_KIND_VOICE_SAMPLE, CC_VOLUME, OLFX_CTL_HARDWARE, 0.6f, &f, &v), OLFX_OK);
    EXPECT_EQ(control(s, 1, CC_VOLUME, 0.6f, 5, OLFX_CTL_HARDWARE), OLFX_OK);
    EXPECT_EQ(param(s, slot_field(2, f), 1), v);
    drain(s);
    EXPECT_EQ(map1(s, 1, 3, 6, NO_NOTE), OLFX_OK);
    drain(s);
    EXPECT_EQ(control(s, 1, CC_OSC_1_VOLUME, 64.f, 6), OLFX_OK);
    EXPECT_EQ(s.configured[3 * n + 1], 1);
    EXPECT_TRUE(s.vdirty_list == std::vector<uint32_t>{3 * n + 1});
    drain(s);
    /* an empty channel, another kit's channel, channels that are none, a control the voice ignores */
    const std::vector<float> mid = s.params;
    EXPECT_EQ(control(s, 1, CC_FILTER_CUTOFF, 90.f, 4), OLFX_OK);
    EXPECT_EQ(control(s, 0, CC_FILTER_CUTOFF, 90.f, 5), OLFX_OK);
    EXPECT_EQ(control(s, 1, CC_FILTER_CUTOFF, 90.f, 17), OLFX_OK);
    EXPECT_EQ(control(s, 1, CC_FILTER_CUTOFF, 90.f, 0xFFFF), OLFX_OK);
    EXPECT_EQ(control(s, 1, CC_NOBODY, 90.f, 5), OLFX_OK);
    EXPECT_TRUE(s.params == mid && s.vdirty_list.empty() && s.dirty_list.empty());
    /* the rack channel: the rack's mapping at the kit's topology */
    EXPECT_EQ(olfx_control_map(OLFX_KIND_FXRACK, CC_FX_FILTER_CUTOFF, OLFX_CTL_MIDI, 70.f, &f, &v), OLFX_OK);
    EXPECT_EQ(control(s, 1, CC_FILTER_CUTOFF, 70.f, OLFX_DK_CHANNEL_RACK), OLFX_OK);      /* topology 1: 41 -> FILTER_* */
    EXPECT_EQ(param(s, R0 + f, 1), v);
    EXPECT_TRUE(s.dirty_list == std::vector<uint32_t>{1});
    EXPECT_TRUE(s.vdirty_list.empty());
    drain(s);
    EXPECT_EQ(control(s, 1, CC_FX_FILTER_CUTOFF, 20.f, OLFX_DK_CHANNEL_RACK), OLFX_OK);   /* topology 1: 45 reaches nothing */
    EXPECT_EQ(param(s, R0 + f, 1), v);
    const float zero = 0.f;
    EXPECT_EQ(s.set_range(1, 1, R0 + OLFX_FR_TOPOLOGY, 1, &zero), OLFX_OK);
    EXPECT_EQ(control(s, 1, CC_FILTER_CUTOFF, 20.f, OLFX_DK_CHANNEL_RACK), OLFX_OK);      /* topology 0: 41 reaches nothing */
    EXPECT_EQ(param(s, R0 + f, 1), v);
    float v20 = 0.f;
    EXPECT_EQ(olfx_control_map(OLFX_KIND_FXRACK, CC_FX_FILTER_CUTOFF, OLFX_CTL_MIDI, 20.f, &f, &v20), OLFX_OK);
    EXPECT_EQ(control(s, 1, CC_FX_FILTER_CUTOFF, 20.f, OLFX_DK_CHANNEL_RACK), OLFX_OK);
    EXPECT_EQ(param(s, R0 + f, 1), v20);
    EXPECT_EQ(control(s, 3, CC_FILTER_CUTOFF, 20.f, 5), OLFX_E_ARG);
    EXPECT_EQ(control(s, 1, CC_FILTER_CUTOFF, 20.f, 5, 7), OLFX_E_ARG);
}

TEST(DrumKit, ResetKeepsMapBankAndAssignments) {
    const uint32_t n = 2, P = 3;
    Shadow s = fresh(n, P);
    const uint64_t offs[3] = {0, 100, 130};
    std::vector<float> pcm(130, 0.25f);
    host::BankPlan plan;
    EXPECT_EQ(s.bank_plan(2, offs, pcm.data(), &plan), OLFX_OK);
    s.bank_commit(std::move(plan));
    EXPECT_EQ(s.vdirty_list.size(), (size_t)n * P);          /* every voice's Sample is fresh */
    drain(s);
    /* olfx_sample_voices takes inst = kit * voices + p */
    const olfx_sample_voice rec{1 * P + 2, 1, OLFX_SAMPLE_LOOP, 0, 3, 20};
    EXPECT_EQ(s.sample_voices(&rec, 1), OLFX_OK);
    EXPECT_TRUE(s.vdirty_list == std::vector<uint32_t>{2 * n + 1});
    const olfx_sample_voice past{n * P, 0, 0, 0, 0, 0};
    EXPECT_EQ(s.sample_voices(&past, 1), OLFX_E_ARG);
    std::vector<uint32_t> w(VCC_N + SMC_N);
    s.derive_voice_record(2 * n + 1, w.data());
    EXPECT_EQ(w[VCC_N + SMC_BASE], 128u);                    /* the second sample's aligned start */
    EXPECT_EQ(w[VCC_N + SMC_LEN], 30u);
    EXPECT_EQ(w[VCC_N + SMC_LS], 3u);
    EXPECT_EQ(w[VCC_N + SMC_LE], 20u);
    EXPECT_EQ(w[VCC_N + SMC_MODE] & 1u, 1u);
    s.derive_voice_record(0 * n + 1, w.data());
    EXPECT_EQ(w[VCC_N + SMC_LEN], 0u);
    EXPECT_EQ(map1(s, 1, 2, 3, 64), OLFX_OK);
    EXPECT_EQ(note(s, 1, OLFX_EV_NOTE_ON, 64), OLFX_OK);
    const float v = 0.3f;
    EXPECT_EQ(s.set_range(1, 1, slot_field(2, 0), 1, &v), OLFX_OK);
    s.reset();
    EXPECT_EQ(s.note2voice[64 * n + 1], 2);
    EXPECT_EQ(s.chan2voice[3 * n + 1], 2);
    EXPECT_EQ(s.order_word(1), 0xFFFFFFF2u);
    EXPECT_EQ(s.samples[1 * P + 2].sample, 1u);
    EXPECT_EQ(s.bank.len.size(), (size_t)2);
    EXPECT_TRUE(s.events.empty());
    EXPECT_TRUE(playing(s, 1) == (std::vector<uint8_t>{0, 0, 0}));
    EXPECT_EQ(s.configured[2 * n + 1], 0);
    EXPECT_EQ(param(s, slot_field(2, 0), 1), 0.f);
    EXPECT_EQ(s.vdirty_list.size(), (size_t)n * P);
    EXPECT_EQ(s.dirty_list.size(), (size_t)n);
}

TEST(DrumKit, PacketHoldsTheWorstCase) {
    for (const uint32_t n : {1u, 63u, 65u, 130u})
        for (const uint32_t P : {1u, 4u, 8u}) {
            Shadow s;
            s.init(K, n, 48000.f, P);
            s.reset();                                        /* every kit and every voice slot dirty */
            for (uint32_t i = 0; i < n; ++i)
                for (uint32_t q = 0; q < P; ++q) {
                    EXPECT_EQ(map1(s, i, q, (uint8_t)q, (uint8_t)(30 + q)), OLFX_OK);
                    EXPECT_EQ(note(s, i, OLFX_EV_NOTE_ON, (uint8_t)(30 + q)), OLFX_OK);
                }
            EXPECT_EQ(s.events.size(), (size_t)n * P);        /* an event per voice */
            s.fold_events();
            const host::PacketPlan pl = s.plan(true);
            EXPECT_EQ(pl.m2, (size_t)n * P);
            EXPECT_TRUE(pl.words <= host::max_packet_words(K, n, s.n_ev()));
            /* the sections in order, none overlapping: kit list and records, slot list and records, events */
            EXPECT_TRUE(pl.dense && pl.o_val == 0);
            EXPECT_TRUE(pl.o_inst2 >= (size_t)n * (FRC_N + DKC_N));
            EXPECT_TRUE(pl.o_val2 >= pl.o_inst2 + (size_t)n * P);
            EXPECT_TRUE(pl.o_ev >= pl.o_val2 + (size_t)n * P * (VCC_N + SMC_N));
            std::vector<uint32_t> buf(pl.words, 0xDEADBEEFu);
            s.fill_records(pl, buf.data());
            s.write_events(buf.data() + pl.o_ev);
            /* the slot list holds device slots p * npad + kit, each once */
            std::vector<uint32_t> slots(buf.begin() + (long)pl.o_inst2, buf.begin() + (long)(pl.o_inst2 + pl.m2));
            slots = sorted(slots);
            for (uint32_t q = 0; q < P; ++q)
                for (uint32_t i = 0; i < n; ++i) EXPECT_EQ(slots[q * n + i], q * s.npad + i);
            /* the kit records' order words follow the map: voices 0 .. P-1 by ascending note */
            uint32_t want = kDkOrderEmpty;
            for (uint32_t q = 0; q < P; ++q) want = (want & ~(0xFu << (4 * q))) | q << (4 * q);
            for (uint32_t i = 0; i < n; ++i) EXPECT_EQ(buf[pl.o_val + (size_t)FRC_N * n + i], want);
            EXPECT_TRUE(s.dirty_list.empty() && s.vdirty_list.empty());
        }
}

int main() { return run_all_tests(); }
