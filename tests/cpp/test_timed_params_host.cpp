/*
 * tests/cpp/test_timed_params_host.cpp -- olfx_timed_params / olfx_timed_control in the engine's HIP-free host
 * core (ol_dsp_amd/csrc/olfx_host.h) on the CPU: the pending list's order, parameters ahead of events at a frame,
 * the carry-over, a record reaching frame 0 ahead of a later set_param, the shadow over time, UPDATE_ONLY
 * configuring a voice at its frame, validation (a refused call changes nothing), the refusals per kind, the span
 * at 16 and 17 mixed times and under the n-record bound, the timed section's offsets and base table at n = 1,
 * 64, 65 and 130, the worst packet against its bound, and a packet without timed parameter records against
 * today's.  Links olfx_host.cpp directly (no libolfx.so, no GPU); built by tests/test_timed_params_host.py with
 * its own build line.
 */
#include "../../ol_dsp_amd/csrc/olfx_host.h"
#include "harness.h"

#include <algorithm>
#include <cmath>

using namespace olfx;
using host::Shadow;

namespace {

Shadow fresh(int kind, uint32_t n) {
    Shadow s;
    s.init(kind, n, 48000.f);
    s.reset();
    const host::PacketPlan pl = s.plan(false);
    std::vector<uint32_t> buf(pl.words);
    s.fill_records(pl, buf.data());
    return s;
}

typedef struct olfx_timed_control TimedControl;     /* (the call hides the record's name) */
olfx_timed_param tp(uint32_t frame, uint32_t inst, uint32_t field, float value) { return olfx_timed_param{frame, inst, field, value}; }
olfx_timed_event tev(uint32_t frame, uint32_t inst, uint8_t type, uint8_t note = 60) {
    return olfx_timed_event{frame, olfx_voice_event{inst, type, note, 100, 0, 0.f}};
}
int queue(Shadow &s, const std::vector<olfx_timed_param> &r) { return s.timed_params(r.data(), (uint32_t)r.size()); }
int queue(Shadow &s, const std::vector<olfx_timed_event> &e) { return s.timed_events(e.data(), (uint32_t)e.size()); }
float param(const Shadow &s, uint32_t inst, uint32_t field) { return s.params[(size_t)field * s.n + inst]; }

/* the whole packet of the next launch of `span` frames, as the engine writes it */
std::vector<uint32_t> packet(Shadow &s, uint32_t span, host::PacketPlan *plan) {
    const bool evs = s.has_events(span);
    if (evs) s.fold_segments(span);
    const host::PacketPlan pl = s.plan(evs);
    std::vector<uint32_t> buf(pl.words + 4, 0xDEADBEEFu);
    s.fill_records(pl, buf.data());
    if (evs) s.write_events(buf.data() + pl.o_ev);
    if (pl.n_tc) s.write_timed_coefs(pl, buf.data());
    for (size_t k = pl.words; k < buf.size(); ++k) EXPECT_EQ(buf[k], 0xDEADBEEFu);       /* nothing past the plan */
    *plan = pl;
    buf.resize(pl.words);
    return buf;
}

/* a voice's coefficient record from the shadow as it stands */
std::vector<uint32_t> record_of(const Shadow &s, uint32_t v) {
    float p[OLFX_VC_NPARAMS];
    for (uint32_t f = 0; f < OLFX_VC_NPARAMS; ++f) p[f] = param(s, v, f);
    std::vector<uint32_t> w(VCC_N);
    host::derive_voice(p, s.configured[v] != 0, s.kd->moog, s.sr, w.data());
    return w;
}

constexpr uint8_t ON = OLFX_EV_NOTE_ON;
constexpr int kVoiceKinds[] = {OLFX_KIND_VOICE, OLFX_KIND_VOICE_MOOG, OLFX_KIND_VOICE_SAMPLE};
constexpr uint8_t CC_CUTOFF = 41;             /* corelib/cc_map.h CC_FILTER_CUTOFF */

}  // namespace

TEST(TimedParams, OrderByFrameThenArrival) {
    Shadow s = fresh(OLFX_KIND_VOICE, 130);
    EXPECT_EQ(queue(s, {tp(16, 1, OLFX_VC_FILTER_CUTOFF, 100.f), tp(8, 2, OLFX_VC_FILTER_CUTOFF, 200.f),
                        tp(16, 3, OLFX_VC_FILTER_CUTOFF, 300.f)}), OLFX_OK);
    /* a control between two parameter calls keeps its place in the one queueing order */
    const TimedControl c = {16, olfx_control_event{1, CC_CUTOFF, OLFX_CTL_HARDWARE, 0, 0.5f}};
    EXPECT_EQ(s.timed_control(&c, 1), OLFX_OK);
    EXPECT_EQ(queue(s, {tp(8, 4, OLFX_VC_FILTER_CUTOFF, 400.f), tp(16, 1, OLFX_VC_FILTER_CUTOFF, 500.f),
                        tp(72, 5, OLFX_VC_FILTER_CUTOFF, 600.f)}), OLFX_OK);
    const uint32_t want_frame[] = {8, 8, 16, 16, 16, 16, 72}, want_inst[] = {2, 4, 1, 3, 1, 1, 5};
    EXPECT_EQ(s.tparams.size(), (size_t)7);
    for (size_t k = 0; k < s.tparams.size() && k < 7; ++k) {
        EXPECT_EQ(s.tparams[k].frame, want_frame[k]);
        EXPECT_EQ(s.tparams[k].inst, want_inst[k]);
    }
    uint32_t f = 0;
    float v = 0.f;
    EXPECT_EQ(olfx_control_map(OLFX_KIND_VOICE, CC_CUTOFF, OLFX_CTL_HARDWARE, 0.5f, &f, &v), OLFX_OK);
    EXPECT_EQ(s.tparams[4].field, f);
    EXPECT_EQ(s.tparams[4].value, v);
    EXPECT_EQ(s.span(64), 64u);
    EXPECT_TRUE(s.has_events(64) && s.has_timed_params(64) && !s.has_timed_params(8));
    s.fold_segments(64);
    EXPECT_EQ(s.n_seg(), 3u);
    EXPECT_EQ(s.seg_frame[1], 8u);
    EXPECT_EQ(s.seg_frame[2], 16u);
    /* the last write of frame 16 on voice 1 wins; one record per voice and segment, by voice */
    EXPECT_EQ(param(s, 1, OLFX_VC_FILTER_CUTOFF), 500.f);
    const uint32_t want_tc[] = {2, 4, 1, 3};
    EXPECT_EQ(s.vrec.lane.size(), (size_t)4);
    for (size_t k = 0; k < 4 && k < s.vrec.lane.size(); ++k) EXPECT_EQ(s.vrec.lane[k], want_tc[k]);
    EXPECT_EQ(s.vrec.first[0], 0u);
    EXPECT_EQ(s.vrec.first[1], 0u);
    EXPECT_EQ(s.vrec.first[2], 2u);
    EXPECT_EQ(s.vrec.first[3], 4u);
    EXPECT_EQ(s.tparams.size(), (size_t)1);
    EXPECT_EQ(s.tparams[0].frame, 72u);
    for (size_t k = 0; k < s.folded.size(); ++k) EXPECT_EQ(s.folded[k].op, (uint32_t)VEV_COEF);   /* VEV_COEF alone */
}

TEST(TimedParams, ParametersPrecedeEventsAtAFrame) {
    /* the event is queued first; the record of the frame still carries the coefficients and the note in one record, and
       the coefficients are those of the parameter */
    Shadow s = fresh(OLFX_KIND_VOICE, 70);
    EXPECT_EQ(queue(s, {tev(8, 5, ON, 64), tev(8, 6, ON, 65)}), OLFX_OK);
    EXPECT_EQ(queue(s, {tp(8, 5, OLFX_VC_AMP_ATTACK, 0.25f)}), OLFX_OK);
    s.fold_segments(64);
    EXPECT_EQ(s.n_seg(), 2u);
    EXPECT_EQ(s.folded.size(), (size_t)2);
    EXPECT_EQ(s.folded[0].inst, 5u);
    EXPECT_EQ(s.folded[0].op, (uint32_t)(VEV_COEF | VEV_GATE_SET | VEV_GATE_ON | VEV_RETRIGGER | VEV_FREQ));
    EXPECT_EQ(s.folded[1].inst, 6u);
    EXPECT_EQ(s.folded[1].op, (uint32_t)(VEV_GATE_SET | VEV_GATE_ON | VEV_RETRIGGER | VEV_FREQ));
    EXPECT_EQ(s.vrec.lane.size(), (size_t)1);
    const std::vector<uint32_t> w = record_of(s, 5);
    for (uint32_t k = 0; k < VCC_N; ++k) EXPECT_EQ(s.vrec.words[k], w[k]);
    /* a NoteOff after the change keeps the bit */
    Shadow t = fresh(OLFX_KIND_VOICE_SAMPLE, 70);
    EXPECT_EQ(queue(t, {tp(12, 9, OLFX_VC_FILTER_CUTOFF, 900.f)}), OLFX_OK);
    EXPECT_EQ(queue(t, {tev(12, 9, OLFX_EV_NOTE_OFF)}), OLFX_OK);
    t.fold_segments(64);
    EXPECT_EQ(t.folded.size(), (size_t)1);
    EXPECT_EQ(t.folded[0].op, (uint32_t)(VEV_COEF | VEV_GATE_SET));
}

TEST(TimedParams, CarryOverTwoCallsAndFrameZeroFirst) {
    Shadow s = fresh(OLFX_KIND_VOICE_MOOG, 8);
    EXPECT_EQ(queue(s, {tp(64, 1, OLFX_VC_FILTER_CUTOFF, 111.f), tp(100, 2, OLFX_VC_FILTER_CUTOFF, 222.f),
                        tp(132, 3, OLFX_VC_FILTER_CUTOFF, 333.f)}), OLFX_OK);
    const float before = param(s, 1, OLFX_VC_FILTER_CUTOFF);
    /* call 1: 64 frames, nothing below the span */
    EXPECT_EQ(s.span(64), 64u);
    EXPECT_TRUE(!s.has_events(64));
    EXPECT_EQ(param(s, 1, OLFX_VC_FILTER_CUTOFF), before);
    s.advance(64);
    /* the record at frame 64 reached frame 0: applied at that boundary, dirty, no longer pending */
    EXPECT_EQ(param(s, 1, OLFX_VC_FILTER_CUTOFF), 111.f);
    EXPECT_EQ(s.configured[1], 1);
    EXPECT_EQ(s.dirty_list.size(), (size_t)1);
    EXPECT_EQ(s.tparams.size(), (size_t)2);
    EXPECT_EQ(s.tparams[0].frame, 36u);
    EXPECT_EQ(s.tparams[1].frame, 68u);
    /* ... ahead of anything set afterwards: a later set_param of the same field wins */
    const float later = 999.f;
    EXPECT_EQ(s.set_range(1, 1, OLFX_VC_FILTER_CUTOFF, 1, &later), OLFX_OK);
    EXPECT_EQ(param(s, 1, OLFX_VC_FILTER_CUTOFF), 999.f);
    /* call 2: the record at 36 is a segment, the one at 68 is carried again */
    EXPECT_EQ(s.span(64), 64u);
    EXPECT_TRUE(s.has_events(64));
    host::PacketPlan pl;
    packet(s, 64, &pl);
    EXPECT_EQ(pl.n_seg, (size_t)2);
    EXPECT_EQ(pl.n_tc, (size_t)1);
    EXPECT_EQ(param(s, 2, OLFX_VC_FILTER_CUTOFF), 222.f);
    s.advance(64);
    EXPECT_EQ(s.tparams.size(), (size_t)1);
    EXPECT_EQ(s.tparams[0].frame, 4u);
    EXPECT_EQ(param(s, 3, OLFX_VC_FILTER_CUTOFF), before);
    /* reset drops what is pending */
    s.reset();
    EXPECT_TRUE(s.tparams.empty());
}

TEST(TimedParams, ShadowOverTimeAndUntimedFirst) {
    Shadow s = fresh(OLFX_KIND_VOICE, 4);
    const float d = param(s, 0, OLFX_VC_FILTER_RESONANCE);
    EXPECT_EQ(queue(s, {tp(0, 0, OLFX_VC_FILTER_RESONANCE, 0.1f), tp(8, 0, OLFX_VC_FILTER_RESONANCE, 0.2f),
                        tp(40, 0, OLFX_VC_FILTER_RESONANCE, 0.3f)}), OLFX_OK);
    EXPECT_TRUE(d != 0.1f);
    EXPECT_EQ(param(s, 0, OLFX_VC_FILTER_RESONANCE), 0.1f);                 /* frame 0: set_param now */
    EXPECT_EQ(s.configured[0], 1);
    /* an untimed write lands at the boundary, before every pending record: the record at 8 overrides it */
    const float u = 0.9f;
    EXPECT_EQ(s.set_range(0, 1, OLFX_VC_FILTER_RESONANCE, 1, &u), OLFX_OK);
    EXPECT_EQ(param(s, 0, OLFX_VC_FILTER_RESONANCE), 0.9f);
    host::PacketPlan pl;
    const std::vector<uint32_t> buf = packet(s, 32, &pl);                   /* frames 0 .. 32 */
    EXPECT_EQ(param(s, 0, OLFX_VC_FILTER_RESONANCE), 0.2f);
    /* the frame-0 record in the packet is the untimed value's, the segment's the timed one's */
    {
        Shadow r = fresh(OLFX_KIND_VOICE, 4);
        EXPECT_EQ(r.set_range(0, 1, OLFX_VC_FILTER_RESONANCE, 1, &u), OLFX_OK);
        const std::vector<uint32_t> w0 = record_of(r, 0), w1 = record_of(s, 0);
        EXPECT_TRUE(w0[VCC_DAMP_RES] != w1[VCC_DAMP_RES]);
        EXPECT_EQ(pl.n_tc, (size_t)1);
        for (uint32_t k = 0; k < VCC_N; ++k) {
            EXPECT_EQ(buf[pl.o_val + k], w0[k]);                            /* m = 1: [W][1] */
            EXPECT_EQ(buf[pl.o_tc + k], w1[k]);
        }
    }
    /* the changed voice stays dirty: its last record goes to the device arrays ahead of the next launch */
    EXPECT_EQ(s.dirty_list.size(), (size_t)1);
    EXPECT_EQ(s.dirty_list[0], 0u);
    s.advance(32);
    EXPECT_EQ(param(s, 0, OLFX_VC_FILTER_RESONANCE), 0.2f);
    packet(s, 32, &pl);                                                     /* frames 32 .. 64: the record at 40 */
    EXPECT_EQ(param(s, 0, OLFX_VC_FILTER_RESONANCE), 0.3f);
    /* olfx_set_member's OLFX_E_STATE rule is judged on the same state */
    EXPECT_EQ(s.set_member(0, OLFX_VC_AMP_ATTACK, 0.5f), OLFX_E_STATE);
    EXPECT_EQ(s.set_member(1, OLFX_VC_AMP_ATTACK, 0.5f), OLFX_OK);
}

TEST(TimedParams, TheKeptRecordIsTheOneScattered) {
    /* the voices a launch changed stay dirty, and the record the next launch scatters is their last timed one: equal
       to the derivation from the shadow, kept only until something writes to the voice again */
    for (const int kind : kVoiceKinds) {
        Shadow s = fresh(kind, 70);
        EXPECT_EQ(queue(s, {tp(8, 3, OLFX_VC_FILTER_CUTOFF, 100.f), tp(8, 69, OLFX_VC_AMP_RELEASE, 0.3f),
                            tp(24, 3, OLFX_VC_FILTER_RESONANCE, 0.7f), tp(24, 5, OLFX_VC_PORTAMENTO, 0.02f)}), OLFX_OK);
        host::PacketPlan pl;
        packet(s, 64, &pl);
        EXPECT_EQ(pl.n_tc, (size_t)4);
        EXPECT_EQ(s.dirty_list.size(), (size_t)3);
        EXPECT_TRUE(s.kept_voice.find(3) != nullptr && s.kept_voice.find(5) != nullptr && s.kept_voice.find(69) != nullptr && s.kept_voice.find(4) == nullptr);
        s.advance(64);
        const float v = 0.9f;
        EXPECT_EQ(s.set_range(5, 1, OLFX_VC_PORTAMENTO, 1, &v), OLFX_OK);       /* voice 5: written again */
        EXPECT_TRUE(s.kept_voice.find(5) == nullptr && s.kept_voice.find(3) != nullptr);
        const std::vector<uint32_t> dirty(s.dirty_list);
        const std::vector<uint32_t> buf = packet(s, 64, &pl);
        EXPECT_EQ(pl.n_seg, (size_t)1);
        const size_t m = dirty.size();
        for (size_t r = 0; r < m; ++r) {
            const std::vector<uint32_t> w = record_of(s, dirty[r]);
            EXPECT_EQ(buf[pl.o_inst + r], dirty[r]);
            for (uint32_t k = 0; k < VCC_N; ++k) EXPECT_EQ(buf[pl.o_val + (size_t)k * m + r], w[k]);
        }
        EXPECT_TRUE(s.dirty_list.empty() && s.kept_voice.words.empty() && s.kept_voice.list.empty() && s.kept_voice.find(3) == nullptr);
    }
}

TEST(TimedParams, UpdateOnlyConfiguresAtItsFrame) {
    /* a control that maps to OLFX_FIELD_UPDATE_ONLY: found by asking the map */
    int cc = -1;
    for (int k = 0; k < 128 && cc < 0; ++k) {
        uint32_t f = 0;
        float v = 0.f;
        if (olfx_control_map(OLFX_KIND_VOICE, (uint8_t)k, OLFX_CTL_MIDI, 64.f, &f, &v) == OLFX_OK && f == OLFX_FIELD_UPDATE_ONLY) cc = k;
    }
    int ignored = -1;
    for (int k = 0; k < 128 && ignored < 0; ++k) {
        uint32_t f = 0;
        float v = 0.f;
        if (olfx_control_map(OLFX_KIND_VOICE, (uint8_t)k, OLFX_CTL_MIDI, 64.f, &f, &v) == OLFX_IGNORED) ignored = k;
    }
    EXPECT_TRUE(ignored >= 0);
    Shadow s = fresh(OLFX_KIND_VOICE, 4);
    /* a control the reference ignores is skipped */
    const TimedControl ig = {8, olfx_control_event{2, (uint8_t)ignored, OLFX_CTL_MIDI, 0, 64.f}};
    EXPECT_EQ(s.timed_control(&ig, 1), OLFX_OK);
    EXPECT_TRUE(s.tparams.empty());
    EXPECT_TRUE(cc >= 0);
    if (cc < 0) return;
    const TimedControl c = {8, olfx_control_event{2, (uint8_t)cc, OLFX_CTL_MIDI, 0, 64.f}};
    EXPECT_EQ(s.timed_control(&c, 1), OLFX_OK);
    EXPECT_EQ(s.tparams.size(), (size_t)1);
    EXPECT_EQ(s.tparams[0].field, OLFX_FIELD_UPDATE_ONLY);
    EXPECT_EQ(s.configured[2], 0);
    const std::vector<uint32_t> w0 = record_of(s, 2);
    const std::vector<float> p0(s.params);
    s.fold_segments(16);
    EXPECT_EQ(s.configured[2], 1);
    EXPECT_TRUE(s.params == p0);              /* members unchanged */
    EXPECT_EQ(s.vrec.lane.size(), (size_t)1);
    const std::vector<uint32_t> w1 = record_of(s, 2);
    EXPECT_TRUE(w0 != w1);                    /* Init's component defaults -> the members' */
    for (uint32_t k = 0; k < VCC_N; ++k) EXPECT_EQ(s.vrec.words[k], w1[k]);
}

TEST(TimedParams, RefusedCallsChangeNothing) {
    for (const int kind : kVoiceKinds) {
        Shadow s = fresh(kind, 10);
        EXPECT_EQ(queue(s, {tp(8, 1, OLFX_VC_FILTER_CUTOFF, 100.f)}), OLFX_OK);
        EXPECT_EQ(queue(s, {tev(8, 1, ON)}), OLFX_OK);
        const std::vector<float> p0(s.params);
        const std::vector<uint8_t> c0(s.configured);
        const auto same = [&] {
            return s.params == p0 && s.configured == c0 && s.tparams.size() == 1 && s.timed.size() == 1 && s.dirty_list.empty();
        };
        const float nan = std::nanf(""), inf = HUGE_VALF;
        /* a good record first in each call: nothing of a refused call is queued or applied */
        const olfx_timed_param good = tp(0, 2, OLFX_VC_FILTER_CUTOFF, 50.f);
        EXPECT_EQ(s.timed_params(nullptr, 1), OLFX_E_ARG);
        EXPECT_TRUE(same());
        for (const olfx_timed_param &bad : {tp(6, 1, 0, 1.f), tp(0x80000000u, 1, 0, 1.f), tp(8, 10, 0, 1.f),
                                             tp(8, 1, OLFX_VC_NPARAMS, 1.f), tp(8, 1, OLFX_FIELD_UPDATE_ONLY, 1.f),
                                             tp(8, 1, OLFX_VC_FILTER_CUTOFF, nan), tp(0, 1, OLFX_VC_FILTER_CUTOFF, inf)}) {
            EXPECT_EQ(queue(s, {good, bad}), OLFX_E_ARG);
            EXPECT_TRUE(same());
        }
        const TimedControl cgood = {0, olfx_control_event{2, CC_CUTOFF, OLFX_CTL_MIDI, 0, 64.f}};
        EXPECT_EQ(s.timed_control(nullptr, 1), OLFX_E_ARG);
        for (const TimedControl &bad :
             {TimedControl{2, olfx_control_event{1, CC_CUTOFF, OLFX_CTL_MIDI, 0, 64.f}},
              TimedControl{0x80000004u, olfx_control_event{1, CC_CUTOFF, OLFX_CTL_MIDI, 0, 64.f}},
              TimedControl{8, olfx_control_event{10, CC_CUTOFF, OLFX_CTL_MIDI, 0, 64.f}},
              TimedControl{8, olfx_control_event{1, CC_CUTOFF, 7, 0, 64.f}},
              TimedControl{8, olfx_control_event{1, CC_CUTOFF, OLFX_CTL_HARDWARE, 0, nan}}}) {
            const TimedControl two[2] = {cgood, bad};
            /* olfx_control refuses the same record (a frame aside) */
            if (!(bad.frame & 3u) && bad.frame < 0x80000000u) {
                Shadow r = fresh(kind, 10);
                EXPECT_TRUE(r.control(&bad.ev, 1) != OLFX_OK);
            }
            EXPECT_EQ(s.timed_control(two, 2), OLFX_E_ARG);
            EXPECT_TRUE(same());
        }
        EXPECT_EQ(s.timed_params(nullptr, 0), OLFX_OK);
        EXPECT_EQ(s.timed_control(nullptr, 0), OLFX_OK);
        EXPECT_TRUE(same());
    }
}

TEST(TimedParams, OtherKindsRefuse) {
    for (int kind = 1; kind <= OLFX_KIND_METER_MONO; ++kind) {
        if (!host::kind_desc(kind).nparts) continue;
        bool voice = false;
        for (const int k : kVoiceKinds) voice = voice || k == kind;
        Shadow s = fresh(kind, 3);
        const olfx_timed_param r = tp(8, 0, 0, 0.5f);
        const TimedControl c = {8, olfx_control_event{0, CC_CUTOFF, OLFX_CTL_MIDI, 0, 64.f}};
        EXPECT_EQ(s.timed_params(&r, 1), voice ? OLFX_OK : OLFX_E_KIND);
        EXPECT_EQ(s.timed_control(&c, 1), voice ? OLFX_OK : OLFX_E_KIND);
        EXPECT_EQ(s.tparams.size(), voice ? (size_t)2 : (size_t)0);
        EXPECT_EQ(host::max_timed_param_words(kind, 3) != 0, voice);
    }
}

TEST(TimedParams, SpanCountsTheUnionOfTimes) {
    /* 15 times past frame 0 are 16 segments: events at 4, 12, 20 ..., parameters at 8, 16, ... and both at 60 */
    Shadow s = fresh(OLFX_KIND_VOICE, 130);
    for (uint32_t k = 1; k <= 15; ++k) {
        if (k & 1 || k == 15) EXPECT_EQ(queue(s, {tev(4 * k, k, ON)}), OLFX_OK);
        if (!(k & 1) || k == 15) EXPECT_EQ(queue(s, {tp(4 * k, k, OLFX_VC_FILTER_CUTOFF, 100.f * (float)k)}), OLFX_OK);
    }
    EXPECT_EQ(s.span(128), 128u);
    /* a 17th time, whichever list holds it, ends the launch there */
    Shadow a = s, b = s;
    EXPECT_EQ(queue(a, {tev(64, 1, ON)}), OLFX_OK);
    EXPECT_EQ(a.span(128), 64u);
    EXPECT_EQ(queue(b, {tp(64, 1, OLFX_VC_FILTER_CUTOFF, 1.f)}), OLFX_OK);
    EXPECT_EQ(b.span(128), 64u);
    EXPECT_EQ(b.span(64), 64u);
    b.fold_segments(64);
    EXPECT_EQ(b.n_seg(), kSegCap);
    for (uint32_t k = 0; k < kSegCap; ++k) EXPECT_EQ(b.seg_frame[k], 4 * k);
    EXPECT_EQ(b.vrec.lane.size(), (size_t)8);
    EXPECT_EQ(b.n_chunks(64, 8), (uint32_t)kSegCap);
    b.advance(64);
    EXPECT_TRUE(b.tparams.empty() && b.timed.empty());
    EXPECT_EQ(param(b, 1, OLFX_VC_FILTER_CUTOFF), 1.f);                     /* frame 64 became frame 0 */
}

TEST(TimedParams, SpanCutByTheRecordBound) {
    /* n = 65: 65 records at one time fill the launch; one more at the next time ends it there */
    Shadow s = fresh(OLFX_KIND_VOICE, 65);
    std::vector<olfx_timed_param> r;
    for (uint32_t i = 0; i < 65; ++i) r.push_back(tp(8, i, OLFX_VC_FILTER_CUTOFF, 100.f + (float)i));
    for (uint32_t i = 0; i < 65; ++i) r.push_back(tp(8, i, OLFX_VC_FILTER_RESONANCE, 0.3f));   /* the same voices: no more records */
    r.push_back(tp(16, 7, OLFX_VC_FILTER_CUTOFF, 1.f));
    EXPECT_EQ(queue(s, r), OLFX_OK);
    EXPECT_EQ(s.span(64), 16u);
    host::PacketPlan pl;
    packet(s, 16, &pl);
    EXPECT_EQ(pl.n_tc, (size_t)65);
    EXPECT_EQ(pl.n_seg, (size_t)2);
    s.advance(16);
    EXPECT_EQ(param(s, 7, OLFX_VC_FILTER_CUTOFF), 1.f);
    EXPECT_EQ(s.span(48), 48u);
    /* 64 records and one more fit */
    Shadow t = fresh(OLFX_KIND_VOICE, 65);
    r.clear();
    for (uint32_t i = 0; i < 64; ++i) r.push_back(tp(8, i, OLFX_VC_FILTER_CUTOFF, 100.f));
    r.push_back(tp(16, 7, OLFX_VC_FILTER_CUTOFF, 1.f));
    r.push_back(tp(20, 8, OLFX_VC_FILTER_CUTOFF, 1.f));
    EXPECT_EQ(queue(t, r), OLFX_OK);
    EXPECT_EQ(t.span(64), 20u);
}

TEST(TimedParams, OffsetsAndBaseTableBySize) {
    const auto up4 = [](size_t w) { return (w + 3) & ~(size_t)3; };
    for (const int kind : kVoiceKinds)
        for (const uint32_t n : {1u, 64u, 65u, 130u}) {
            Shadow s = fresh(kind, n);
            /* segment 1 (frame 8): every third voice; segment 2 (frame 12): an event only; segment 3 (frame 24): the highest
               voices, as many as the launch's bound of n records leaves (none at n = 1: three segments) */
            std::vector<olfx_timed_param> r;
            std::vector<uint32_t> third;
            for (uint32_t i = 0; i < n; i += 3) {
                r.push_back(tp(8, i, OLFX_VC_FILTER_CUTOFF, 50.f + (float)i));
                third.push_back(i);
            }
            for (uint32_t i = n; i-- > 0;) r.push_back(tp(24, i, OLFX_VC_FILTER_ENV_AMOUNT, 0.01f * (float)i));
            if (r.size() > n) r.resize(third.size() + (n - third.size()));   /* the bound: n records in the launch */
            EXPECT_EQ(queue(s, r), OLFX_OK);
            EXPECT_EQ(queue(s, {tev(12, 0, ON)}), OLFX_OK);
            EXPECT_EQ(s.span(64), 64u);
            host::PacketPlan pl;
            const std::vector<uint32_t> buf = packet(s, 64, &pl);
            const size_t groups = (n + 63) / 64, T = s.vrec.lane.size();
            const size_t nseg = 3 + (n > third.size());
            EXPECT_EQ(pl.n_seg, nseg);
            EXPECT_EQ(T, (size_t)n);
            EXPECT_EQ(pl.n_tc, T);
            EXPECT_EQ(pl.o_tcb, up4(pl.o_seg + ((nseg + 1) & ~(size_t)1)));
            EXPECT_EQ(pl.o_tc, up4(pl.o_tcb + nseg * groups));
            EXPECT_EQ(pl.words, pl.o_tc + VCC_N * T);
            const uint32_t *base = buf.data() + pl.o_tcb;
            /* the base table restated: a segment's records by voice, a group's run where the lower groups' end */
            size_t before = 0;
            for (size_t sgm = 0; sgm < nseg; ++sgm) {
                std::vector<uint32_t> in(s.vrec.lane.begin() + s.vrec.first[sgm], s.vrec.lane.begin() + s.vrec.first[sgm + 1]);
                EXPECT_TRUE(std::is_sorted(in.begin(), in.end()));
                for (size_t g = 0; g < groups; ++g) {
                    size_t lower = 0;
                    for (const uint32_t v : in) lower += (v >> 6) < g;
                    EXPECT_EQ((size_t)base[sgm * groups + g], before + lower);
                }
                /* every record where the kernel looks for it: base + the group's lower voices with a record */
                for (const uint32_t v : in) {
                    size_t rank = 0;
                    for (const uint32_t u : in) rank += (u >> 6) == (v >> 6) && u < v;
                    const size_t rec = base[sgm * groups + (v >> 6)] + rank;
                    EXPECT_TRUE(rec < T);
                    EXPECT_EQ(s.vrec.lane[rec], v);
                    for (uint32_t w = 0; w < VCC_N; ++w) EXPECT_EQ(buf[pl.o_tc + (size_t)w * T + rec], s.vrec.words[rec * VCC_N + w]);
                }
                before += in.size();
            }
            EXPECT_EQ(s.vrec.first[1], 0u);
            EXPECT_EQ((size_t)s.vrec.first[2], third.size());
            EXPECT_EQ(s.vrec.first[3], s.vrec.first[2]);
        }
}

TEST(TimedParams, WorstPacketReachesTheBound) {
    /* every voice with an event in every segment, every coefficient dirty, and n coefficient records in the last
       segment: the event part is max_packet_words', the timed section max_timed_param_words' to the word (its
       leading alignment aside) */
    const auto up4 = [](size_t w) { return (w + 3) & ~(size_t)3; };
    for (const int kind : kVoiceKinds)
        for (const uint32_t n : {64u, 130u}) {
            Shadow s;
            s.init(kind, n, 48000.f);
            s.reset();                                                     /* all dirty */
            std::vector<olfx_timed_event> evs;
            for (uint32_t k = 0; k < kSegCap; ++k)
                for (uint32_t i = 0; i < n; ++i) evs.push_back(tev(4 * k, i, ON));
            EXPECT_EQ(queue(s, evs), OLFX_OK);
            std::vector<olfx_timed_param> r;
            for (uint32_t i = 0; i < n; ++i) r.push_back(tp(60, i, OLFX_VC_FILTER_CUTOFF, 100.f));
            r.push_back(tp(64, 0, OLFX_VC_FILTER_CUTOFF, 100.f));
            EXPECT_EQ(queue(s, r), OLFX_OK);
            EXPECT_EQ(s.span(128), 64u);
            host::PacketPlan pl;
            packet(s, 64, &pl);
            const size_t groups = (n + 63) / 64;
            EXPECT_EQ(pl.n_seg, (size_t)kSegCap);
            EXPECT_EQ(pl.n_tc, (size_t)n);
            EXPECT_EQ(pl.words - pl.o_tcb, up4(kSegCap * groups) + (size_t)VCC_N * n);
            EXPECT_EQ(pl.words - pl.o_tcb + 3, host::max_timed_param_words(kind, n));
            EXPECT_TRUE(pl.o_tcb - (pl.o_seg + kSegCap) <= 3);
            EXPECT_TRUE(pl.o_seg + kSegCap <= host::max_packet_words(kind, n, 0, kSegCap));
            EXPECT_TRUE(pl.words <= host::max_packet_words(kind, n, 0, kSegCap) + host::max_timed_param_words(kind, n));
            /* max_packet_words keeps its value: the timed section is a figure of its own */
            const size_t W = s.kd->words;
            EXPECT_EQ(host::max_packet_words(kind, n, 0, kSegCap),
                      n + W * n + 2 * (size_t)kSegCap * (groups * kVevCap + n) + kSegCap + 16);
        }
}

TEST(TimedParams, NoTimedRecordNoChange) {
    /* timed events alone, a parameter record at frame 0, and one past the span: the packet is today's, word for word
       (the same shadow driven by set_param and timed events only) */
    for (const int kind : kVoiceKinds) {
        Shadow a = fresh(kind, 130), b = fresh(kind, 130);
        const std::vector<olfx_timed_event> evs = {tev(8, 3, ON), tev(8, 70, ON, 62), tev(24, 129, OLFX_EV_NOTE_OFF), tev(0, 5, ON)};
        EXPECT_EQ(queue(a, evs), OLFX_OK);
        EXPECT_EQ(queue(b, evs), OLFX_OK);
        EXPECT_EQ(queue(a, {tp(0, 9, OLFX_VC_FILTER_CUTOFF, 700.f), tp(64, 9, OLFX_VC_FILTER_CUTOFF, 800.f)}), OLFX_OK);
        const float v = 700.f;
        EXPECT_EQ(b.set_range(9, 1, OLFX_VC_FILTER_CUTOFF, 1, &v), OLFX_OK);
        EXPECT_EQ(a.span(64), b.span(64));
        host::PacketPlan pa, pb;
        const std::vector<uint32_t> wa = packet(a, 64, &pa), wb = packet(b, 64, &pb);
        EXPECT_EQ(pa.n_tc, (size_t)0);
        EXPECT_EQ(pa.o_tcb, (size_t)0);
        EXPECT_EQ(pa.words, pb.words);
        EXPECT_TRUE(wa == wb);
        EXPECT_TRUE(a.dirty_list.empty());
        /* ... and with nothing but the frame-0 write, the unsegmented packet */
        Shadow c = fresh(kind, 130), d = fresh(kind, 130);
        EXPECT_EQ(queue(c, {tp(0, 9, OLFX_VC_FILTER_CUTOFF, 700.f), tp(64, 9, OLFX_VC_FILTER_CUTOFF, 800.f)}), OLFX_OK);
        EXPECT_EQ(d.set_range(9, 1, OLFX_VC_FILTER_CUTOFF, 1, &v), OLFX_OK);
        EXPECT_TRUE(!c.has_events(64));
        const std::vector<uint32_t> wc = packet(c, 64, &pa), wd = packet(d, 64, &pb);
        EXPECT_EQ(pa.n_seg, (size_t)1);
        EXPECT_TRUE(wc == wd);
    }
}

int main() { return run_all_tests(); }
