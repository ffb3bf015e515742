/*
 * tests/cpp/test_timed_instrument_params_host.cpp -- olfx_timed_instrument_params / olfx_timed_instrument_control in
 * the engine's HIP-free host core (ol_dsp_amd/csrc/olfx_host.h) on the CPU, for OLFX_KIND_SYNTH, OLFX_KIND_SYNTH_SVF
 * and OLFX_KIND_DRUMKIT: parameters ahead of notes at a time, a control mapped at its frame (under the topology and
 * the channel2voice table of that moment), the carry-over, the launch's end at a boundary field, the union of times
 * against the 16 segments and the record cap on both sides, validation (a refused call changes nothing), the
 * refusals per kind, the section's offsets, tables and records at n = 1, 65, 130 and 8230, a fold without records
 * against the packet of the untouched path, the reads over time and the kept records.  Links olfx_host.cpp directly
 * (no libolfx.so, no GPU); built by tests/test_timed_instrument_params_host.py with its own build line.
 */
#include "../../ol_dsp_amd/csrc/olfx_host.h"
#include "harness.h"

#include <algorithm>
#include <cmath>
#include <cstring>

using namespace olfx;
using host::Shadow;

namespace {

Shadow fresh(int kind, uint32_t n, uint32_t voices = 4) {
    Shadow s;
    s.init(kind, n, 48000.f, voices);
    s.reset();
    const host::PacketPlan pl = s.plan(false);
    std::vector<uint32_t> buf(pl.words);
    s.fill_records(pl, buf.data());
    return s;
}

typedef struct olfx_timed_control TimedControl;     /* (the call hides the record's name) */
olfx_timed_param tp(uint32_t frame, uint32_t inst, uint32_t field, float value) { return olfx_timed_param{frame, inst, field, value}; }
TimedControl tc(uint32_t frame, uint32_t inst, uint8_t cc, float value, uint16_t pad = 0, uint8_t source = OLFX_CTL_MIDI) {
    return TimedControl{frame, olfx_control_event{inst, cc, source, pad, value}};
}
olfx_timed_note tn(uint32_t frame, uint32_t inst, uint8_t type, uint8_t note = 60) {
    return olfx_timed_note{frame, olfx_event{inst, type, note, 100, 0}};
}
int queue(Shadow &s, const std::vector<olfx_timed_param> &r) { return s.timed_instrument_params(r.data(), (uint32_t)r.size()); }
int queue(Shadow &s, const std::vector<TimedControl> &r) { return s.timed_instrument_control(r.data(), (uint32_t)r.size()); }
int queue(Shadow &s, const std::vector<olfx_timed_note> &e) { return s.timed_notes(e.data(), (uint32_t)e.size()); }
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
    if (pl.n_iv + pl.n_if) s.write_timed_inst(pl, buf.data());
    for (size_t k = pl.words; k < buf.size(); ++k) EXPECT_EQ(buf[k], 0xDEADBEEFu);       /* nothing past the plan */
    *plan = pl;
    buf.resize(pl.words);
    return buf;
}
/* one launch as olfx_process runs it: the span, the packet, the advance; returns the span */
uint32_t launch(Shadow &s, uint32_t frames, host::PacketPlan *plan = nullptr, std::vector<uint32_t> *buf = nullptr) {
    const uint32_t span = s.span(frames);
    host::PacketPlan pl;
    std::vector<uint32_t> b = packet(s, span, &pl);
    s.advance(span);
    if (plan) *plan = pl;
    if (buf) buf->swap(b);
    return span;
}

/* a synth instrument's (slot = 0) or a kit voice slot's voice record from the shadow as it stands */
std::vector<uint32_t> voice_record(const Shadow &s, uint32_t inst, uint32_t slot = 0) {
    float p[OLFX_VC_NPARAMS];
    for (uint32_t f = 0; f < OLFX_VC_NPARAMS; ++f) p[f] = param(s, inst, s.kd->voice0 + slot * OLFX_VC_NPARAMS + f);
    std::vector<uint32_t> w(VCC_N);
    host::derive_voice(p, s.configured[s.kit() ? slot * s.n + inst : inst] != 0, s.kd->moog, s.sr, w.data());
    return w;
}
std::vector<uint32_t> rack_record(const Shadow &s, uint32_t inst) {
    float p[OLFX_FR_NPARAMS];
    const uint32_t rack0 = s.kd->topo_field - OLFX_FR_TOPOLOGY;
    for (uint32_t f = 0; f < OLFX_FR_NPARAMS; ++f) p[f] = param(s, inst, rack0 + f);
    uint32_t w[FRC_N];
    host::derive_fxrack(p, s.sr, w);
    return std::vector<uint32_t>(w + FRC_RBAL, w + FRC_RBAL + TIF_N);
}

constexpr uint8_t ON = OLFX_EV_NOTE_ON;
constexpr int kInstrumentKinds[] = {OLFX_KIND_SYNTH, OLFX_KIND_SYNTH_SVF, OLFX_KIND_DRUMKIT};
constexpr uint8_t CC_VOLUME = 7, CC_DELAY_TIME = 35, CC_CUTOFF = 41, CC_FX_CUTOFF = 45, CC_OSC_1_VOLUME = 114;   /* corelib/cc_map.h */
uint32_t rack0_of(int kind) { return kind == OLFX_KIND_DRUMKIT ? OLFX_DK_RACK0 : OLFX_SY_RACK0; }

/* everything a refused call must leave alone */
struct Snapshot {
    std::vector<float> params;
    std::vector<uint8_t> configured, playing;
    std::vector<uint32_t> dirty, vdirty;
    size_t pending, notes, events;
    explicit Snapshot(const Shadow &s)
        : params(s.params), configured(s.configured), playing(s.playing), dirty(s.dirty_list), vdirty(s.vdirty_list),
          pending(s.iparams.size()), notes(s.timed.size()), events(s.events.size()) {}
    bool same(const Shadow &s) const {
        return params.size() == s.params.size() && !std::memcmp(params.data(), s.params.data(), params.size() * 4) &&
               configured == s.configured && playing == s.playing && dirty == s.dirty_list && vdirty == s.vdirty_list &&
               pending == s.iparams.size() && notes == s.timed.size() && events == s.events.size();
    }
};

}  // namespace

TEST(TimedInstrumentParams, OneOrderForBothCallsAndParametersPrecedeNotes) {
    Shadow s = fresh(OLFX_KIND_SYNTH, 130);
    /* the note is queued first; at frame 8 the record still lands ahead of it */
    EXPECT_EQ(queue(s, {tn(8, 5, ON, 64)}), OLFX_OK);
    EXPECT_EQ(queue(s, {tp(16, 1, OLFX_SY_VOICE0 + OLFX_VC_FILTER_CUTOFF, 100.f), tp(8, 5, OLFX_SY_VOICE0 + OLFX_VC_AMP_ATTACK, 0.25f)}), OLFX_OK);
    EXPECT_EQ(queue(s, {tc(16, 1, CC_CUTOFF, 64.f)}), OLFX_OK);
    EXPECT_EQ(queue(s, {tp(16, 1, OLFX_SY_VOICE0 + OLFX_VC_FILTER_CUTOFF, 500.f), tp(72, 2, OLFX_SY_VOICE0 + OLFX_VC_FILTER_CUTOFF, 600.f)}), OLFX_OK);
    const uint32_t want_frame[] = {8, 16, 16, 16, 72};
    const bool want_ctl[] = {false, false, true, false, false};
    EXPECT_EQ(s.iparams.size(), (size_t)5);
    for (size_t k = 0; k < s.iparams.size() && k < 5; ++k) {
        EXPECT_EQ(s.iparams[k].frame, want_frame[k]);
        EXPECT_EQ(s.iparams[k].ctl, want_ctl[k]);
    }
    EXPECT_TRUE(s.has_events(64) && s.has_timed_inst(64) && !s.has_timed_inst(8));
    EXPECT_EQ(s.span(64), 64u);
    const float rack_cutoff = param(s, 1, OLFX_SY_RACK0 + OLFX_FR_FILTER_CUTOFF);
    s.fold_segments(64);
    EXPECT_EQ(s.n_seg(), 3u);
    EXPECT_EQ(s.seg_frame[1], 8u);
    EXPECT_EQ(s.seg_frame[2], 16u);
    /* segment 1: instrument 5's voice record, as the parameter leaves it, and the note routed after it */
    EXPECT_EQ(s.vrec.first[1], 0u);
    EXPECT_EQ(s.vrec.first[2], 1u);
    EXPECT_EQ(s.vrec.lane[0], 5u);
    EXPECT_EQ(param(s, 5, OLFX_SY_VOICE0 + OLFX_VC_AMP_ATTACK), 0.25f);
    EXPECT_EQ(s.configured[5], 1);
    const std::vector<uint32_t> w5 = voice_record(s, 5);
    for (uint32_t k = 0; k < VCC_N; ++k) EXPECT_EQ(s.vrec.words[k], w5[k]);
    EXPECT_EQ(s.seg_first[2] - s.seg_first[1], 1u);
    EXPECT_EQ(s.folded[s.seg_first[1]].inst, 5u);            /* voice 0 of instrument 5 */
    EXPECT_EQ(s.playing[5], 64);
    /* segment 2: the last write of frame 16 wins on the voice; the control between the writes hit the rack too (CC 41
       at topology 1 reaches FILTER_CUTOFF): one voice record and one rack record for instrument 1 */
    EXPECT_EQ(param(s, 1, OLFX_SY_VOICE0 + OLFX_VC_FILTER_CUTOFF), 500.f);
    EXPECT_TRUE(param(s, 1, OLFX_SY_RACK0 + OLFX_FR_FILTER_CUTOFF) != rack_cutoff);
    EXPECT_EQ(s.vrec.first[3], 2u);
    EXPECT_EQ(s.vrec.lane[1], 1u);
    EXPECT_EQ(s.frec.first[2], 0u);
    EXPECT_EQ(s.frec.first[3], 1u);
    EXPECT_EQ(s.frec.lane[0], 1u);
    const std::vector<uint32_t> f1 = rack_record(s, 1);
    for (uint32_t k = 0; k < TIF_N; ++k) EXPECT_EQ(s.frec.words[k], f1[k]);
    EXPECT_EQ(s.iparams.size(), (size_t)1);
    EXPECT_EQ(s.iparams[0].frame, 72u);
    /* no record touched the dirty lists; fill_records puts the changed instruments back, each once */
    EXPECT_TRUE(s.dirty_list.empty());
    const host::PacketPlan pl = s.plan(true);
    std::vector<uint32_t> buf(pl.words);
    s.fill_records(pl, buf.data());
    std::vector<uint32_t> d = s.dirty_list;
    std::sort(d.begin(), d.end());
    EXPECT_TRUE(d == (std::vector<uint32_t>{1, 5}));
}

TEST(TimedInstrumentParams, ControlMappedAtItsFrame) {
    /* the Svf synth: CC 45 reaches FILTER_CUTOFF at topology 0 and nothing at topology 1.  With a TOPOLOGY record at
       frame 8 the control at frame 12 maps under the new topology; queued alone it is ignored */
    Shadow a = fresh(OLFX_KIND_SYNTH_SVF, 8), b = fresh(OLFX_KIND_SYNTH_SVF, 8);
    const uint32_t cutoff = OLFX_SY_RACK0 + OLFX_FR_FILTER_CUTOFF, topo = OLFX_SY_RACK0 + OLFX_FR_TOPOLOGY;
    const float before = param(a, 3, cutoff);
    EXPECT_EQ(param(a, 3, topo), 1.f);
    EXPECT_EQ(queue(a, {tc(12, 3, CC_FX_CUTOFF, 32.f)}), OLFX_OK);
    EXPECT_EQ(queue(a, {tp(8, 3, topo, 0.f)}), OLFX_OK);
    EXPECT_EQ(queue(b, {tc(12, 3, CC_FX_CUTOFF, 32.f)}), OLFX_OK);
    EXPECT_EQ(launch(a, 64), 8u);                            /* the topology ends the launch */
    EXPECT_EQ(param(a, 3, topo), 0.f);
    EXPECT_EQ(param(a, 3, cutoff), before);
    EXPECT_EQ(launch(a, 56), 56u);
    EXPECT_TRUE(param(a, 3, cutoff) != before);
    EXPECT_EQ(launch(b, 64), 64u);
    EXPECT_EQ(param(b, 3, cutoff), before);
    /* ... and the other way round: at topology 0 the voice-filter CC 41 stops short of the rack */
    Shadow c = fresh(OLFX_KIND_SYNTH_SVF, 8);
    const float zero = 0.f;
    EXPECT_EQ(c.set_range(3, 1, topo, 1, &zero), OLFX_OK);
    EXPECT_EQ(queue(c, {tc(12, 3, CC_CUTOFF, 32.f)}), OLFX_OK);
    EXPECT_EQ(launch(c, 64), 64u);
    EXPECT_EQ(param(c, 3, cutoff), before);
    EXPECT_TRUE(param(c, 3, OLFX_SY_VOICE0 + OLFX_VC_FILTER_CUTOFF) != param(b, 3, OLFX_SY_VOICE0 + OLFX_VC_FILTER_CUTOFF));

    /* a kit: the channel control pending across olfx_drumkit_map follows the new table */
    Shadow k = fresh(OLFX_KIND_DRUMKIT, 8);
    const olfx_drumkit_voice first[] = {{2, 1, 3, 40, 0}, {2, 2, OLFX_DK_NO_CHANNEL, 41, 0}};
    EXPECT_EQ(k.drumkit_map(first, 2), OLFX_OK);
    EXPECT_EQ(queue(k, {tc(8, 2, CC_CUTOFF, 32.f, 3)}), OLFX_OK);
    const olfx_drumkit_voice second[] = {{2, 2, 3, OLFX_DK_NO_NOTE, 0}};
    EXPECT_EQ(k.drumkit_map(second, 1), OLFX_OK);
    const float v1 = param(k, 2, OLFX_DK_VOICE0 + 16 * 1 + OLFX_VC_FILTER_CUTOFF), v2 = param(k, 2, OLFX_DK_VOICE0 + 16 * 2 + OLFX_VC_FILTER_CUTOFF);
    host::PacketPlan pl;
    EXPECT_EQ(launch(k, 64, &pl), 64u);
    EXPECT_EQ(param(k, 2, OLFX_DK_VOICE0 + 16 * 1 + OLFX_VC_FILTER_CUTOFF), v1);
    EXPECT_TRUE(param(k, 2, OLFX_DK_VOICE0 + 16 * 2 + OLFX_VC_FILTER_CUTOFF) != v2);
    EXPECT_EQ(k.configured[2 * k.n + 2], 1);
    EXPECT_EQ(k.configured[1 * k.n + 2], 0);
    EXPECT_EQ(pl.n_iv, (size_t)1);                           /* that voice slot alone, and no rack record */
    EXPECT_EQ(pl.n_if, (size_t)0);
    /* a channel nobody sits at, and an update-only control on a never-configured voice */
    Shadow u = fresh(OLFX_KIND_DRUMKIT, 8);
    EXPECT_EQ(u.drumkit_map(first, 2), OLFX_OK);
    EXPECT_EQ(queue(u, {tc(8, 2, CC_CUTOFF, 32.f, 9), tc(12, 2, CC_OSC_1_VOLUME, 32.f, 3)}), OLFX_OK);
    EXPECT_EQ(launch(u, 64, &pl), 64u);
    EXPECT_EQ(pl.n_seg, (size_t)3);
    EXPECT_EQ(pl.n_iv, (size_t)1);
    EXPECT_EQ(u.configured[1 * u.n + 2], 1);
    EXPECT_EQ(u.vrec.first.size(), (size_t)4);
}

TEST(TimedInstrumentParams, CarryOverAndFrameZeroFirst) {
    for (const int kind : kInstrumentKinds) {
        Shadow s = fresh(kind, 8);
        const uint32_t f = s.kd->voice0 + OLFX_VC_FILTER_CUTOFF;
        EXPECT_EQ(queue(s, {tp(64, 1, f, 111.f), tp(100, 2, f, 222.f), tp(132, 3, f, 333.f)}), OLFX_OK);
        const float before = param(s, 1, f);
        EXPECT_EQ(s.span(64), 64u);
        EXPECT_TRUE(!s.has_events(64));
        EXPECT_EQ(launch(s, 64), 64u);
        /* the record at frame 64 reached frame 0 as the call returned: applied, dirty, no longer pending */
        EXPECT_TRUE(before != 111.f);
        EXPECT_EQ(param(s, 1, f), 111.f);
        EXPECT_EQ(s.iparams.size(), (size_t)2);
        EXPECT_EQ(s.kit() ? s.vdirty_list.size() : s.dirty_list.size(), (size_t)1);
        /* a set_param made now lands behind it */
        const float later = 999.f;
        EXPECT_EQ(s.set_range(1, 1, f, 1, &later), OLFX_OK);
        EXPECT_EQ(param(s, 1, f), 999.f);
        EXPECT_EQ(s.iparams[0].frame, 36u);
        EXPECT_TRUE(param(s, 2, f) != 222.f);
        EXPECT_EQ(launch(s, 64), 64u);                       /* frame 36 of this call */
        EXPECT_EQ(param(s, 2, f), 222.f);
        EXPECT_EQ(s.iparams[0].frame, 4u);
        EXPECT_EQ(launch(s, 64), 64u);
        EXPECT_EQ(param(s, 3, f), 333.f);
        EXPECT_TRUE(s.iparams.empty());
        /* reset drops pending records */
        EXPECT_EQ(queue(s, {tp(8, 1, f, 5.f)}), OLFX_OK);
        s.reset();
        EXPECT_TRUE(s.iparams.empty());
    }
}

TEST(TimedInstrumentParams, BoundaryFieldsEndTheLaunch) {
    const uint32_t boundary[] = {OLFX_FR_DELAY_TIME, OLFX_FR_DELAY_FEEDBACK, OLFX_FR_DELAY_BALANCE, OLFX_FR_DELAY_CUTOFF,
                                 OLFX_FR_DELAY_RESONANCE, OLFX_FR_TOPOLOGY};
    const uint32_t inside[] = {OLFX_FR_REVERB_BALANCE, OLFX_FR_FILTER_CUTOFF, OLFX_FR_FILTER_RESONANCE, OLFX_FR_FILTER_DRIVE,
                               OLFX_FR_FILTER_TYPE, OLFX_FR_MASTER_VOLUME};
    for (const int kind : kInstrumentKinds) {
        for (const uint32_t rf : boundary) {
            Shadow s = fresh(kind, 70);
            const float v = rf == OLFX_FR_TOPOLOGY ? 1.f : 0.25f;
            EXPECT_EQ(queue(s, {tp(20, 69, rack0_of(kind) + rf, v)}), OLFX_OK);
            EXPECT_EQ(s.span(64), 20u);
            EXPECT_EQ(launch(s, 64), 20u);
            EXPECT_EQ(param(s, 69, rack0_of(kind) + rf), v);  /* frame 0 of the next launch: applied, on the dirty list */
            EXPECT_EQ(s.dirty_list.size(), (size_t)1);
            EXPECT_EQ(s.span(44), 44u);
        }
        for (const uint32_t rf : inside) {
            Shadow s = fresh(kind, 70);
            EXPECT_EQ(queue(s, {tp(20, 69, rack0_of(kind) + rf, rf == OLFX_FR_FILTER_TYPE ? 2.f : 0.25f)}), OLFX_OK);
            EXPECT_EQ(s.span(64), 64u);
            host::PacketPlan pl;
            EXPECT_EQ(launch(s, 64, &pl), 64u);
            EXPECT_EQ(pl.n_if, (size_t)1);
            EXPECT_EQ(pl.n_iv, (size_t)0);
        }
        Shadow s = fresh(kind, 70);
        EXPECT_EQ(queue(s, {tp(20, 69, s.kd->voice0 + OLFX_VC_FILTER_RESONANCE, 0.25f)}), OLFX_OK);
        EXPECT_EQ(s.span(64), 64u);
        /* a control that can map to a delay field ends it as well; a kit's only when it goes to the rack */
        Shadow c = fresh(kind, 70);
        EXPECT_EQ(queue(c, {tc(20, 1, CC_DELAY_TIME, 64.f, kind == OLFX_KIND_DRUMKIT ? OLFX_DK_CHANNEL_RACK : 0)}), OLFX_OK);
        EXPECT_EQ(c.span(64), 20u);
        if (kind == OLFX_KIND_DRUMKIT) {
            Shadow d = fresh(kind, 70);
            EXPECT_EQ(queue(d, {tc(20, 1, CC_DELAY_TIME, 64.f, 3)}), OLFX_OK);
            EXPECT_EQ(d.span(64), 64u);
        }
    }
    /* two boundary times and a voice record between them: three launches */
    Shadow s = fresh(OLFX_KIND_SYNTH, 70);
    EXPECT_EQ(queue(s, {tp(20, 1, OLFX_SY_RACK0 + OLFX_FR_DELAY_TIME, 0.001f), tp(28, 1, OLFX_SY_VOICE0 + OLFX_VC_FILTER_CUTOFF, 300.f),
                        tp(36, 1, OLFX_SY_RACK0 + OLFX_FR_DELAY_TIME, 0.f)}), OLFX_OK);
    EXPECT_EQ(launch(s, 64), 20u);
    EXPECT_EQ(launch(s, 44), 16u);
    EXPECT_EQ(launch(s, 28), 28u);
    EXPECT_TRUE(s.iparams.empty());
}

TEST(TimedInstrumentParams, SixteenTimesInALaunch) {
    for (const int kind : kInstrumentKinds) {
        /* frame 0, seven note times and eight record times: 16; one more time, of either sort, ends the launch */
        for (int extra = 0; extra < 3; ++extra) {
            Shadow s = fresh(kind, 16);                      /* (ten records: under the record cap) */
            std::vector<olfx_timed_note> notes;
            std::vector<olfx_timed_param> recs;
            for (uint32_t k = 1; k <= 7; ++k) notes.push_back(tn(8 * k, 0, ON));
            for (uint32_t k = 1; k <= 8; ++k) recs.push_back(tp(8 * k - 4, 1, s.kd->voice0 + OLFX_VC_FILTER_CUTOFF, 100.f * (float)k));
            recs.push_back(tp(56, 2, s.kd->voice0 + OLFX_VC_FILTER_CUTOFF, 50.f));       /* a time both share */
            if (extra == 1) notes.push_back(tn(64, 0, ON));
            if (extra == 2) recs.push_back(tp(64, 1, s.kd->voice0 + OLFX_VC_FILTER_CUTOFF, 1.f));
            EXPECT_EQ(queue(s, notes), OLFX_OK);
            EXPECT_EQ(queue(s, recs), OLFX_OK);
            EXPECT_EQ(s.span(128), extra ? 64u : 128u);
            host::PacketPlan pl;
            EXPECT_EQ(launch(s, 128, &pl), extra ? 64u : 128u);
            EXPECT_EQ(pl.n_seg, (size_t)kSegCap);
            EXPECT_EQ(pl.n_iv, (size_t)9);
        }
    }
}

TEST(TimedInstrumentParams, RecordCapOnBothSides) {
    for (const int kind : kInstrumentKinds) {
        const uint32_t n = 8, voices = 4, cap = host::timed_instrument_cap(kind, n, voices);
        EXPECT_EQ(cap, kind == OLFX_KIND_DRUMKIT ? n * voices : n);
        EXPECT_EQ(host::timed_instrument_cap(OLFX_KIND_VOICE, n, voices), 0u);
        for (const uint32_t over : {0u, 1u}) {
            Shadow s = fresh(kind, n, voices);
            std::vector<olfx_timed_param> r;
            for (uint32_t k = 0; k < cap - 1; ++k) r.push_back(tp(8, k % n, s.kd->voice0 + OLFX_VC_FILTER_CUTOFF, 100.f + (float)k));
            for (uint32_t k = 0; k < 1 + over; ++k) r.push_back(tp(24, k, rack0_of(kind) + OLFX_FR_FILTER_CUTOFF, 900.f));
            EXPECT_EQ(queue(s, r), OLFX_OK);
            EXPECT_EQ(s.span(64), over ? 24u : 64u);
        }
        /* one time alone always fits, however many records name its lanes */
        Shadow s = fresh(kind, n, voices);
        std::vector<olfx_timed_param> r;
        for (uint32_t k = 0; k < 3 * cap; ++k) r.push_back(tp(8, k % n, s.kd->voice0 + OLFX_VC_FILTER_CUTOFF, 100.f + (float)k));
        r.push_back(tp(12, 0, s.kd->voice0 + OLFX_VC_FILTER_CUTOFF, 1.f));
        EXPECT_EQ(queue(s, r), OLFX_OK);
        EXPECT_EQ(s.span(64), 12u);
        host::PacketPlan pl;
        EXPECT_EQ(launch(s, 64, &pl), 12u);
        EXPECT_EQ(pl.n_iv, (size_t)n);
        EXPECT_TRUE(pl.words <= host::max_packet_words(kind, n, s.n_ev(), kSegCap) + host::max_timed_instrument_words(kind, n, voices));
        EXPECT_EQ(s.span(52), 52u);
    }
}

TEST(TimedInstrumentParams, RefusedCallsChangeNothing) {
    for (const int kind : kInstrumentKinds) {
        Shadow s = fresh(kind, 70);
        EXPECT_EQ(queue(s, {tp(8, 1, s.kd->voice0 + OLFX_VC_FILTER_CUTOFF, 100.f)}), OLFX_OK);
        const Snapshot snap(s);
        const uint32_t f = s.kd->voice0 + OLFX_VC_FILTER_CUTOFF, topo = rack0_of(kind) + OLFX_FR_TOPOLOGY;
        const olfx_timed_param good = tp(0, 2, f, 700.f);     /* a good frame-0 record ahead of each bad one */
        const olfx_timed_param bad[] = {tp(6, 0, f, 1.f), tp(0x80000000u, 0, f, 1.f), tp(8, 70, f, 1.f), tp(8, 0, s.n_params, 1.f),
                                        tp(8, 0, f, NAN), tp(8, 0, f, INFINITY), tp(8, 0, topo, 2.f), tp(8, 0, topo, 0.5f),
                                        tp(8, 0, topo, kind == OLFX_KIND_SYNTH ? 0.f : 5.f)};
        for (const olfx_timed_param &b : bad) {
            EXPECT_EQ(queue(s, {good, b}), OLFX_E_ARG);
            EXPECT_TRUE(snap.same(s));
        }
        EXPECT_EQ(s.timed_instrument_params(nullptr, 1), OLFX_E_ARG);
        EXPECT_EQ(s.timed_instrument_params(nullptr, 0), OLFX_OK);
        const uint16_t rack = kind == OLFX_KIND_DRUMKIT ? OLFX_DK_CHANNEL_RACK : 0;
        const TimedControl cgood = tc(0, 2, CC_CUTOFF, 64.f, rack);
        const TimedControl cbad[] = {tc(6, 0, CC_CUTOFF, 64.f, rack), tc(0x80000000u, 0, CC_CUTOFF, 64.f, rack), tc(8, 70, CC_CUTOFF, 64.f, rack),
                                     tc(8, 0, CC_CUTOFF, 64.f, rack, 2), tc(8, 0, CC_CUTOFF, NAN, rack), tc(8, 0, CC_CUTOFF, 64.f, 3, 2)};
        for (const TimedControl &b : cbad) {
            /* (a kit's rack takes CC 41 at topology 1 only; the last record goes to a kit's channel: a bad source) */
            if (kind != OLFX_KIND_DRUMKIT && &b == &cbad[5]) continue;
            EXPECT_EQ(queue(s, {cgood, b}), OLFX_E_ARG);
            EXPECT_TRUE(snap.same(s));
        }
        EXPECT_EQ(s.timed_instrument_control(nullptr, 1), OLFX_E_ARG);
        EXPECT_TRUE(snap.same(s));
        /* the good records alone are taken: frame 0 is set_param / control now */
        EXPECT_EQ(queue(s, {good}), OLFX_OK);
        EXPECT_EQ(param(s, 2, f), 700.f);
        EXPECT_EQ(s.iparams.size(), (size_t)1);
    }
    const olfx_timed_param r = tp(8, 0, 0, 1.f);
    const TimedControl c = tc(8, 0, CC_CUTOFF, 64.f);
    for (const int kind : {OLFX_KIND_VOICE, OLFX_KIND_VOICE_MOOG, OLFX_KIND_VOICE_SAMPLE}) {
        Shadow s = fresh(kind, 8);
        EXPECT_EQ(s.timed_instrument_params(&r, 1), OLFX_E_KIND);
        EXPECT_EQ(s.timed_instrument_control(&c, 1), OLFX_E_KIND);
        EXPECT_TRUE(s.iparams.empty() && s.tparams.empty());
        EXPECT_EQ(host::max_timed_instrument_words(kind, 8, 4), (size_t)0);
    }
    for (const int kind : {OLFX_KIND_DATTORRO, OLFX_KIND_CHORUS, OLFX_KIND_PITCHSHIFT, OLFX_KIND_CHAIN, OLFX_KIND_FXRACK,
                           OLFX_KIND_PLATERACK, OLFX_KIND_METER, OLFX_KIND_METER_MONO}) {
        Shadow s = fresh(kind, 8);
        EXPECT_EQ(s.timed_instrument_params(&r, 1), OLFX_E_STATE);
        EXPECT_EQ(s.timed_instrument_control(&c, 1), OLFX_E_STATE);
        EXPECT_TRUE(s.iparams.empty());
        EXPECT_EQ(host::max_timed_instrument_words(kind, 8, 4), (size_t)0);
    }
    /* the voice kinds' calls still refuse the instruments, and their sizing is theirs */
    for (const int kind : kInstrumentKinds) {
        Shadow s = fresh(kind, 8);
        EXPECT_EQ(s.timed_params(&r, 1), OLFX_E_KIND);
        EXPECT_EQ(host::max_timed_param_words(kind, 8), (size_t)0);
        EXPECT_TRUE(host::max_timed_instrument_words(kind, 8, 4) > 0);
    }
}

TEST(TimedInstrumentParams, SectionOffsetsTablesAndRecordsBySize) {
    const auto up4 = [](size_t w) { return (w + 3) & ~(size_t)3; };
    for (const int kind : kInstrumentKinds)
        for (const uint32_t n : {1u, 65u, 130u, 8230u}) {
            const uint32_t voices = 5;
            Shadow s = fresh(kind, n, voices);
            const bool kit = kind == OLFX_KIND_DRUMKIT;
            /* frame 8: a voice field of every third instrument (a kit: slot i % 5); frame 12: a note only; frame 24: a
               rack field of the highest instruments and, past 40 instruments, CC 41 on instrument 0 (a synth: voice and
               rack).  n = 1: a launch takes one record, so everything sits at frame 24 (one time always fits) */
            std::vector<olfx_timed_param> r;
            std::vector<uint32_t> lanes;
            for (uint32_t i = 0; i < n; i += 3) lanes.push_back(kit ? (i % voices) * s.npad + i : i);
            std::sort(lanes.begin(), lanes.end());
            for (uint32_t i = 0; i < n; i += 3)
                r.push_back(tp(n == 1 ? 24 : 8, i, s.kd->voice0 + (kit ? 16 * (i % voices) : 0) + OLFX_VC_FILTER_CUTOFF, 50.f + (float)i));
            for (uint32_t i = n; i-- > n - std::min(n, 40u);) r.push_back(tp(24, i, rack0_of(kind) + OLFX_FR_REVERB_BALANCE, 0.5f));
            EXPECT_EQ(queue(s, r), OLFX_OK);
            EXPECT_EQ(queue(s, {tn(12, 0, ON)}), OLFX_OK);
            if (n > 40) EXPECT_EQ(queue(s, {tc(24, 0, CC_CUTOFF, 64.f, kit ? OLFX_DK_CHANNEL_RACK : 0)}), OLFX_OK);
            EXPECT_EQ(s.span(64), 64u);
            host::PacketPlan pl;
            const std::vector<uint32_t> buf = packet(s, 64, &pl);
            const size_t G = (n + 63) / 64, gv = kit ? voices * G : G, nseg = n == 1 ? 3 : 4;
            EXPECT_EQ(pl.n_seg, nseg);
            EXPECT_EQ(pl.n_tc, (size_t)0);
            EXPECT_EQ(pl.gv, gv);
            EXPECT_EQ(pl.gf, G);
            EXPECT_EQ(pl.n_iv, s.vrec.lane.size());
            EXPECT_EQ(pl.n_if, s.frec.lane.size());
            EXPECT_EQ(pl.n_iv, (size_t)((n + 2) / 3) + (!kit && n > 40 ? 1u : 0u));
            EXPECT_EQ(pl.n_if, (size_t)std::min(n, 40u) + (n > 40 ? 1u : 0u));
            EXPECT_EQ(pl.o_ivt, up4(pl.o_seg + ((nseg + 1) & ~(size_t)1)));
            EXPECT_EQ(pl.o_ift, pl.o_ivt + 4 * nseg * gv);
            EXPECT_EQ(pl.o_iv, pl.o_ift + 4 * nseg * G);
            EXPECT_EQ(pl.o_if, up4(pl.o_iv + VCC_N * pl.n_iv));
            EXPECT_EQ(pl.words, pl.o_if + TIF_N * pl.n_if);
            EXPECT_TRUE(pl.words <= host::max_packet_words(kind, n, s.n_ev(), kSegCap) + host::max_timed_instrument_words(kind, n, voices));
            /* every record where the kernel looks for it: base + the rank among the mask's lower bits */
            auto check = [&](size_t o_tab, size_t groups, const std::vector<uint32_t> &lane, const std::vector<uint32_t> &first,
                             size_t o_rec, uint32_t W, const std::vector<uint32_t> &words) {
                const size_t T = lane.size();
                size_t seen = 0;
                for (size_t sgm = 0; sgm < nseg; ++sgm)
                    for (size_t g = 0; g < groups; ++g) {
                        const uint32_t *e = buf.data() + o_tab + 4 * (sgm * groups + g);
                        const uint64_t mask = (uint64_t)e[0] | (uint64_t)e[1] << 32;
                        EXPECT_EQ(e[3], 0u);
                        for (uint32_t b = 0; b < 64; ++b) {
                            if (!(mask >> b & 1)) continue;
                            const size_t rec = e[2] + (size_t)__builtin_popcountll(mask & ((1ull << b) - 1));
                            EXPECT_TRUE(rec < T && rec >= first[sgm] && rec < first[sgm + 1]);
                            if (rec >= T) continue;
                            EXPECT_EQ((size_t)lane[rec], g * 64 + b);
                            for (uint32_t w = 0; w < W; ++w) EXPECT_EQ(buf[o_rec + (size_t)w * T + rec], words[rec * W + w]);
                            ++seen;
                        }
                    }
                EXPECT_EQ(seen, T);
            };
            check(pl.o_ivt, gv, s.vrec.lane, s.vrec.first, pl.o_iv, VCC_N, s.vrec.words);
            check(pl.o_ift, G, s.frec.lane, s.frec.first, pl.o_if, TIF_N, s.frec.words);
            /* the lanes: a synth's instrument, a kit's device voice slot p npad + kit; the records as the shadow has them */
            EXPECT_TRUE(std::equal(lanes.begin(), lanes.end(), s.vrec.lane.begin()));
            const std::vector<uint32_t> w0 = rack_record(s, n - 1);
            for (uint32_t w = 0; w < TIF_N; ++w) EXPECT_EQ(s.frec.words[(s.frec.lane.size() - 1) * TIF_N + w], w0[w]);
        }
}

TEST(TimedInstrumentParams, NoRecordNoChange) {
    /* timed notes alone, a record at frame 0 and one past the span: the packet is the untouched path's, word for word
       (the same shadow driven by set_param and timed notes only), and none of the new state is touched */
    for (const int kind : kInstrumentKinds) {
        Shadow a = fresh(kind, 130), b = fresh(kind, 130);
        if (kind == OLFX_KIND_DRUMKIT) {
            const olfx_drumkit_voice m[] = {{3, 0, 0, 60, 0}, {70, 1, 1, 62, 0}, {129, 0, 0, 60, 0}, {5, 2, 2, 60, 0}};
            EXPECT_EQ(a.drumkit_map(m, 4), OLFX_OK);
            EXPECT_EQ(b.drumkit_map(m, 4), OLFX_OK);
        }
        const std::vector<olfx_timed_note> evs = {tn(8, 3, ON), tn(8, 70, ON, 62), tn(24, 129, OLFX_EV_NOTE_OFF), tn(0, 5, ON)};
        EXPECT_EQ(queue(a, evs), OLFX_OK);
        EXPECT_EQ(queue(b, evs), OLFX_OK);
        const uint32_t f = a.kd->voice0 + OLFX_VC_FILTER_CUTOFF;
        EXPECT_EQ(queue(a, {tp(0, 9, f, 700.f), tp(64, 9, f, 800.f)}), OLFX_OK);
        const float v = 700.f;
        EXPECT_EQ(b.set_range(9, 1, f, 1, &v), OLFX_OK);
        EXPECT_EQ(a.span(64), b.span(64));
        host::PacketPlan pa, pb;
        const std::vector<uint32_t> wa = packet(a, 64, &pa), wb = packet(b, 64, &pb);
        EXPECT_EQ(pa.n_iv + pa.n_if, (size_t)0);
        EXPECT_EQ(pa.o_ivt, (size_t)0);
        EXPECT_EQ(pa.n_seg, (size_t)3);
        EXPECT_EQ(pa.words, pb.words);
        EXPECT_TRUE(wa == wb);
        EXPECT_TRUE(a.dirty_list.empty() && a.vdirty_list.empty());
        EXPECT_TRUE(a.kept_inst.words.empty() && a.kept_slot.words.empty() && a.changed_inst.empty() && a.changed_slot.empty() && !a.fold_fresh);
        /* ... and with nothing but the frame-0 write, the unsegmented packet */
        Shadow c = fresh(kind, 130), d = fresh(kind, 130);
        EXPECT_EQ(queue(c, {tp(0, 9, f, 700.f), tp(64, 9, f, 800.f)}), OLFX_OK);
        EXPECT_EQ(d.set_range(9, 1, f, 1, &v), OLFX_OK);
        EXPECT_TRUE(!c.has_events(64));
        const std::vector<uint32_t> wc = packet(c, 64, &pa), wd = packet(d, 64, &pb);
        EXPECT_EQ(pa.n_seg, (size_t)1);
        EXPECT_TRUE(wc == wd);
    }
}

TEST(TimedInstrumentParams, FrameZeroRecordsAndKeptRecords) {
    /* an instrument dirty at frame 0 and changed again at frame 8: the packet's own record is frame 0's, the timed record
       is frame 8's, and the next packet delivers frame 8's again without a second derivation (the kept record) */
    for (const int kind : kInstrumentKinds) {
        Shadow s = fresh(kind, 70), twin = fresh(kind, 70);
        const bool kit = kind == OLFX_KIND_DRUMKIT;
        const uint32_t f = s.kd->voice0 + (kit ? 16 * 2 : 0) + OLFX_VC_FILTER_CUTOFF, rb = rack0_of(kind) + OLFX_FR_REVERB_BALANCE;
        const float v0 = 300.f, r0 = 0.75f;
        for (Shadow *x : {&s, &twin}) {
            EXPECT_EQ(x->set_range(7, 1, f, 1, &v0), OLFX_OK);
            EXPECT_EQ(x->set_range(7, 1, rb, 1, &r0), OLFX_OK);
        }
        EXPECT_EQ(queue(s, {tp(8, 7, f, 4000.f), tp(8, 7, rb, 0.25f)}), OLFX_OK);
        host::PacketPlan pl, pt;
        std::vector<uint32_t> buf, tbuf;
        EXPECT_EQ(launch(s, 64, &pl, &buf), 64u);
        EXPECT_EQ(launch(twin, 64, &pt, &tbuf), 64u);
        /* the records ahead of the event section are the twin's, which never saw frame 8 */
        EXPECT_EQ(pl.o_ev, pt.o_ev);
        EXPECT_TRUE(std::equal(buf.begin(), buf.begin() + (ptrdiff_t)pl.o_ev, tbuf.begin()));
        EXPECT_EQ(pl.n_iv, (size_t)1);
        EXPECT_EQ(pl.n_if, (size_t)1);
        const std::vector<uint32_t> vw = voice_record(s, 7, kit ? 2 : 0), fw = rack_record(s, 7);
        for (uint32_t w = 0; w < VCC_N; ++w) EXPECT_EQ(buf[pl.o_iv + w], vw[w]);
        for (uint32_t w = 0; w < TIF_N; ++w) EXPECT_EQ(buf[pl.o_if + w], fw[w]);
        /* back on the lists with the last record kept; the next packet is what set_param of frame 8's values gives */
        EXPECT_EQ(s.dirty_list.size(), (size_t)1);
        EXPECT_EQ(s.vdirty_list.size(), (size_t)(kit ? 1 : 0));
        EXPECT_TRUE(!s.kept_inst.words.empty() && s.kept_inst.of[7] == 0);
        if (kit) EXPECT_TRUE(!s.kept_slot.words.empty() && s.kept_slot.of[2 * s.n + 7] == 0);
        const float v8 = 4000.f, r8 = 0.25f;
        EXPECT_EQ(twin.set_range(7, 1, f, 1, &v8), OLFX_OK);
        EXPECT_EQ(twin.set_range(7, 1, rb, 1, &r8), OLFX_OK);
        EXPECT_EQ(launch(s, 64, &pl, &buf), 64u);
        EXPECT_EQ(launch(twin, 64, &pt, &tbuf), 64u);
        EXPECT_TRUE(buf == tbuf);
        EXPECT_TRUE(s.kept_inst.words.empty() && s.kept_slot.words.empty() && s.dirty_list.empty() && s.vdirty_list.empty());
        /* a write after the launch forgets the kept record */
        EXPECT_EQ(queue(s, {tp(8, 7, f, 5000.f)}), OLFX_OK);
        EXPECT_EQ(launch(s, 64), 64u);
        const float v9 = 6000.f;
        EXPECT_EQ(s.set_range(7, 1, f, 1, &v9), OLFX_OK);
        EXPECT_EQ(twin.set_range(7, 1, f, 1, &v9), OLFX_OK);
        EXPECT_EQ(launch(s, 64, &pl, &buf), 64u);
        EXPECT_EQ(launch(twin, 64, &pt, &tbuf), 64u);
        EXPECT_TRUE(buf == tbuf);
    }
}

TEST(TimedInstrumentParams, ReadsAsOfTheFramesProcessed) {
    Shadow s = fresh(OLFX_KIND_SYNTH_SVF, 8);
    const uint32_t f = OLFX_SY_VOICE0 + OLFX_VC_FILTER_RESONANCE, m = OLFX_SY_RACK0 + OLFX_FR_MASTER_VOLUME;
    const float f0 = param(s, 4, f), m0 = param(s, 4, m);
    EXPECT_EQ(queue(s, {tp(20, 4, f, 0.5f), tp(68, 4, m, 0.25f)}), OLFX_OK);
    EXPECT_EQ(queue(s, {tc(100, 4, CC_VOLUME, 127.f)}), OLFX_OK);
    EXPECT_EQ(param(s, 4, f), f0);                           /* nothing processed yet */
    EXPECT_EQ(launch(s, 16), 16u);
    EXPECT_EQ(param(s, 4, f), f0);
    EXPECT_EQ(launch(s, 16), 16u);                           /* frames 16 .. 31 hold frame 20 */
    EXPECT_EQ(param(s, 4, f), 0.5f);
    EXPECT_EQ(param(s, 4, m), m0);
    EXPECT_EQ(launch(s, 64), 64u);
    EXPECT_EQ(param(s, 4, m), 0.25f);
    /* CC 7 at topology 1 reaches the voices' amp_env_amount alone */
    const float amp = param(s, 4, OLFX_SY_VOICE0 + OLFX_VC_AMP_ENV_AMOUNT);
    EXPECT_EQ(launch(s, 64), 64u);
    EXPECT_TRUE(param(s, 4, OLFX_SY_VOICE0 + OLFX_VC_AMP_ENV_AMOUNT) != amp);
    EXPECT_EQ(param(s, 4, m), 0.25f);
    EXPECT_TRUE(s.iparams.empty());
}

int main() { return run_all_tests(); }
