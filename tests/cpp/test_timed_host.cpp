/*
 * tests/cpp/test_timed_host.cpp -- olfx_timed_events in the engine's HIP-free host core
 * (ol_dsp_amd/csrc/olfx_host.h) on the CPU: the pending list's order and its segments, each segment's fold
 * against the fold of a split queue, the carry-over arithmetic, validation (a refused call changes
 * nothing), the refusals per kind, a frame-0-only queue's packet against today's, the worst packet
 * against max_packet_words and its offsets at n = 1, 64, 65 and 8230, the span at exactly 16, 17, 32 and 33
 * times, an event at frame == span, and the chunk count of ragged spans.  Links olfx_host.cpp directly (no libolfx.so, no GPU); built by
 * tests/test_timed_host.py with its own build line.
 */
#include "../../ol_dsp_amd/csrc/olfx_host.h"
#include "harness.h"

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

olfx_voice_event vev(uint32_t inst, uint8_t type, uint8_t note = 60, float value = 0.f) {
    return olfx_voice_event{inst, type, note, 100, 0, value};
}
olfx_timed_event tev(uint32_t frame, uint32_t inst, uint8_t type, uint8_t note = 60, float value = 0.f) {
    return olfx_timed_event{frame, vev(inst, type, note, value)};
}
int queue(Shadow &s, const std::vector<olfx_timed_event> &e) { return s.timed_events(e.data(), (uint32_t)e.size()); }

/* the event section of the next launch of `span` frames, as the engine writes it; *pl: its plan */
std::vector<uint32_t> section(Shadow &s, uint32_t span, host::PacketPlan *plan = nullptr) {
    s.fold_segments(span);
    const host::PacketPlan pl = s.plan(true);
    std::vector<uint32_t> buf(pl.words + 4, 0xDEADBEEFu);
    s.fill_records(pl, buf.data());
    s.write_events(buf.data() + pl.o_ev);
    for (size_t k = pl.words; k < buf.size(); ++k) EXPECT_EQ(buf[k], 0xDEADBEEFu);       /* nothing past the plan */
    if (plan) *plan = pl;
    return std::vector<uint32_t>(buf.begin() + (ptrdiff_t)pl.o_ev, buf.begin() + (ptrdiff_t)pl.words);
}

/* the records of one segment's groups, overflow runs followed, as (voice, op, freq) in slot order */
struct Rec { uint32_t inst, op, freq; bool operator==(const Rec &o) const { return inst == o.inst && op == o.op && freq == o.freq; } };
std::vector<Rec> decode(const uint32_t *fix, const uint32_t *more, uint32_t n) {
    std::vector<Rec> out;
    for (uint32_t g = 0; g < (n + 63) / 64; ++g) {
        const uint32_t *slot = fix + 2 * (size_t)g * kVevCap;
        if ((slot[0] >> 8) & VEV_MORE) {
            for (uint32_t k = 0; k < slot[0] >> 16; ++k) {
                const uint32_t *r = more + 2 * ((size_t)slot[1] + k);
                out.push_back(Rec{g * 64 + (r[0] & 63u), r[0] >> 8, r[1]});
            }
        } else {
            for (uint32_t k = 0; k < kVevCap; ++k)
                if (slot[2 * k] >> 8) out.push_back(Rec{g * 64 + (slot[2 * k] & 63u), slot[2 * k] >> 8, slot[2 * k + 1]});
        }
    }
    return out;
}

constexpr uint8_t ON = OLFX_EV_NOTE_ON, OFF = OLFX_EV_NOTE_OFF, GON = OLFX_EV_GATE_ON, SETF = OLFX_EV_SET_FREQUENCY;

}  // namespace

TEST(Timed, StableOrderAndSegments) {
    Shadow s = fresh(OLFX_KIND_VOICE, 130);
    /* three calls, frames out of order, ties across calls; frame 0 joins the untimed queue in arrival order */
    EXPECT_EQ(queue(s, {tev(16, 1, ON, 61), tev(8, 2, ON, 62), tev(16, 3, ON, 63)}), OLFX_OK);
    const olfx_voice_event u = vev(9, ON, 70);
    EXPECT_EQ(s.voice_events(&u, 1), OLFX_OK);
    EXPECT_EQ(queue(s, {tev(8, 4, ON, 64), tev(0, 9, OFF), tev(16, 1, OFF), tev(72, 5, ON)}), OLFX_OK);
    EXPECT_EQ(queue(s, {tev(8, 2, SETF, 0, 100.f)}), OLFX_OK);
    EXPECT_EQ(s.events.size(), (size_t)2);
    EXPECT_EQ(s.events[0].type, ON);
    EXPECT_EQ(s.events[1].type, OFF);
    const uint32_t want_frame[] = {8, 8, 8, 16, 16, 16, 72}, want_inst[] = {2, 4, 2, 1, 3, 1, 5};
    EXPECT_EQ(s.timed.size(), (size_t)7);
    for (size_t k = 0; k < s.timed.size() && k < 7; ++k) {
        EXPECT_EQ(s.timed[k].frame, want_frame[k]);
        EXPECT_EQ(s.timed[k].ev.inst, want_inst[k]);
    }
    EXPECT_EQ(s.span(64), 64u);
    EXPECT_TRUE(s.has_events(64));
    s.fold_segments(64);
    EXPECT_EQ(s.n_seg(), 3u);
    EXPECT_EQ(s.seg_frame[0], 0u);
    EXPECT_EQ(s.seg_frame[1], 8u);
    EXPECT_EQ(s.seg_frame[2], 16u);
    EXPECT_EQ(s.n_chunks(64, 8), 1u + 1u + 6u);
    /* segment 0: NoteOn then NoteOff on voice 9; segment 1: voice 2 (NoteOn, then SetFrequency wins the pitch) and 4;
       segment 2: voice 1 (NoteOn, NoteOff) and 3 -- by first appearance */
    EXPECT_EQ(s.seg_first.size(), (size_t)4);
    EXPECT_EQ(s.folded.size(), (size_t)5);
    EXPECT_EQ(s.folded[0].inst, 9u);
    EXPECT_EQ(s.folded[0].op, (uint32_t)(VEV_GATE_SET | VEV_RETRIGGER | VEV_FREQ));
    EXPECT_EQ(s.folded[1].inst, 2u);
    const float hz = 100.f;
    uint32_t hzb;
    std::memcpy(&hzb, &hz, 4);
    EXPECT_EQ(s.folded[1].freq, hzb);
    EXPECT_EQ(s.folded[2].inst, 4u);
    EXPECT_EQ(s.folded[3].inst, 1u);
    EXPECT_EQ(s.folded[3].op, (uint32_t)(VEV_GATE_SET | VEV_RETRIGGER | VEV_FREQ));
    EXPECT_EQ(s.folded[4].inst, 3u);
    /* the event at 72 stays, counted from the next block */
    EXPECT_EQ(s.timed.size(), (size_t)1);
    s.advance(64);
    EXPECT_EQ(s.timed[0].frame, 8u);
    EXPECT_TRUE(!s.has_events(8) && s.has_events(12));
}

TEST(Timed, SegmentFoldsEqualSplitQueues) {
    /* group 0 crowded in two segments (two overflow runs), group 1 with exactly kVevCap, a voice with three events
       at one frame, an empty segment 0; sample voices, so the seek bit is in it */
    const uint32_t n = 130;
    for (const int kind : {OLFX_KIND_VOICE, OLFX_KIND_VOICE_MOOG, OLFX_KIND_VOICE_SAMPLE}) {
        std::vector<olfx_timed_event> evs;
        for (uint32_t i = 0; i < 9; ++i) evs.push_back(tev(20, i * 7, ON, (uint8_t)(40 + i)));
        for (uint32_t i = 0; i < 4; ++i) evs.push_back(tev(20, 64 + i * 9, GON));
        for (uint32_t i = 0; i < 6; ++i) evs.push_back(tev(4, 3 + i, i & 1 ? OFF : ON, (uint8_t)(50 + i)));
        evs.push_back(tev(4, 129, ON, 33));
        evs.push_back(tev(4, 129, OFF));
        evs.push_back(tev(4, 129, SETF, 0, 441.f));
        evs.push_back(tev(60, 128, SETF, 0, 99.f));
        Shadow s = fresh(kind, n);
        EXPECT_EQ(queue(s, evs), OLFX_OK);
        host::PacketPlan pl;
        const std::vector<uint32_t> sec = section(s, 64, &pl);
        const uint32_t frames[] = {0, 4, 20, 60};
        EXPECT_EQ(pl.n_seg, (size_t)4);
        const size_t groups = 3, fixw = 2 * groups * kVevCap;
        EXPECT_EQ(s.n_more, 6u + 9u);
        EXPECT_EQ(sec.size(), 4 * fixw + 2 * (size_t)s.n_more + 4);
        EXPECT_EQ(pl.o_seg, pl.o_ev + 4 * fixw + 2 * (size_t)s.n_more);
        const uint32_t *more = sec.data() + 4 * fixw;
        for (uint32_t k = 0; k < 4; ++k) {
            EXPECT_EQ(more[2 * s.n_more + k], frames[k]);
            /* the twin: that frame's events queued with olfx_voice_events, folded as a block's */
            Shadow t = fresh(kind, n);
            for (const olfx_timed_event &e : evs)
                if (e.frame == frames[k]) EXPECT_EQ(t.voice_events(&e.ev, 1), OLFX_OK);
            const bool any = !t.events.empty();
            t.fold_events();
            const host::PacketPlan tp = t.plan(true);
            std::vector<uint32_t> tb(tp.words);
            t.fill_records(tp, tb.data());
            t.write_events(tb.data() + tp.o_ev);
            const uint32_t *tfix = tb.data() + tp.o_ev;
            const std::vector<Rec> want = decode(tfix, tfix + fixw, n);
            const std::vector<Rec> got = decode(sec.data() + k * fixw, more, n);
            EXPECT_EQ(any, !want.empty());
            EXPECT_TRUE(got == want);
            /* a segment without a crowded group has the twin's fixed slots word for word */
            if (!t.n_more) EXPECT_TRUE(std::memcmp(sec.data() + k * fixw, tfix, fixw * 4) == 0);
        }
    }
}

TEST(Timed, CarryOverAcrossThreeCalls) {
    Shadow s = fresh(OLFX_KIND_VOICE_MOOG, 8);
    EXPECT_EQ(queue(s, {tev(64 + 8, 1, ON), tev(128, 2, ON), tev(64, 3, ON), tev(60, 4, ON), tev(128 + 64, 5, ON)}), OLFX_OK);
    /* call 1 of 64 frames: the event at 60 */
    EXPECT_EQ(s.span(64), 64u);
    s.fold_segments(64);
    EXPECT_EQ(s.n_seg(), 2u);
    EXPECT_EQ(s.seg_frame[1], 60u);
    EXPECT_EQ(s.folded.size(), (size_t)1);
    s.advance(64);
    /* frame == n_frames is frame 0 of call 2, ahead of anything queued after call 1 */
    EXPECT_EQ(s.events.size(), (size_t)1);
    EXPECT_EQ(s.events[0].inst, 3u);
    const olfx_voice_event u = vev(3, OFF);
    EXPECT_EQ(s.voice_events(&u, 1), OLFX_OK);
    EXPECT_EQ(s.timed.size(), (size_t)3);
    EXPECT_EQ(s.timed[0].frame, 8u);
    EXPECT_EQ(s.timed[1].frame, 64u);
    EXPECT_EQ(s.timed[2].frame, 128u);
    s.fold_segments(64);
    EXPECT_EQ(s.n_seg(), 2u);
    EXPECT_EQ(s.seg_frame[1], 8u);
    EXPECT_EQ(s.folded[0].inst, 3u);
    EXPECT_EQ(s.folded[0].op, (uint32_t)(VEV_GATE_SET | VEV_RETRIGGER | VEV_FREQ));      /* NoteOn, then NoteOff */
    EXPECT_EQ(s.folded[1].inst, 1u);
    s.advance(64);
    /* call 3, of 32 frames only: voice 2 at its frame 0; voice 5 stays at 64 - 32 */
    EXPECT_EQ(s.events.size(), (size_t)1);
    EXPECT_EQ(s.events[0].inst, 2u);
    s.fold_segments(32);
    EXPECT_EQ(s.n_seg(), 1u);
    s.advance(32);
    EXPECT_EQ(s.timed.size(), (size_t)1);
    EXPECT_EQ(s.timed[0].frame, 32u);
    EXPECT_TRUE(s.events.empty());
    /* reset drops the pending events with the queued ones */
    const olfx_voice_event v = vev(0, ON);
    EXPECT_EQ(s.voice_events(&v, 1), OLFX_OK);
    s.reset();
    EXPECT_TRUE(s.events.empty() && s.timed.empty());
}

TEST(Timed, BadRecordsLeaveTheQueueUntouched) {
    Shadow s = fresh(OLFX_KIND_VOICE, 10);
    EXPECT_EQ(queue(s, {tev(8, 1, ON), tev(0, 2, ON)}), OLFX_OK);
    const std::vector<olfx_timed_event> before = s.timed;
    const olfx_timed_event bad[] = {
        tev(6, 0, ON), tev(0x80000000u, 0, ON), tev(0xFFFFFFFCu, 0, ON), tev(8, 10, ON), tev(8, 0, ON, 128),
        tev(8, 0, 5), tev(8, 0, SETF, 0, INFINITY), tev(8, 0, SETF, 0, NAN)};
    for (const olfx_timed_event &b : bad) {
        EXPECT_EQ(queue(s, {tev(4, 5, ON), tev(0, 6, ON), b}), OLFX_E_ARG);
        EXPECT_TRUE(s.msg[0] != 0);
        EXPECT_EQ(s.timed.size(), before.size());
        EXPECT_TRUE(std::memcmp(s.timed.data(), before.data(), before.size() * sizeof(olfx_timed_event)) == 0);
        EXPECT_EQ(s.events.size(), (size_t)1);
    }
    EXPECT_EQ(s.timed_events(nullptr, 1), OLFX_E_ARG);
    EXPECT_EQ(s.timed_events(nullptr, 0), OLFX_OK);
    EXPECT_EQ(queue(s, {tev(0x7FFFFFFCu, 9, ON)}), OLFX_OK);              /* the last frame there is */
    EXPECT_EQ(s.timed.size(), (size_t)2);
}

TEST(Timed, RefusalsPerKind) {
    const olfx_timed_event e = tev(8, 0, ON);
    for (const int kind : {OLFX_KIND_VOICE, OLFX_KIND_VOICE_MOOG, OLFX_KIND_VOICE_SAMPLE}) {
        Shadow s = fresh(kind, 4);
        EXPECT_EQ(s.timed_events(&e, 1), OLFX_OK);
    }
    for (const int kind : {OLFX_KIND_SYNTH, OLFX_KIND_SYNTH_SVF, OLFX_KIND_DRUMKIT}) {
        Shadow s = fresh(kind, 4);
        EXPECT_EQ(s.timed_events(&e, 1), OLFX_E_KIND);
        EXPECT_TRUE(s.timed.empty() && s.events.empty());
        for (const uint8_t p : s.playing) EXPECT_EQ(p, 0);
    }
    for (const int kind : {OLFX_KIND_DATTORRO, OLFX_KIND_CHORUS, OLFX_KIND_PITCHSHIFT, OLFX_KIND_CHAIN, OLFX_KIND_FXRACK,
                           OLFX_KIND_PLATERACK, OLFX_KIND_METER, OLFX_KIND_METER_MONO}) {
        Shadow s = fresh(kind, 4);
        EXPECT_EQ(s.timed_events(&e, 1), OLFX_E_STATE);
        EXPECT_EQ(s.note_events(nullptr, 0), OLFX_E_STATE);
    }
}

TEST(Timed, FrameZeroOnlyIsTodaysPacket) {
    /* the same events through olfx_timed_events at frame 0 and through olfx_voice_events, coefficients dirty too:
       the whole packet, word for word, and one segment */
    for (const int kind : {OLFX_KIND_VOICE, OLFX_KIND_VOICE_MOOG, OLFX_KIND_VOICE_SAMPLE}) {
        Shadow a = fresh(kind, 130), b = fresh(kind, 130);
        std::vector<olfx_timed_event> evs;
        for (uint32_t i = 0; i < 130; i += 3) evs.push_back(tev(0, i, i % 2 ? GON : ON, (uint8_t)(30 + i % 60)));
        evs.push_back(tev(0, 6, SETF, 0, 123.f));
        evs.push_back(tev(256, 7, ON));                                    /* past the block: not in it */
        const float cut = 900.f;
        for (Shadow *s : {&a, &b}) EXPECT_EQ(s->set_range(5, 1, OLFX_VC_FILTER_CUTOFF, 1, &cut), OLFX_OK);
        EXPECT_EQ(queue(a, evs), OLFX_OK);
        for (const olfx_timed_event &e : evs)
            if (!e.frame) EXPECT_EQ(b.voice_events(&e.ev, 1), OLFX_OK);
        EXPECT_EQ(a.span(256), 256u);
        a.fold_segments(256);
        b.fold_events();
        EXPECT_EQ(a.n_seg(), 1u);
        const host::PacketPlan pa = a.plan(true), pb = b.plan(true);
        EXPECT_EQ(pa.words, pb.words);
        EXPECT_EQ(pa.o_ev, pb.o_ev);
        EXPECT_EQ(pa.n_seg, (size_t)1);
        EXPECT_EQ(pa.words, host::plan_packet(130, 1, a.kd->words, true, b.n_more).words);
        std::vector<uint32_t> wa(pa.words, 0xA5A5A5A5u), wb(pb.words, 0xA5A5A5A5u);   /* (alignment gaps are not written) */
        a.fill_records(pa, wa.data());
        b.fill_records(pb, wb.data());
        a.write_events(wa.data() + pa.o_ev);
        b.write_events(wb.data() + pb.o_ev);
        EXPECT_TRUE(wa == wb);
    }
}

TEST(Timed, SpanSplitsAtTheCap) {
    Shadow s = fresh(OLFX_KIND_VOICE, 130);
    std::vector<olfx_timed_event> evs;
    for (uint32_t f = 0; f < 256; f += 4) evs.push_back(tev(f, f % 130, ON));
    EXPECT_EQ(queue(s, evs), OLFX_OK);
    uint32_t f0 = 0, launches = 0, seen = 0;
    while (f0 < 256) {
        const uint32_t span = s.span(256 - f0);
        EXPECT_TRUE(span > 0 && span % 4 == 0);
        s.fold_segments(span);
        EXPECT_TRUE(s.n_seg() <= kSegCap);
        for (uint32_t k = 0; k < s.n_seg(); ++k) EXPECT_EQ(f0 + s.seg_frame[k], 4 * (seen + k));
        seen += s.n_seg();
        EXPECT_EQ(s.n_chunks(span, 8), s.n_seg());                        /* every segment one 4-frame chunk */
        s.advance(span);
        f0 += span;
        ++launches;
    }
    EXPECT_EQ(f0, 256u);
    EXPECT_EQ(seen, 64u);
    EXPECT_EQ(launches, 64u / kSegCap);
    EXPECT_TRUE(s.timed.empty() && s.events.empty());
    /* an empty segment 0 counts: 16 timed frames past 0 are 17 segments */
    for (uint32_t f = 4; f <= 64; f += 4) {
        const olfx_timed_event e = tev(f, 1, ON);
        EXPECT_EQ(s.timed_events(&e, 1), OLFX_OK);
    }
    EXPECT_EQ(s.span(128), 64u);
}

TEST(Timed, WorstPacketFitsTheMaximum) {
    /* every voice with an event in every segment up to the cap, every coefficient dirty, n = 130 */
    for (const int kind : {OLFX_KIND_VOICE, OLFX_KIND_VOICE_MOOG, OLFX_KIND_VOICE_SAMPLE}) {
        Shadow s;
        s.init(kind, 130, 48000.f);
        s.reset();                                                         /* all dirty */
        std::vector<olfx_timed_event> evs;
        for (uint32_t k = 0; k < kSegCap + 1; ++k)
            for (uint32_t i = 0; i < 130; ++i) evs.push_back(tev(4 * k, i, ON));
        EXPECT_EQ(queue(s, evs), OLFX_OK);
        const uint32_t span = s.span(256);
        EXPECT_EQ(span, 4 * kSegCap);
        host::PacketPlan pl;
        const std::vector<uint32_t> sec = section(s, span, &pl);
        EXPECT_EQ(pl.n_seg, (size_t)kSegCap);
        EXPECT_TRUE(pl.dense);
        EXPECT_EQ(s.n_more, kSegCap * 128u);                              /* the last group's two voices fit its slots */
        EXPECT_EQ(host::max_segments(kind), kSegCap);
        EXPECT_TRUE(pl.words <= host::max_packet_words(kind, 130, 0, host::max_segments(kind)));
        EXPECT_TRUE(pl.words > host::max_packet_words(kind, 130));         /* ... and not one segment's */
        /* the kinds that take no timed events keep one segment */
        EXPECT_EQ(host::max_segments(OLFX_KIND_SYNTH), 1u);
        EXPECT_EQ(host::max_segments(OLFX_KIND_DRUMKIT), 1u);
        EXPECT_EQ(host::max_segments(OLFX_KIND_FXRACK), 1u);
    }
}

TEST(Timed, WorstPacketOffsetsBySize) {
    /* every voice in each of kSegCap segments, every coefficient dirty, at n = 1 (one lane), 64 (one full group), 65
       (a group of one voice, which fits its fixed slots) and 8230 (128 full groups and 38 voices: a segment's
       records alone are past 64 KiB).  The section's offsets, restated: slots [kSegCap][groups][kVevCap], the
       overflow list, the start frames -- and the maximum is reached exactly where every group is crowded */
    const auto up4 = [](size_t w) { return (w + 3) & ~(size_t)3; };
    for (const int kind : {OLFX_KIND_VOICE, OLFX_KIND_VOICE_MOOG, OLFX_KIND_VOICE_SAMPLE})
        for (const uint32_t n : {1u, 64u, 65u, 8230u}) {
            Shadow s;
            s.init(kind, n, 48000.f);
            s.reset();                                                     /* all dirty */
            std::vector<olfx_timed_event> evs;
            for (uint32_t k = 0; k < kSegCap; ++k)
                for (uint32_t i = 0; i < n; ++i) evs.push_back(tev(4 * k, i, k & 1 ? OFF : ON, (uint8_t)(30 + (i + k) % 90)));
            EXPECT_EQ(queue(s, evs), OLFX_OK);
            EXPECT_EQ(s.span(64), 64u);
            host::PacketPlan pl;
            const std::vector<uint32_t> sec = section(s, 64, &pl);
            const size_t groups = (n + 63) / 64, W = s.kd->words, fixw = 2 * groups * kVevCap;
            const size_t tail = n % 64, crowded = (n / 64) * 64 + (tail > kVevCap ? tail : 0);
            EXPECT_TRUE(pl.dense);
            EXPECT_EQ(pl.n_seg, (size_t)kSegCap);
            EXPECT_EQ(pl.o_val, (size_t)0);
            EXPECT_EQ(pl.o_ev, up4(W * n));
            EXPECT_EQ((size_t)s.n_more, kSegCap * crowded);
            EXPECT_EQ(pl.o_seg, pl.o_ev + kSegCap * fixw + 2 * (size_t)s.n_more);
            EXPECT_EQ(pl.words, pl.o_seg + kSegCap);
            EXPECT_EQ(sec.size(), pl.words - pl.o_ev);
            const size_t most = host::max_packet_words(kind, n, 0, kSegCap);
            EXPECT_TRUE(pl.words <= most);
            /* the maximum's event part: 2 * segs * (groups * kVevCap + n) + segs words */
            const size_t ev_most = 2 * (size_t)kSegCap * (groups * kVevCap + n) + kSegCap;
            if (crowded == n) {
                EXPECT_EQ(sec.size(), ev_most);
                EXPECT_TRUE(most - pl.words <= n + 16);                    /* the absent instance list, the slack */
            } else {
                EXPECT_EQ(sec.size() + 2 * (size_t)kSegCap * (n - crowded), ev_most);
            }
            if (n == 8230) EXPECT_TRUE(8 * (size_t)n >= 65536);
            /* what was written there: the start frames, and every segment's records in voice order */
            const uint32_t *more = sec.data() + kSegCap * fixw;
            for (uint32_t k = 0; k < kSegCap; ++k) {
                EXPECT_EQ(more[2 * s.n_more + k], 4 * k);
                const std::vector<Rec> got = decode(sec.data() + k * fixw, more, n);
                EXPECT_EQ(got.size(), (size_t)n);
                bool ok = got.size() == n;
                for (uint32_t i = 0; ok && i < n; ++i) {
                    const bool gate = !(k & 1);
                    ok = got[i].inst == i && (got[i].op & VEV_GATE_SET) && !(got[i].op & VEV_GATE_ON) == !gate &&
                         !(got[i].op & VEV_RETRIGGER) == !gate;
                }
                EXPECT_TRUE(ok);
            }
            EXPECT_TRUE(s.timed.empty() && s.events.empty());
        }
}

TEST(Timed, SpanAtTheCapExactly) {
    /* 16, 17, 32 and 33 distinct times, frame 0 among them: one launch, 16 + 1, 16 + 16, 16 + 16 + 1 */
    const uint32_t counts[] = {16, 17, 32, 33};
    for (const uint32_t times : counts) {
        Shadow s = fresh(OLFX_KIND_VOICE_SAMPLE, 70);
        std::vector<olfx_timed_event> evs;
        for (uint32_t k = 0; k < times; ++k) evs.push_back(tev(4 * k, k % 70, ON));
        EXPECT_EQ(queue(s, evs), OLFX_OK);
        const uint32_t total = 256;
        std::vector<uint32_t> spans, segs;
        for (uint32_t f0 = 0; f0 < total;) {
            const uint32_t span = s.span(total - f0);
            s.fold_segments(span);
            spans.push_back(span);
            segs.push_back(s.n_seg());
            s.advance(span);
            f0 += span;
        }
        const std::vector<uint32_t> want_spans = times == 16 ? std::vector<uint32_t>{256} : times == 17 ? std::vector<uint32_t>{64, 192}
                                               : times == 32 ? std::vector<uint32_t>{64, 192} : std::vector<uint32_t>{64, 64, 128};
        const std::vector<uint32_t> want_segs = times == 16 ? std::vector<uint32_t>{16} : times == 17 ? std::vector<uint32_t>{16, 1}
                                              : times == 32 ? std::vector<uint32_t>{16, 16} : std::vector<uint32_t>{16, 16, 1};
        EXPECT_TRUE(spans == want_spans);
        EXPECT_TRUE(segs == want_segs);
        EXPECT_TRUE(s.timed.empty() && s.events.empty());
    }
    /* the same 16 times past an empty frame 0 are 17 segments */
    Shadow s = fresh(OLFX_KIND_VOICE, 70);
    std::vector<olfx_timed_event> evs;
    for (uint32_t k = 1; k <= 16; ++k) evs.push_back(tev(4 * k, k, ON));
    EXPECT_EQ(queue(s, evs), OLFX_OK);
    EXPECT_EQ(s.span(68), 64u);
    EXPECT_EQ(s.span(64), 64u);
}

TEST(Timed, AdvanceWithAnEventAtTheSpan) {
    /* frame == span is frame 0 of the next launch, whether the span is the call's length or the cap's cut */
    Shadow s = fresh(OLFX_KIND_VOICE, 8);
    EXPECT_EQ(queue(s, {tev(64, 1, ON, 61), tev(64, 2, OFF), tev(68, 3, ON), tev(60, 4, ON)}), OLFX_OK);
    EXPECT_EQ(s.span(64), 64u);
    s.fold_segments(64);
    EXPECT_EQ(s.n_seg(), 2u);
    s.advance(64);
    EXPECT_EQ(s.events.size(), (size_t)2);
    EXPECT_EQ(s.events[0].inst, 1u);
    EXPECT_EQ(s.events[1].inst, 2u);
    EXPECT_EQ(s.timed.size(), (size_t)1);
    EXPECT_EQ(s.timed[0].frame, 4u);
    EXPECT_TRUE(s.has_events(4));
    s.reset();
    std::vector<olfx_timed_event> evs;
    for (uint32_t k = 0; k <= 16; ++k) evs.push_back(tev(4 * k, k % 8, ON, (uint8_t)(40 + k)));
    EXPECT_EQ(queue(s, evs), OLFX_OK);
    const uint32_t span = s.span(128);
    EXPECT_EQ(span, 64u);
    s.fold_segments(span);
    EXPECT_EQ(s.n_seg(), kSegCap);
    EXPECT_EQ(s.timed.size(), (size_t)1);
    s.advance(span);
    EXPECT_TRUE(s.timed.empty());
    EXPECT_EQ(s.events.size(), (size_t)1);
    EXPECT_EQ(s.events[0].note, 56);
    EXPECT_EQ(s.span(64), 64u);
    s.fold_segments(64);
    EXPECT_EQ(s.n_seg(), 1u);
    EXPECT_EQ(s.folded.size(), (size_t)1);
}

TEST(Timed, ChunksOfRaggedSpans) {
    /* n_chunks is the sum over the segments of their frames in chunks of 8, the last one up to the span */
    const uint32_t frames[] = {4, 16, 44, 48, 96};
    for (const uint32_t span : {100u, 104u, 128u, 300u}) {
        Shadow s = fresh(OLFX_KIND_VOICE_MOOG, 70);
        for (const uint32_t f : frames) {
            const olfx_timed_event e = tev(f, f % 70, ON);
            EXPECT_EQ(s.timed_events(&e, 1), OLFX_OK);
        }
        EXPECT_EQ(s.span(span), span);
        s.fold_segments(span);
        EXPECT_EQ(s.n_seg(), 6u);
        uint32_t want = 0;
        for (uint32_t k = 0; k < 6; ++k) {
            const uint32_t a = k ? frames[k - 1] : 0u, b = k < 5 ? frames[k] : span;
            want += (b - a + 7) / 8;
        }
        EXPECT_EQ(s.n_chunks(span, 8), want);
        EXPECT_TRUE(want > (span + 7) / 8);                                /* more than an unsegmented launch's */
    }
}

int main() { return run_all_tests(); }
