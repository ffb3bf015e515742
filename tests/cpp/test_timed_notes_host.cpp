/*
 * tests/cpp/test_timed_notes_host.cpp -- olfx_timed_notes in the engine's HIP-free host core
 * (ol_dsp_amd/csrc/olfx_host.h) on the CPU: a note is routed through Polyvoice / the VoiceMap when the engine
 * reaches its frame.  Routing over time on a two-voice synth (the per-segment folded voice events and Playing()),
 * the carry-over (a note at frame == N is routed as the call returns, ahead of a later untimed one; a note past N
 * over two calls), notes queued in mixed order, the drum kit (a map change reroutes pending notes, an unmapped note
 * is an empty segment, GATE_ON is refused), validation (a refused call changes nothing) and the refusals per kind,
 * a frame-0-only queue's packet against olfx_note_events', the span at exactly 16 and 17 times, and the worst
 * packet against max_packet_words.  Links olfx_host.cpp directly (no libolfx.so, no GPU); built by
 * tests/test_timed_notes_host.py with its own build line.
 */
#include "../../ol_dsp_amd/csrc/olfx_host.h"
#include "harness.h"

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

olfx_event nev(uint32_t inst, uint8_t type, uint8_t note = 60) { return olfx_event{inst, type, note, 100, 0}; }
olfx_timed_note tn(uint32_t frame, uint32_t inst, uint8_t type, uint8_t note = 60) { return olfx_timed_note{frame, nev(inst, type, note)}; }
int queue(Shadow &s, const std::vector<olfx_timed_note> &e) { return s.timed_notes(e.data(), (uint32_t)e.size()); }
int untimed(Shadow &s, const std::vector<olfx_event> &e) { return s.note_events(e.data(), (uint32_t)e.size()); }

/* the kit's map: voice p of every kit at note 36 + p */
void map_kit(Shadow &s) {
    std::vector<olfx_drumkit_voice> recs;
    for (uint32_t i = 0; i < s.n; ++i)
        for (uint32_t p = 0; p < s.voices; ++p) {
            olfx_drumkit_voice r{};
            r.kit = i;
            r.voice = p;
            r.note = 36 + p;
            r.channel = p;
            recs.push_back(r);
        }
    EXPECT_EQ(s.drumkit_map(recs.data(), (uint32_t)recs.size()), OLFX_OK);
}

/* the launch of `span` frames: its whole packet */
std::vector<uint32_t> packet(Shadow &s, uint32_t span, host::PacketPlan *plan = nullptr) {
    s.fold_segments(span);
    const host::PacketPlan pl = s.plan(true);
    std::vector<uint32_t> buf(pl.words + 4, 0xDEADBEEFu);
    s.fill_records(pl, buf.data());
    s.write_events(buf.data() + pl.o_ev);
    for (size_t k = pl.words; k < buf.size(); ++k) EXPECT_EQ(buf[k], 0xDEADBEEFu);       /* nothing past the plan */
    if (plan) *plan = pl;
    buf.resize(pl.words);
    return buf;
}

/* segment sgm of the last fold as (voice slot, op) in order of first appearance */
struct Rec { uint32_t slot, op; bool operator==(const Rec &o) const { return slot == o.slot && op == o.op; } };
std::vector<Rec> segment(const Shadow &s, uint32_t sgm) {
    std::vector<Rec> out;
    for (uint32_t f = s.seg_first[sgm]; f < s.seg_first[sgm + 1]; ++f) out.push_back(Rec{s.folded[f].inst, s.folded[f].op});
    return out;
}
std::vector<uint8_t> playing(Shadow &s, uint32_t inst) {
    std::vector<uint8_t> p(s.voices);
    EXPECT_EQ(s.synth_playing(inst, p.data()), OLFX_OK);
    return p;
}

constexpr uint8_t ON = OLFX_EV_NOTE_ON, OFF = OLFX_EV_NOTE_OFF, GON = OLFX_EV_GATE_ON, GOFF = OLFX_EV_GATE_OFF;
constexpr uint32_t kOn = VEV_GATE_SET | VEV_GATE_ON | VEV_RETRIGGER | VEV_FREQ, kOff = VEV_GATE_SET;
const int kInstruments[] = {OLFX_KIND_SYNTH, OLFX_KIND_SYNTH_SVF, OLFX_KIND_DRUMKIT};

}  // namespace

TEST(TimedNotes, RoutingOverTime) {
    /* P = 2: NoteOn x 2 at frame 0, a third at 4 (no free voice at its frame: dropped), NoteOff at 8, NoteOn at 12
       (takes the voice freed at 8); on instruments 1 and 69 of 70 (voice slot p * npad + i, npad = 128) */
    for (const int kind : {OLFX_KIND_SYNTH, OLFX_KIND_SYNTH_SVF}) {
        Shadow s = fresh(kind, 70, 2);
        EXPECT_EQ(s.npad, 128u);
        for (const uint32_t i : {1u, 69u})
            EXPECT_EQ(queue(s, {tn(12, i, ON, 72), tn(0, i, ON, 60), tn(4, i, ON, 67), tn(0, i, ON, 64), tn(8, i, OFF, 60)}), OLFX_OK);
        /* frame 0 was routed at the call, the rest is pending and Playing() does not know it */
        EXPECT_EQ(s.events.size(), (size_t)4);
        EXPECT_EQ(s.timed.size(), (size_t)6);
        EXPECT_TRUE(playing(s, 1) == (std::vector<uint8_t>{60, 64}));
        EXPECT_EQ(s.span(64), 64u);
        EXPECT_TRUE(s.has_events(64));
        s.fold_segments(64);
        EXPECT_EQ(s.n_seg(), 4u);
        const uint32_t frames[] = {0, 4, 8, 12};
        for (uint32_t k = 0; k < 4; ++k) EXPECT_EQ(s.seg_frame[k], frames[k]);
        EXPECT_TRUE(segment(s, 0) == (std::vector<Rec>{{1, kOn}, {128 + 1, kOn}, {69, kOn}, {128 + 69, kOn}}));
        EXPECT_TRUE(segment(s, 1).empty());                               /* dropped: an empty segment */
        EXPECT_TRUE(segment(s, 2) == (std::vector<Rec>{{1, kOff}, {69, kOff}}));
        EXPECT_TRUE(segment(s, 3) == (std::vector<Rec>{{1, kOn}, {69, kOn}}));
        EXPECT_TRUE(playing(s, 1) == (std::vector<uint8_t>{72, 64}));
        EXPECT_TRUE(playing(s, 69) == (std::vector<uint8_t>{72, 64}));
        EXPECT_TRUE(playing(s, 0) == (std::vector<uint8_t>{0, 0}));
        EXPECT_TRUE(s.timed.empty() && s.events.empty());
        /* gates fan out to every voice at their frame */
        EXPECT_EQ(queue(s, {tn(8, 1, GOFF), tn(16, 1, GON)}), OLFX_OK);
        s.fold_segments(64);
        EXPECT_EQ(s.n_seg(), 3u);
        EXPECT_TRUE(segment(s, 1) == (std::vector<Rec>{{1, kOff}, {128 + 1, kOff}}));
        EXPECT_TRUE(segment(s, 2) == (std::vector<Rec>{{1, VEV_GATE_SET | VEV_GATE_ON}, {128 + 1, VEV_GATE_SET | VEV_GATE_ON}}));
    }
}

TEST(TimedNotes, CarryOver) {
    Shadow s = fresh(OLFX_KIND_SYNTH, 8, 2);
    EXPECT_EQ(untimed(s, {nev(3, ON, 60), nev(3, ON, 64)}), OLFX_OK);
    /* a NoteOff at frame == N, a NoteOn two calls on */
    EXPECT_EQ(queue(s, {tn(64, 3, OFF, 60), tn(128 + 8, 3, ON, 81), tn(128 + 4, 3, OFF, 64)}), OLFX_OK);
    EXPECT_EQ(s.span(64), 64u);
    s.fold_segments(64);
    EXPECT_EQ(s.n_seg(), 1u);
    EXPECT_TRUE(playing(s, 3) == (std::vector<uint8_t>{60, 64}));
    s.advance(64);
    /* routed as the call returned: Playing() shows it, and the untimed NoteOn of the same note queued now finds that
       voice (routed behind it, it would have found no free voice while the NoteOff still closed the gate) */
    EXPECT_TRUE(playing(s, 3) == (std::vector<uint8_t>{0, 64}));
    EXPECT_EQ(s.events.size(), (size_t)1);
    EXPECT_EQ(untimed(s, {nev(3, ON, 60)}), OLFX_OK);
    EXPECT_TRUE(playing(s, 3) == (std::vector<uint8_t>{60, 64}));
    EXPECT_EQ(s.timed.size(), (size_t)2);
    EXPECT_EQ(s.timed[0].frame, 68u);
    s.fold_segments(64);
    EXPECT_EQ(s.n_seg(), 1u);
    /* voice 0: NoteOff then NoteOn in one block -- retriggered with the gate on */
    EXPECT_TRUE(segment(s, 0) == (std::vector<Rec>{{3, kOn}}));
    s.advance(64);
    EXPECT_EQ(s.timed[0].frame, 4u);
    EXPECT_EQ(s.timed[1].frame, 8u);
    EXPECT_TRUE(s.events.empty());
    s.fold_segments(64);
    EXPECT_EQ(s.n_seg(), 3u);
    EXPECT_TRUE(segment(s, 1) == (std::vector<Rec>{{64 + 3, kOff}}));           /* voice 1: slot npad + 3 */
    EXPECT_TRUE(segment(s, 2) == (std::vector<Rec>{{64 + 3, kOn}}));
    EXPECT_TRUE(playing(s, 3) == (std::vector<uint8_t>{60, 81}));
    /* reset drops pending notes */
    EXPECT_EQ(queue(s, {tn(8, 0, ON)}), OLFX_OK);
    s.reset();
    EXPECT_TRUE(s.timed.empty() && s.events.empty());
    EXPECT_TRUE(playing(s, 3) == (std::vector<uint8_t>{0, 0}));
}

TEST(TimedNotes, MixedOrder) {
    /* an untimed note queued after timed ones is routed at its call, against a Playing() that ignores the pending: a
       NoteOn is pending at frame 8, and the untimed NoteOn queued after it takes voice 0 all the same; a frame-0 timed
       NoteOff queued later releases that voice at its call; at frame 8 the pending NoteOns find voices 0 and 1 in
       queueing order */
    Shadow s = fresh(OLFX_KIND_SYNTH_SVF, 4, 2);
    EXPECT_EQ(queue(s, {tn(8, 2, ON, 70)}), OLFX_OK);
    EXPECT_TRUE(playing(s, 2) == (std::vector<uint8_t>{0, 0}));
    EXPECT_EQ(untimed(s, {nev(2, ON, 50)}), OLFX_OK);
    EXPECT_TRUE(playing(s, 2) == (std::vector<uint8_t>{50, 0}));
    EXPECT_EQ(queue(s, {tn(0, 2, OFF, 50), tn(8, 2, ON, 71)}), OLFX_OK);          /* frame 0: at the call, in call order */
    EXPECT_TRUE(playing(s, 2) == (std::vector<uint8_t>{0, 0}));
    s.fold_segments(64);
    EXPECT_EQ(s.n_seg(), 2u);
    EXPECT_TRUE(segment(s, 0) == (std::vector<Rec>{{2, VEV_GATE_SET | VEV_RETRIGGER | VEV_FREQ}}));
    EXPECT_TRUE(segment(s, 1) == (std::vector<Rec>{{2, kOn}, {64 + 2, kOn}}));
    EXPECT_TRUE(playing(s, 2) == (std::vector<uint8_t>{70, 71}));
}

TEST(TimedNotes, DrumKit) {
    Shadow s = fresh(OLFX_KIND_DRUMKIT, 3, 4);
    map_kit(s);
    EXPECT_EQ(queue(s, {tn(8, 1, ON, 36), tn(12, 1, ON, 99), tn(72, 1, ON, 36)}), OLFX_OK);
    EXPECT_EQ(queue(s, {tn(4, 1, GON, 36)}), OLFX_E_ARG);                 /* a drum kit takes NoteOn and NoteOff only */
    EXPECT_EQ(queue(s, {tn(4, 1, GOFF, 36)}), OLFX_E_ARG);
    EXPECT_EQ(s.timed.size(), (size_t)3);
    s.fold_segments(64);
    EXPECT_EQ(s.n_seg(), 3u);
    const uint32_t on = kOn | VEV_SEEK;
    EXPECT_TRUE(segment(s, 1) == (std::vector<Rec>{{0 * 64 + 1, on}}));
    EXPECT_TRUE(segment(s, 2).empty());                                   /* nobody sits at 99 */
    EXPECT_TRUE(playing(s, 1) == (std::vector<uint8_t>{36, 0, 0, 0}));
    s.advance(64);
    /* a map change with a note pending: note 36 now belongs to voice 2 (voice 0 sits nowhere) */
    olfx_drumkit_voice recs[2] = {};
    recs[0].kit = 1; recs[0].voice = OLFX_DK_NO_VOICE; recs[0].note = 38; recs[0].channel = OLFX_DK_NO_CHANNEL;
    recs[1].kit = 1; recs[1].voice = 2; recs[1].note = 36; recs[1].channel = OLFX_DK_NO_CHANNEL;
    EXPECT_EQ(s.drumkit_map(recs, 2), OLFX_OK);
    s.fold_segments(64);
    EXPECT_EQ(s.n_seg(), 2u);
    EXPECT_EQ(s.seg_frame[1], 8u);
    EXPECT_TRUE(segment(s, 1) == (std::vector<Rec>{{2 * 64 + 1, on}}));
    EXPECT_TRUE(playing(s, 1) == (std::vector<uint8_t>{36, 0, 36, 0}));
}

TEST(TimedNotes, RefusalsPerKind) {
    const olfx_timed_note e = tn(8, 0, ON);
    for (const int kind : kInstruments) {
        Shadow s = fresh(kind, 4);
        if (kind == OLFX_KIND_DRUMKIT) map_kit(s);
        EXPECT_EQ(s.timed_notes(&e, 1), OLFX_OK);
        EXPECT_EQ(s.timed.size(), (size_t)1);
        EXPECT_EQ(s.timed_notes(nullptr, 0), OLFX_OK);
    }
    for (const int kind : {OLFX_KIND_VOICE, OLFX_KIND_VOICE_MOOG, OLFX_KIND_VOICE_SAMPLE}) {
        Shadow s = fresh(kind, 4);
        EXPECT_EQ(s.timed_notes(&e, 1), OLFX_E_KIND);
        EXPECT_TRUE(s.timed.empty() && s.events.empty() && s.msg[0] != 0);
    }
    for (const int kind : {OLFX_KIND_DATTORRO, OLFX_KIND_CHORUS, OLFX_KIND_PITCHSHIFT, OLFX_KIND_CHAIN, OLFX_KIND_FXRACK,
                           OLFX_KIND_PLATERACK, OLFX_KIND_METER, OLFX_KIND_METER_MONO}) {
        Shadow s = fresh(kind, 4);
        EXPECT_EQ(s.timed_notes(&e, 1), OLFX_E_STATE);
    }
    /* the pins: olfx_timed_events still refuses the instruments, and its launches still take one segment there */
    EXPECT_EQ(host::max_segments(OLFX_KIND_SYNTH), 1u);
    EXPECT_EQ(host::max_segments(OLFX_KIND_DRUMKIT), 1u);
    for (const int kind : kInstruments) EXPECT_EQ(host::max_note_segments(kind), kSegCap);
    for (const int kind : {OLFX_KIND_VOICE, OLFX_KIND_VOICE_MOOG, OLFX_KIND_VOICE_SAMPLE, OLFX_KIND_FXRACK, OLFX_KIND_METER})
        EXPECT_EQ(host::max_note_segments(kind), 1u);
}

TEST(TimedNotes, BadRecordsChangeNothing) {
    for (const int kind : kInstruments) {
        Shadow s = fresh(kind, 10, 2);
        if (kind == OLFX_KIND_DRUMKIT) map_kit(s);
        EXPECT_EQ(queue(s, {tn(8, 1, ON, 36), tn(0, 2, ON, 37)}), OLFX_OK);
        const std::vector<olfx_timed_event> timed = s.timed;
        const std::vector<uint8_t> pl = s.playing;
        const size_t queued = s.events.size();
        EXPECT_EQ(queued, (size_t)1);
        std::vector<olfx_timed_note> bad = {tn(6, 0, ON), tn(0x80000000u, 0, ON), tn(0xFFFFFFFCu, 0, ON), tn(8, 10, ON),
                                            tn(8, 0, ON, 128), tn(8, 0, OLFX_EV_SET_FREQUENCY), tn(8, 0, 5)};
        if (kind == OLFX_KIND_DRUMKIT) bad.push_back(tn(8, 0, GON, 36));
        for (const olfx_timed_note &b : bad) {
            /* good records ahead of the bad one, one of them at frame 0: neither queued nor routed */
            EXPECT_EQ(queue(s, {tn(4, 5, ON, 36), tn(0, 6, ON, 36), b}), OLFX_E_ARG);
            EXPECT_TRUE(s.msg[0] != 0);
            EXPECT_EQ(s.timed.size(), timed.size());
            EXPECT_TRUE(std::memcmp(s.timed.data(), timed.data(), timed.size() * sizeof(olfx_timed_event)) == 0);
            EXPECT_EQ(s.events.size(), queued);
            EXPECT_TRUE(s.playing == pl);
        }
        EXPECT_EQ(s.timed_notes(nullptr, 1), OLFX_E_ARG);
        EXPECT_EQ(queue(s, {tn(0x7FFFFFFCu, 9, ON, 36)}), OLFX_OK);                 /* the last frame there is */
        EXPECT_EQ(s.timed.size(), timed.size() + 1);
    }
}

TEST(TimedNotes, FrameZeroOnlyIsTodaysPacket) {
    /* the same notes through olfx_timed_notes at frame 0 and through olfx_note_events, a rack field dirty too: the
       whole packet, word for word, and one segment; a note past the block is not in it */
    for (const int kind : kInstruments)
        for (const uint32_t voices : {1u, 4u, 8u}) {
            Shadow a = fresh(kind, 130, voices), b = fresh(kind, 130, voices);
            if (kind == OLFX_KIND_DRUMKIT) { map_kit(a); map_kit(b); }
            std::vector<olfx_timed_note> evs;
            for (uint32_t i = 0; i < 130; i += 3)
                for (uint32_t p = 0; p < voices; ++p) evs.push_back(tn(0, i, ON, (uint8_t)(36 + p)));
            for (uint32_t i = 0; i < 130; i += 6) evs.push_back(tn(0, i, OFF, 36));
            evs.push_back(tn(256, 7, ON, 36));
            EXPECT_EQ(queue(a, evs), OLFX_OK);
            for (const olfx_timed_note &e : evs)
                if (!e.frame) EXPECT_EQ(b.note_events(&e.ev, 1), OLFX_OK);
            EXPECT_TRUE(a.playing == b.playing);
            EXPECT_EQ(a.span(256), 256u);
            host::PacketPlan pa;
            const std::vector<uint32_t> wa = packet(a, 256, &pa);
            b.fold_events();
            const host::PacketPlan pb = b.plan(true);
            std::vector<uint32_t> wb(pb.words, 0xDEADBEEFu);
            b.fill_records(pb, wb.data());
            b.write_events(wb.data() + pb.o_ev);
            EXPECT_EQ(a.n_seg(), 1u);
            EXPECT_EQ(pa.n_seg, (size_t)1);
            EXPECT_EQ(pa.o_seg, (size_t)0);
            EXPECT_EQ(pa.words, pb.words);
            EXPECT_TRUE(wa == wb);
            EXPECT_EQ(a.timed.size(), (size_t)1);
        }
}

TEST(TimedNotes, SpanAtTheCapExactly) {
    for (const int kind : kInstruments)
        for (const uint32_t times : {16u, 17u}) {
            Shadow s = fresh(kind, 70);
            if (kind == OLFX_KIND_DRUMKIT) map_kit(s);
            std::vector<olfx_timed_note> evs;
            for (uint32_t k = 0; k < times; ++k) evs.push_back(tn(4 * k, k % 70, ON, 36));
            EXPECT_EQ(queue(s, evs), OLFX_OK);
            std::vector<uint32_t> spans, segs;
            for (uint32_t f0 = 0; f0 < 128;) {
                const uint32_t span = s.span(128 - f0);
                s.fold_segments(span);
                spans.push_back(span);
                segs.push_back(s.n_seg());
                s.advance(span);
                f0 += span;
            }
            EXPECT_TRUE(spans == (times == 16 ? std::vector<uint32_t>{128} : std::vector<uint32_t>{64, 64}));
            EXPECT_TRUE(segs == (times == 16 ? std::vector<uint32_t>{16} : std::vector<uint32_t>{16, 1}));
            EXPECT_TRUE(s.timed.empty() && s.events.empty());
            EXPECT_EQ(playing(s, 5)[0], 36);
        }
}

TEST(TimedNotes, WorstPacketFitsTheMaximum) {
    /* every voice of every instrument with a record in each of kSegCap segments -- NoteOn on every voice and NoteOff
       of every voice in turn, so that no note is dropped -- every coefficient dirty: every full group is crowded
       in every segment.  groups = voices * npad / 64, group p * (npad / 64) + g */
    for (const int kind : kInstruments)
        for (const uint32_t n : {1u, 64u, 65u, 130u})
            for (const uint32_t voices : {1u, 4u, 8u}) {
                Shadow s;
                s.init(kind, n, 48000.f, voices);
                s.reset();                                                     /* all dirty */
                if (kind == OLFX_KIND_DRUMKIT) map_kit(s);
                std::vector<olfx_timed_note> evs;
                for (uint32_t k = 0; k < kSegCap; ++k)
                    for (uint32_t i = 0; i < n; ++i)
                        for (uint32_t p = 0; p < voices; ++p) evs.push_back(tn(4 * k, i, k & 1 ? OFF : ON, (uint8_t)(36 + p)));
                EXPECT_EQ(queue(s, evs), OLFX_OK);
                EXPECT_EQ(s.span(64), 64u);
                host::PacketPlan pl;
                const std::vector<uint32_t> w = packet(s, 64, &pl);
                const uint32_t npad = (n + 63) / 64 * 64, groups = voices * npad / 64;
                EXPECT_EQ(s.n_ev(), voices * npad);
                EXPECT_EQ(pl.n_seg, (size_t)kSegCap);
                EXPECT_EQ(s.ev_count.size(), (size_t)kSegCap * groups);
                for (uint32_t k = 0; k < kSegCap; ++k) {
                    EXPECT_EQ(w[pl.o_seg + k], 4 * k);
                    for (uint32_t p = 0; p < voices; ++p)
                        for (uint32_t g = 0; g < npad / 64; ++g)
                            EXPECT_EQ(s.ev_count[(size_t)k * groups + p * (npad / 64) + g], std::min(64u, n - 64 * g));
                }
                const size_t most = host::max_packet_words(kind, n, s.n_ev(), host::max_note_segments(kind));
                EXPECT_TRUE(pl.words <= most);
                if (n >= 64) EXPECT_TRUE(pl.words > host::max_packet_words(kind, n, s.n_ev()));   /* ... not one segment's */
                EXPECT_TRUE(s.timed.empty() && s.events.empty());
            }
}

int main() { return run_all_tests(); }
