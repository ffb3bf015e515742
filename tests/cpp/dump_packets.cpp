// tests/cpp/dump_packets.cpp -- the control packets of the host core (ol_dsp_amd/csrc/olfx_host.cpp) for a set
// of small scenarios around the timed calls, as plain text: per launch the span, every PacketPlan field, the
// segments and chunks, the dirty lists' sizes before and after, and a 64-bit FNV-1a hash of the packet's words.
// tests/test_host_packets.py compares the output byte for byte with tests/golden/host_packets.txt.
// The Shadow is driven only through the calls olfx_engine.cpp makes (the queueing entry points, then span,
// has_events, fold_segments, plan, fill_records, write_events, write_timed_coefs, write_timed_inst, n_chunks and
// advance, looping launches over a block as olfx_process does), so the same source compiles against any
// arrangement of the Shadow's members.  The coefficient words come from libm's expf / powf: the hashes hold on
// the toolchain the golden file was written with.
// `dump_packets --time R` prints nothing of the above: it repeats the timed-parameter and the timed-instrument
// scenarios R times and prints the mean nanoseconds a launch spends from span() through the write_* calls.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../ol_dsp_amd/csrc/olfx_host.h"

using namespace olfx;
using host::Shadow;

namespace {

bool g_time = false;                         // --time: no output, the launches are timed
double g_ns = 0.0;
size_t g_launches = 0;
std::vector<uint32_t> g_buf(1u << 16);
size_t g_used = 0;                           // the words the last packet may have written

typedef struct olfx_timed_control TimedControl;
olfx_timed_param tp(uint32_t frame, uint32_t inst, uint32_t field, float value) { return olfx_timed_param{frame, inst, field, value}; }
TimedControl tc(uint32_t frame, uint32_t inst, uint8_t cc, float value, uint16_t pad = 0, uint8_t source = OLFX_CTL_MIDI) {
    return TimedControl{frame, olfx_control_event{inst, cc, source, pad, value}};
}
olfx_timed_note tn(uint32_t frame, uint32_t inst, uint8_t type, uint8_t note = 60) {
    return olfx_timed_note{frame, olfx_event{inst, type, note, 100, 0}};
}
olfx_timed_event te(uint32_t frame, uint32_t inst, uint8_t type, uint8_t note = 60, float value = 0.f) {
    return olfx_timed_event{frame, olfx_voice_event{inst, type, note, 100, 0, value}};
}
constexpr uint8_t ON = OLFX_EV_NOTE_ON, OFF = OLFX_EV_NOTE_OFF;
// corelib/cc_map.h
constexpr uint8_t CC_VOLUME = 7, CC_DELAY_TIME = 35, CC_DELAY_FEEDBACK = 36, CC_CUTOFF = 41, CC_FX_CUTOFF = 45, CC_ENV_AMP_A = 108,
                  CC_OSC_1_VOLUME = 114;

// a call's code, and its message when it refused
void said(const char *call, Shadow &s, int rc) {
    if (g_time) return;
    if (rc) std::printf("  %s: rc %d '%s'\n", call, rc, s.msg);
    else std::printf("  %s: rc 0\n", call);
}
void q(Shadow &s, const std::vector<olfx_timed_event> &r) { said("timed_events", s, s.timed_events(r.data(), (uint32_t)r.size())); }
void q(Shadow &s, const std::vector<olfx_timed_note> &r) { said("timed_notes", s, s.timed_notes(r.data(), (uint32_t)r.size())); }
void qp(Shadow &s, const std::vector<olfx_timed_param> &r) { said("timed_params", s, s.timed_params(r.data(), (uint32_t)r.size())); }
void qc(Shadow &s, const std::vector<TimedControl> &r) { said("timed_control", s, s.timed_control(r.data(), (uint32_t)r.size())); }
void qip(Shadow &s, const std::vector<olfx_timed_param> &r) {
    said("timed_instrument_params", s, s.timed_instrument_params(r.data(), (uint32_t)r.size()));
}
void qic(Shadow &s, const std::vector<TimedControl> &r) {
    said("timed_instrument_control", s, s.timed_instrument_control(r.data(), (uint32_t)r.size()));
}
void set(Shadow &s, uint32_t inst, uint32_t field, float v) { said("set_range", s, s.set_range(inst, 1, field, 1, &v)); }

uint64_t fnv1a(const uint32_t *w, size_t words) {
    uint64_t h = 0xcbf29ce484222325ull;
    const unsigned char *b = reinterpret_cast<const unsigned char *>(w);
    for (size_t k = 0; k < words * 4; ++k) h = (h ^ b[k]) * 0x100000001b3ull;
    return h;
}

// One block as olfx_process runs it: a launch per span, each with its packet (submit_control), then the advance.
void block(Shadow &s, uint32_t n_frames) {
    if (!g_time) std::printf("  block %u\n", n_frames);
    for (uint32_t f0 = 0; f0 < n_frames;) {
        std::memset(g_buf.data(), 0, g_used * 4);         // the up4 gaps are otherwise unspecified
        const auto t0 = std::chrono::steady_clock::now();
        const uint32_t span = s.span(n_frames - f0);
        const bool evs = host::takes_note_events(s.kind) && s.has_events(span);
        const size_t m = s.dirty_list.size(), m2 = s.vdirty_list.size();
        if (m || m2 || evs) {
            if (evs) s.fold_segments(span);
            const host::PacketPlan pl = s.plan(evs);
            if (g_buf.size() < pl.words + 4) g_buf.resize(pl.words + 4, 0u);
            g_used = pl.words + 4;
            uint32_t *buf = g_buf.data();
            s.fill_records(pl, buf);
            const bool materialise = s.rf_materialise;
            s.rf_materialise = false;
            if (evs) s.write_events(buf + pl.o_ev);
            if (pl.n_tc) s.write_timed_coefs(pl, buf);
            if (pl.n_iv + pl.n_if) s.write_timed_inst(pl, buf);
            const uint32_t chunks = evs ? s.n_chunks(span, kVoiceChunk) : 0u;
            if (g_time) {
                g_ns += std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count();
                ++g_launches;
            } else {
                std::printf("    launch f0 %u span %u evs %d dense %d o_inst %zu o_val %zu o_ev %zu words %zu n_seg %zu o_seg %zu "
                            "n_tc %zu o_tcb %zu o_tc %zu m2 %zu o_inst2 %zu o_val2 %zu n_iv %zu n_if %zu gv %zu gf %zu o_ivt %zu "
                            "o_ift %zu o_iv %zu o_if %zu | segs %u chunks %u dirty %zu->%zu vdirty %zu->%zu mat %d past %d hash %016llx\n",
                            f0, span, (int)evs, (int)pl.dense, pl.o_inst, pl.o_val, pl.o_ev, pl.words, pl.n_seg, pl.o_seg, pl.n_tc,
                            pl.o_tcb, pl.o_tc, pl.m2, pl.o_inst2, pl.o_val2, pl.n_iv, pl.n_if, pl.gv, pl.gf, pl.o_ivt, pl.o_ift,
                            pl.o_iv, pl.o_if, evs ? s.n_seg() : 1u, chunks, m, s.dirty_list.size(), m2, s.vdirty_list.size(),
                            (int)materialise, (int)((buf[pl.words] | buf[pl.words + 1] | buf[pl.words + 2] | buf[pl.words + 3]) != 0u),
                            (unsigned long long)fnv1a(buf, pl.words));
            }
        } else if (!g_time) {
            std::printf("    launch f0 %u span %u: no packet\n", f0, span);
        }
        s.rf.advance(span);
        s.advance(span);
        f0 += span;
    }
}

void title(const char *what, int kind, uint32_t n) {
    if (!g_time) std::printf("%s kind %d n %u\n", what, kind, n);
}

// ---- the voice kinds ----
Shadow voice_engine(int kind, uint32_t n) {
    Shadow s;
    s.init(kind, n, 48000.f);
    s.reset();
    if (kind == OLFX_KIND_VOICE_SAMPLE) {                 // a bank of two samples, a voice at each
        const uint64_t offsets[3] = {0, 100, 250};
        const float pcm = 0.f;                            // (the plan never reads the data)
        host::BankPlan plan;
        said("bank_plan", s, s.bank_plan(2, offsets, &pcm, &plan));
        s.bank_commit(std::move(plan));
        const olfx_sample_voice sv[2] = {{3, 0, OLFX_SAMPLE_ONESHOT, 0, 0, 0}, {n - 1, 1, OLFX_SAMPLE_LOOP, 0, 10, 120}};
        said("sample_voices", s, s.sample_voices(sv, 2));
    }
    return s;
}

// the timed parameter and control records of one block: at frame 0 and past it, two records on one voice at one
// time, Update() alone, events and records sharing a time
void queue_voice_records(Shadow &s) {
    const uint32_t n = s.n;
    q(s, {te(8, 5, ON, 64), te(24, 3, ON, 50), te(24, n - 1, OLFX_EV_SET_FREQUENCY, 0, 330.f)});
    qp(s, {tp(0, 2, OLFX_VC_FILTER_CUTOFF, 900.f), tp(8, 3, OLFX_VC_FILTER_CUTOFF, 1200.f), tp(8, 3, OLFX_VC_AMP_ATTACK, 0.05f),
           tp(8, 5, OLFX_VC_FILTER_RESONANCE, 0.4f), tp(16, n - 1, OLFX_VC_AMP_RELEASE, 0.3f), tp(16, 65, OLFX_VC_PORTAMENTO, 0.1f)});
    qc(s, {tc(0, 4, CC_VOLUME, 100.f), tc(8, 66, CC_CUTOFF, 64.f), tc(16, 3, CC_OSC_1_VOLUME, 10.f),
           tc(24, 3, CC_ENV_AMP_A, 0.25f, 0, OLFX_CTL_HARDWARE), tc(24, 7, 1, 5.f)});
    qp(s, {tp(8, 3, OLFX_VC_FILTER_CUTOFF, 1500.f), tp(40, 6, OLFX_VC_AMP_SUSTAIN, 0.5f)});
}

void voice_params_scenario(int kind, uint32_t n) {
    title("voice timed params", kind, n);
    Shadow s = voice_engine(kind, n);
    block(s, 64);
    queue_voice_records(s);
    block(s, 64);
    block(s, 64);                                         // nothing timed: the kept records are served and forgotten
    queue_voice_records(s);
    block(s, 64);
    set(s, 3, OLFX_VC_FILTER_RESONANCE, 0.7f);            // a kept voice written between the two launches
    block(s, 64);
    block(s, 64);
    // more than n records below the block: three times of n / 2 + 5 voices each, the third cuts the launch
    std::vector<olfx_timed_param> many;
    for (uint32_t t = 0; t < 3; ++t)
        for (uint32_t k = 0; k < n / 2 + 5; ++k) many.push_back(tp(4 * (t + 1), (k * 2 + t) % n, OLFX_VC_FILTER_CUTOFF, 100.f * (float)(t + 1) + (float)k));
    many.push_back(tp(8, 1, OLFX_VC_AMP_DECAY, 0.2f));    // a second record on a voice of that time
    qp(s, many);
    q(s, {te(8, 1, ON, 70), te(12, 2, OFF)});
    block(s, 64);
    block(s, 64);
}

void voice_event_scenarios(int kind, uint32_t n) {
    title("voice events", kind, n);
    Shadow s = voice_engine(kind, n);
    block(s, 64);                                         // the dense first packet
    // a crowded group: six records in group 0 of segment 0 and of the segment at 16; events at three times
    std::vector<olfx_voice_event> now;
    for (uint32_t v = 0; v < 6; ++v) now.push_back(olfx_voice_event{v * 3, ON, (uint8_t)(40 + v), 100, 0, 0.f});
    now.push_back(olfx_voice_event{n - 1, ON, 72, 100, 0, 0.f});
    said("voice_events", s, s.voice_events(now.data(), (uint32_t)now.size()));
    std::vector<olfx_timed_event> ev = {te(8, 1, ON, 61), te(32, 65, OLFX_EV_GATE_ON), te(32, 1, OFF, 61)};
    for (uint32_t v = 0; v < 7; ++v) ev.push_back(te(16, 63 - v * 2, v & 1 ? OFF : ON, (uint8_t)(50 + v)));
    q(s, ev);
    block(s, 64);
    // 17 distinct times in one block: the launch ends before the one that does not fit
    ev.clear();
    for (uint32_t t = 1; t <= 17; ++t) ev.push_back(te(4 * t, (t * 11) % n, ON, (uint8_t)(30 + t)));
    q(s, ev);
    block(s, 128);
    // the refusals: the frame check of each call
    q(s, {te(6, 0, ON)});
    q(s, {te(0x80000000u, 0, ON)});
    qp(s, {tp(4, 0, OLFX_VC_FILTER_CUTOFF, 1.f), tp(5, 0, OLFX_VC_FILTER_CUTOFF, 1.f)});
    qc(s, {tc(0x80000004u, 0, CC_VOLUME, 1.f)});
    qp(s, {tp(4, n, OLFX_VC_FILTER_CUTOFF, 1.f)});
    q(s, std::vector<olfx_timed_note>{tn(8, 0, ON)});
    qip(s, {tp(8, 0, 0, 1.f)});
    qic(s, {tc(8, 0, CC_VOLUME, 1.f)});
    block(s, 64);
}

// ---- the synths and the drum kit ----
bool is_kit(int kind) { return kind == OLFX_KIND_DRUMKIT; }
uint32_t rack0_of(int kind) { return is_kit(kind) ? OLFX_DK_RACK0 : OLFX_SY_RACK0; }
uint32_t voice0_of(int kind) { return is_kit(kind) ? OLFX_DK_VOICE0 : OLFX_SY_VOICE0; }

Shadow instrument_engine(int kind, uint32_t n, uint32_t voices) {
    Shadow s;
    s.init(kind, n, 48000.f, voices);
    s.reset();
    if (is_kit(kind)) {                                   // voice p of every kit at note 36 + p and channel p
        std::vector<olfx_drumkit_voice> map;
        for (uint32_t i = 0; i < n; ++i)
            for (uint32_t p = 0; p < voices; ++p) map.push_back(olfx_drumkit_voice{i, p, (uint8_t)p, (uint8_t)(36 + p), 0});
        said("drumkit_map", s, s.drumkit_map(map.data(), (uint32_t)map.size()));
        const uint64_t offsets[2] = {0, 64};
        const float pcm = 0.f;
        host::BankPlan plan;
        said("bank_plan", s, s.bank_plan(1, offsets, &pcm, &plan));
        s.bank_commit(std::move(plan));
        const olfx_sample_voice sv[2] = {{7 * voices + 2, 0, OLFX_SAMPLE_ONESHOT, 0, 0, 0}, {1, 0, OLFX_SAMPLE_LOOP, 0, 4, 60}};
        said("sample_voices", s, s.sample_voices(sv, 2));
    }
    return s;
}

// records that touch voice fields only (8), rack fields only (16) and both (24), notes sharing two of the times
void queue_instrument_records(Shadow &s) {
    const int kind = s.kind;
    const uint32_t v0 = voice0_of(kind), r0 = rack0_of(kind), n = s.n;
    const uint8_t note = is_kit(kind) ? 38 : 60;
    q(s, {tn(16, 5, ON, note), tn(24, 7, ON, note), tn(24, n - 1, ON, is_kit(kind) ? 37 : 64), tn(40, 5, OFF, note)});
    qip(s, {tp(0, 1, v0 + OLFX_VC_AMP_ATTACK, 0.02f), tp(8, 3, v0 + OLFX_VC_FILTER_CUTOFF, 700.f),
            tp(8, 3, v0 + OLFX_VC_AMP_ATTACK, 0.05f), tp(8, 66, v0 + OLFX_VC_FILTER_RESONANCE, 0.3f),
            tp(16, 3, r0 + OLFX_FR_FILTER_CUTOFF, 5000.f), tp(16, n - 1, r0 + OLFX_FR_REVERB_BALANCE, 0.4f),
            tp(24, 5, v0 + OLFX_VC_AMP_RELEASE, 0.2f), tp(24, 5, r0 + OLFX_FR_MASTER_VOLUME, 0.5f),
            tp(24, 7, r0 + OLFX_FR_FILTER_RESONANCE, 0.2f)});
    // controls: one that reaches a voice field and a rack field, Update() alone, the rack's volume, an ignored one
    qic(s, {tc(0, 2, CC_VOLUME, 90.f, OLFX_DK_CHANNEL_RACK), tc(8, 7, CC_CUTOFF, 64.f, 2), tc(16, 7, CC_OSC_1_VOLUME, 3.f, 1),
            tc(24, 7, CC_CUTOFF, 80.f, OLFX_DK_CHANNEL_RACK), tc(24, 3, CC_ENV_AMP_A, 0.3f, 0, OLFX_CTL_HARDWARE),
            tc(32, 9, 1, 5.f, 0), tc(32, 7, CC_VOLUME, 70.f, 9), tc(32, 7, CC_VOLUME, 60.f, 3)});
    if (is_kit(kind))                                     // a slot past the kit's voices: stored, read by nothing
        qip(s, {tp(32, 7, v0 + 5 * OLFX_VC_NPARAMS + OLFX_VC_AMP_DECAY, 0.1f), tp(32, 7, v0 + 2 * OLFX_VC_NPARAMS + OLFX_VC_AMP_DECAY, 0.1f)});
}

void instrument_scenario(int kind, uint32_t n, uint32_t voices) {
    title("instrument timed params", kind, n);
    Shadow s = instrument_engine(kind, n, voices);
    const uint32_t v0 = voice0_of(kind), r0 = rack0_of(kind);
    block(s, 64);                                         // the dense first packet
    q(s, {tn(8, 1, ON, is_kit(kind) ? 36 : 60), tn(8, 5, ON, is_kit(kind) ? 39 : 62), tn(16, 69, ON, is_kit(kind) ? 36 : 60),
          tn(16, 1, OFF, is_kit(kind) ? 36 : 60), tn(0, 2, ON, is_kit(kind) ? 37 : 50)});
    block(s, 64);                                         // timed notes alone
    queue_instrument_records(s);
    block(s, 64);
    block(s, 64);                                         // an untimed launch: the kept records are served and forgotten
    queue_instrument_records(s);
    block(s, 64);
    set(s, 5, r0 + OLFX_FR_FILTER_CUTOFF, 2500.f);        // writes to a kept instrument and a kept voice (slot)
    set(s, 7, v0 + (is_kit(kind) ? 2 * OLFX_VC_NPARAMS : 0) + OLFX_VC_AMP_DECAY, 0.4f);
    block(s, 64);
    block(s, 64);
    // boundary records in the middle of a block: the topology (then a control whose mapping depends on it), a delay
    // field and CC 35 each end the launch and land at the next one's frame 0
    const float topo = kind == OLFX_KIND_SYNTH ? 1.f : 0.f;
    qip(s, {tp(8, 2, r0 + OLFX_FR_TOPOLOGY, topo), tp(4, 2, v0 + OLFX_VC_AMP_DECAY, 0.3f), tp(24, 4, r0 + OLFX_FR_DELAY_FEEDBACK, 0.6f)});
    qic(s, {tc(16, 2, CC_FX_CUTOFF, 64.f, OLFX_DK_CHANNEL_RACK), tc(16, 2, CC_CUTOFF, 64.f, OLFX_DK_CHANNEL_RACK),
            tc(40, 6, CC_DELAY_TIME, 30.f, OLFX_DK_CHANNEL_RACK), tc(40, 6, CC_DELAY_FEEDBACK, 30.f, 1),
            tc(48, 2, CC_FX_CUTOFF, 100.f, OLFX_DK_CHANNEL_RACK)});
    q(s, {tn(16, 2, ON, is_kit(kind) ? 36 : 60)});
    block(s, 64);
    block(s, 64);
    if (kind != OLFX_KIND_SYNTH) {                        // back to the firmware's chain, in a block of its own
        qip(s, {tp(8, 2, r0 + OLFX_FR_TOPOLOGY, 1.f)});
        qic(s, {tc(8, 2, CC_FX_CUTOFF, 64.f, OLFX_DK_CHANNEL_RACK), tc(8, 2, CC_CUTOFF, 70.f, OLFX_DK_CHANNEL_RACK)});
        block(s, 64);
        block(s, 64);
    }
    // the record cap: three times of 3/7 of the cap each, the third ends the launch
    const uint32_t cap = host::timed_instrument_cap(kind, n, voices), per = cap * 3 / 7;
    std::vector<olfx_timed_param> many;
    for (uint32_t t = 0; t < 3; ++t)
        for (uint32_t k = 0; k < per; ++k) {
            const uint32_t lane = (k + t * 5) % cap, slot = is_kit(kind) ? lane / n : 0u;
            many.push_back(tp(4 * (t + 1), lane % n, v0 + slot * OLFX_VC_NPARAMS + OLFX_VC_FILTER_CUTOFF, 50.f * (float)(t + 1) + (float)k));
        }
    many.push_back(tp(8, 0, r0 + OLFX_FR_FILTER_CUTOFF, 3000.f));
    qip(s, many);
    block(s, 64);
    block(s, 64);
    // records pending across blocks
    qip(s, {tp(72, 9, v0 + OLFX_VC_FILTER_CUTOFF, 444.f), tp(136, 9, r0 + OLFX_FR_REVERB_BALANCE, 0.7f), tp(64, 10, r0 + OLFX_FR_FILTER_CUTOFF, 999.f)});
    qic(s, {tc(128, 11, CC_CUTOFF, 20.f, 0), tc(140, 12, CC_VOLUME, 20.f, OLFX_DK_CHANNEL_RACK)});
    q(s, {tn(72, 9, ON, is_kit(kind) ? 36 : 60), tn(200, 9, OFF, is_kit(kind) ? 36 : 60)});
    block(s, 64);
    block(s, 64);
    block(s, 64);
    block(s, 64);
    // reset() with records pending
    queue_instrument_records(s);
    s.reset();
    block(s, 64);
    block(s, 64);
    // the refusals: the frame check of each call
    q(s, {tn(2, 0, ON)});
    qip(s, {tp(7, 0, v0, 1.f)});
    qic(s, {tc(0x80000000u, 0, CC_VOLUME, 1.f)});
    qip(s, {tp(8, n, v0, 1.f)});
    q(s, std::vector<olfx_timed_event>{te(8, 0, ON)});
    qp(s, {tp(8, 0, 0, 1.f)});
    qc(s, {tc(8, 0, CC_VOLUME, 1.f)});
    block(s, 64);
}

// the chorus kind: fill_records' pitch_sent / rf_materialise path
void chorus_scenario(uint32_t n) {
    title("chorus", OLFX_KIND_CHORUS, n);
    Shadow s;
    s.init(OLFX_KIND_CHORUS, n, 48000.f);
    s.reset();
    block(s, 64);
    set(s, 3, OLFX_CH_MIX, 0.25f);                        // no pitch or window word changes
    block(s, 64);
    set(s, 3, OLFX_CH_PITCH, 1.5f);                       // materialise
    block(s, 64);
    set(s, 3, OLFX_CH_PITCH, 1.5f);                       // the same words: no change
    set(s, 69, OLFX_CH_WINDOW, 6.f);                      // already on the ring kernel: nothing to materialise
    block(s, 64);
    block(s, 4096);
    set(s, 5, OLFX_CH_WINDOW, 7.f);
    block(s, 64);
}

constexpr int kVoiceKinds[] = {OLFX_KIND_VOICE, OLFX_KIND_VOICE_MOOG, OLFX_KIND_VOICE_SAMPLE};
constexpr int kInstrumentKinds[] = {OLFX_KIND_SYNTH, OLFX_KIND_SYNTH_SVF, OLFX_KIND_DRUMKIT};

}  // namespace

int main(int argc, char **argv) {
    if (argc == 3 && !std::strcmp(argv[1], "--time")) {
        const long reps = std::atol(argv[2]);
        g_time = true;
        for (long r = 0; r < reps; ++r)
            for (const int kind : kVoiceKinds)
                for (const uint32_t n : {70u, 130u}) voice_params_scenario(kind, n);
        std::printf("timed_params launches %zu ns_per_launch %.1f\n", g_launches, g_launches ? g_ns / (double)g_launches : 0.0);
        g_ns = 0.0;
        g_launches = 0;
        for (long r = 0; r < reps; ++r)
            for (const int kind : kInstrumentKinds) instrument_scenario(kind, 70, 4);
        std::printf("timed_instrument launches %zu ns_per_launch %.1f\n", g_launches, g_launches ? g_ns / (double)g_launches : 0.0);
        return 0;
    }
    for (const int kind : kVoiceKinds)
        for (const uint32_t n : {70u, 130u}) {
            voice_event_scenarios(kind, n);
            voice_params_scenario(kind, n);
        }
    for (const int kind : kInstrumentKinds) instrument_scenario(kind, 70, 4);
    chorus_scenario(70);
    return 0;
}
