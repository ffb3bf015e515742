// ol_dsp_amd/csrc/olfx_host.h -- the host's control logic that touches neither the GPU nor a HIP
// type: the kind table, the reference's setter arithmetic (parameters -> coefficient words), the
// host shadow of an engine's parameters with its validation and bookkeeping, and the format of the
// control packet.  olfx_engine.cpp owns a Shadow by value and delivers the packets it fills;
// tests/cpp/test_host_core.cpp drives the same code on the CPU.
// The timed calls share one path: three pending lists under one discipline (frame check, merge by frame, shift and
// pop), one walk over the times of a launch for span() and fold_segments(), the launch's coefficient records in
// SegRecords and the records kept for the next scatter in KeptRecords.  tests/cpp/dump_packets.cpp pins its packets.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/olfx.h"
#include "olfx_layout.h"

namespace olfx {
namespace host __attribute__((visibility("hidden"))) {

// ---- components and kinds (the table is in olfx_host.cpp) ----
// A component is the unit that has parameters, defaults, a setter restatement and a coefficient block.
enum Comp : uint8_t { CP_PLATE, CP_CHORUS, CP_PITCH, CP_VOICE, CP_RACK, CP_SAMPLE, CP_ORDER, CP_METER, CP_COUNT };
// The engine's coefficient arrays (olfx_engine.cpp gives each its pointer and stride).
enum Dst : uint8_t { TO_DT, TO_CH, TO_PS, TO_VC, TO_FR, TO_SM, TO_ORD, TO_MT, TO_COUNT };
// A component of a kind: where its parameters start in the kind's fields, where its coefficients go.
struct Part { Comp comp; uint8_t field0; Dst dst; };
constexpr uint32_t kNoField = 0xFFFFFFFFu;
struct KindDesc {
    uint32_t nparts = 0;                         // 0: not a kind
    Part parts[3] = {};                          // in record order
    // what the parts add up to: the kind's fields and record words; a plate part's pre-delay field and a
    // rack part's topology field (kNoField: no such part); a voice part's fields; whether there is a Sample
    uint32_t n_params = 0, words = 0, pre_field = kNoField, topo_field = kNoField, voice0 = 0, voice_end = 0;
    bool has_sample = false;
    // a kit of voices that each have their own fields (the drum kit): `vparts` repeat voice_slots times in the
    // fields, slot p's at vparts[].field0 + p * OLFX_VC_NPARAMS, and make one coefficient record of `vwords`
    // words per voice slot, delivered apart from the kind's own record (`parts`).  0: no such voices
    uint32_t voice_slots = 0, nvparts = 0, vwords = 0;
    Part vparts[2] = {};
    uint32_t nset = 0;
    struct { uint8_t field; float value; } set[5] = {};   // defaults that differ from the parts' own
    uint8_t in_ch = 2, out_ch = 2;
    enum : uint8_t { EFFECTS, VOICES, INSTRUMENTS } instances = EFFECTS;   // INSTRUMENTS: of several voices each
    bool moog = false;                           // the voice's filter: MoogFilter (VCS_N_MOOG state slots) or Svf
    uint8_t topologies = 0;                      // bit t: the rack part accepts OLFX_FR_TOPOLOGY t
    const char *topology_msg = nullptr;          // why not, otherwise
    double bytes_per_frame = 0.0, read_bytes_per_frame = 0.0;
    const char *kernel = nullptr;                // null: the standalone reverb's, which follows its pre-delays
    bool planes_32bit = false;                   // the kernel addresses the audio planes with 32-bit offsets
    bool pad_plate = false;                      // the plate runs n rounded up to 64 instances
    bool state_counts_padding = false;           // ... and state_bytes counts them (the chain's figure does not)
    bool no_controls = false;                    // no control maps to the kind: olfx_control_map and olfx_control refuse it
    bool reset_keeps_params = false;             // the parameters are configuration: olfx_reset clears the state alone

    bool takes_note_events() const { return instances != EFFECTS; }
};
const KindDesc &kind_desc(int kind);             // an empty row (nparts = 0) for a number that is no kind

// ---- per-kind figures, read from the table ----
uint32_t n_params_of(int kind);              // 0: unknown kind
uint32_t in_channels(int kind);
uint32_t out_channels(int kind);
void default_params(int kind, float *p);     // the reference's defaults of the user-facing parameters
void chorus_sizes(float sr, uint32_t *psize, uint32_t *csize);
// The chorus kind's history: the frames of pitch-shifter output its tap can reach (the chorus's
// largest delay + 2), and the depth of its x ring, which holds that history's own pitch windows too
// (chorus_stage_rf.h).  The pitch-shift kind and the chain keep chorus_sizes' psize.
uint32_t chorus_history(float sr);
uint32_t chorus_x_size(float sr);
uint64_t state_bytes(int kind, uint32_t n, float sr);      // the synth kinds: the 4-voice figure
// kinds that take note events (the voices, and the synth through its Polyvoice router)
bool takes_note_events(int kind);
constexpr uint32_t kSynthDefaultVoices = 4, kSynthMaxVoices = 8;
double algorithmic_bytes_per_frame(int kind);
double algorithmic_read_bytes_per_frame(int kind);

// ---- the reference setters: parameters [OLFX_*] -> coefficient words [*C_*] ----
float core_scale(float in, float inlow, float inhigh, float outlow, float outhigh, float power);
uint32_t dattorro_predelay_samples(float v);
void derive_dattorro(const float *p, uint32_t *c);
void derive_chorus(const float *p, double sr, uint32_t *c);
void derive_pitchshift(const float *p, double sr, uint32_t *c);
void derive_fxrack(const float *p, float sr, uint32_t *c);
void derive_voice(const float *p, bool configured, bool moog, float sr, uint32_t *c);
void derive_meter(const float *p, float sr, uint32_t *c);

// An instance's coefficient record: the words of each destination array (field-major on the
// device, CoefScatterArgs), in record order.
struct Segments {
    uint32_t nseg, words[3];
    uint32_t total() const { return words[0] + words[1] + words[2]; }
};
Segments coef_segments(int kind);
Segments voice_segments(int kind);           // a kit kind's record per voice slot (KindDesc::vparts); else none

// ---- the control packet (u32 words, 16-B aligned sections) ----
// instance list (absent when every instance changed: dense) | coefficient records [W][m] | event
// slots [groups][kVevCap] and the overflow list, 8-B records (write_events); with timed events, n_seg >= 2
// segments: slots [n_seg][groups][kVevCap] | one overflow list | the segments' start frames [n_seg]
// (olfx_layout.h kSegCap)
// timed parameters (n_tc >= 1 coefficient records in the launch's segments), after the start frames: the base
// table [n_seg][groups] (the launch-wide number of a 64-voice group's first record of a segment) | the records,
// field-major [VCC_N][n_tc], segment by segment and by voice index inside a segment
// timed instrument parameters (the synths and the drum kit; n_iv + n_if >= 1 records in the launch's segments),
// after the start frames, 16-B aligned: the voice table [n_seg][gv] and the rack table [n_seg][gf], four words an
// entry {lane mask low, lane mask high, base, 0} -- the 64 lanes of a group that have a record in the segment and
// the launch-wide number of the first of them, so a lane's record is base + its rank among the mask's lower bits |
// the voice records, field-major [VCC_N][n_iv] | the rack records, field-major [TIF_N][n_if] (olfx_layout.h TIF_*:
// the six words the F role reads).  A synth's group is 64 instruments (gv = gf = npad / 64): its voice record is
// the instrument's and reaches all its voices.  A kit's voice record is a voice slot's: group p (npad / 64) + g,
// lane = kit (gv = voices npad / 64); its rack record is the kit's.  An instrument changed at a time has a voice
// record, a rack record or both there; records run segment by segment and by lane inside a segment.
struct PacketPlan {
    bool dense;
    size_t o_inst, o_val, o_ev, words;
    size_t n_seg = 1, o_seg = 0;          // o_seg: the start frames (n_seg >= 2)
    size_t n_tc = 0, o_tcb = 0, o_tc = 0; // timed coefficient records: the base table, the records
    // a kit kind's second section, ahead of the events: the m2 changed voice slots (device slots p * npad + kit,
    // always listed) and their records [W2][m2]
    size_t m2 = 0, o_inst2 = 0, o_val2 = 0;
    // timed instrument records: the voice and rack tables, the voice and rack records
    size_t n_iv = 0, n_if = 0, gv = 0, gf = 0, o_ivt = 0, o_ift = 0, o_iv = 0, o_if = 0;
};
// n instances of which m changed, W words per record, `evs`: an event section with n_more
// overflow records for n_ev voice slots (0: the n instances are the voices)
// n_seg: the event section's segments (timed events)
// n_tc: the launch's timed coefficient records (olfx_timed_params; 0: no such section)
// n_iv, n_if: the launch's timed instrument records (voice, rack) over tables of gv and gf groups a segment
PacketPlan plan_packet(uint32_t n, size_t m, uint32_t W, bool evs, uint32_t n_more, uint32_t n_ev = 0, size_t m2 = 0,
                       uint32_t W2 = 0, uint32_t n_seg = 1, size_t n_tc = 0, size_t n_iv = 0, size_t n_if = 0,
                       uint32_t gv = 0, uint32_t gf = 0);
// The largest packet an engine can produce: every instance's coefficients and, for voices, an
// event for every voice (plan_packet's layout, rounded up); n_ev as above (the synth's voice slots).  A kit
// kind: every kit's record, every voice slot's record and an event per voice.  n_seg: the segments of a
// launch (timed events: the voice kinds' kSegCap, max_segments) -- an event for every voice in each.
size_t max_packet_words(int kind, uint32_t n, uint32_t n_ev = 0, uint32_t n_seg = 1);
// What the timed-parameter section adds to the largest packet (olfx_timed_params: the voice kinds, else 0): a
// launch carries at most n coefficient records over all its segments (Shadow::span), so the worst packet grows
// by one full voice-coefficient upload and the base table, not by kSegCap uploads.
size_t max_timed_param_words(int kind, uint32_t n);
// The same for olfx_timed_instrument_params (the synths and the drum kit, else 0): both tables of a full launch and
// timed_instrument_cap voice records and as many rack records.  An engine sizes its packet slots by the sum of both.
size_t max_timed_instrument_words(int kind, uint32_t n, uint32_t voices);
// the raw records one launch takes (Shadow::span): n, a kit voices x n -- what one time can change at the most
uint32_t timed_instrument_cap(int kind, uint32_t n, uint32_t voices);
// the segments one launch of a kind can take: kSegCap for the kinds olfx_timed_events accepts, else 1
uint32_t max_segments(int kind);
// ... for the kinds olfx_timed_notes accepts (the synths and the drum kit): kSegCap, else 1.  An engine's packet
// slots are sized by the larger of the two
uint32_t max_note_segments(int kind);

struct Folded { uint32_t inst, op, freq, pad; };
// A pending olfx_timed_instrument_params / olfx_timed_instrument_control record, held raw: a control is mapped when
// the engine reaches its frame (the topology and the kit's channel2voice in force there)
struct TimedInst {
    uint32_t frame;
    bool ctl;
    olfx_timed_param p;                   // !ctl
    olfx_control_event ev;                // ctl
};

// A launch's timed coefficient records of W words each, segment by segment: segment s is records first[s] ..
// first[s + 1], ascending by lane inside a segment; words [records][W].
template <uint32_t W>
struct SegRecords {
    std::vector<uint32_t> lane, first, words;
    void clear() { lane.clear(); first.clear(); words.clear(); }
    void open() { clear(); first.assign(2, 0u); }                     // segment 0 (frame 0) has none
    uint32_t *add(uint32_t lane_) {
        lane.push_back(lane_);
        words.resize(words.size() + W);
        return words.data() + words.size() - W;
    }
    void close_segment() { first.push_back((uint32_t)lane.size()); }
    size_t size() const { return lane.size(); }
    void write_field_major(uint32_t *dst) const {                     // [W][records]
        const size_t T = lane.size();
        const uint32_t *src = words.data();
        for (size_t r = 0; r < T; ++r)
            for (uint32_t w = 0; w < W; ++w) dst[(size_t)w * T + r] = src[r * W + w];
    }
};

// Records kept by index (a voice, an instrument, a kit's voice slot): of[i] = the first word of i's record in
// `words`, or -1; `list`: the indices that have one.  Empty, it costs its users one test.
struct KeptRecords {
    uint32_t W = 0;
    std::vector<int32_t> of;
    std::vector<uint32_t> words, list;
    void init(size_t count, uint32_t W_) { W = W_; of.assign(count, -1); words.clear(); list.clear(); }
    const uint32_t *find(uint32_t i) const { return !list.empty() && of[i] >= 0 ? words.data() + of[i] : nullptr; }
    void forget(uint32_t i) { if (!list.empty()) of[i] = -1; }
    void forget_all() {
        for (const uint32_t i : list) of[i] = -1;
        list.clear();
        words.clear();
    }
    // records [list_.size()][W] in order: the last record of an index stays
    void keep(const std::vector<uint32_t> &list_, const std::vector<uint32_t> &words_) {
        list = list_;
        words = words_;
        for (size_t r = 0; r < list.size(); ++r) of[list[r]] = (int32_t)(r * W);
    }
};

// ---- sample voices: the bank's layout and each voice's Sample (olfx_sample_bank / olfx_sample_voices) ----
// A validated bank: where each sample goes in the device allocation (kSmAlign-aligned starts, a
// padded tail) and its frames.  n_samples = 0: no bank (floats = 0).
struct BankPlan {
    std::vector<uint32_t> base, len;      // [n_samples], floats / frames
    uint64_t floats = 0;                  // the allocation, padding included
};
struct SampleAsg {
    uint32_t sample = OLFX_NO_SAMPLE, mode = OLFX_SAMPLE_ONESHOT;
    uint64_t loop_start = 0, loop_end = 0;
    uint32_t gen = 1;                     // bumped whenever the voice gets a fresh Sample object
};

// Which kernel the chorus kind runs (chorus_stage_rf.h).  The ring-free kernel recomputes the
// pitch-shifter's past output from the x ring under the CURRENT pitch and window coefficients, so it
// may run only while those have been in force for every instance over the whole history; after a
// change the engine fills the chorus ring from the x ring under the old coefficients (materialise)
// and runs the ring kernel until `depth` frames have passed.  A change before the first frame since
// create / reset does not count: all history is zero then, and psv of zeros is +0 under any coefficients.
struct RingFree {
    uint32_t depth = 0;                   // chorus_history
    uint64_t seen = 0;                    // frames since create / reset
    uint64_t quiet = 0;                   // frames since the last change, saturating at depth
    void reset() { seen = 0; quiet = depth; }
    bool active() const { return quiet >= depth; }
    // a pitch or window word changed ahead of the next block: whether the chorus ring must be
    // materialised first (it is already current while the ring kernel runs)
    bool changed() {
        if (!seen) return false;
        const bool materialise = active();
        quiet = 0;
        return materialise;
    }
    void advance(uint32_t n_frames) {
        seen += n_frames;
        quiet = quiet + n_frames < depth ? quiet + n_frames : depth;
    }
};

// The host shadow of an engine: what the caller has set, what of it the device has yet to see, and
// the note events queued for the next block.  Every operation that can refuse returns OLFX_OK or
// an OLFX_E_* code with the reason in `msg`, and a refused call changes nothing.
struct Shadow {
    int kind = 0;
    const KindDesc *kd = &kind_desc(0);   // the kind's row, looked up once (init)
    uint32_t n = 0, n_params = 0;
    float sr = 48000.f;
    std::vector<float> params;            // [n_params][n]
    std::vector<uint8_t> configured;      // voice: UpdateConfig seen; a kit kind: per voice slot [voices][n]
    // instances whose coefficients must be re-derived at the next block (each listed once)
    std::vector<uint32_t> dirty_list;
    std::vector<uint8_t> dirty_mark;
    // a kit kind: the voice slots (p * n + kit) whose record must be re-derived; dirty_list holds the kits whose
    // rack or sum order changed
    std::vector<uint32_t> vdirty_list;
    std::vector<uint8_t> vdirty_mark;
    // the kit's VoiceMap (VoiceMap.h:27-58): note2voice [128][n] and channel2voice [16][n], kNoVoice = nobody.
    // Configuration like the bank: reset() keeps it
    static constexpr uint8_t kNoVoice = 0xFF;
    std::vector<uint8_t> note2voice, chan2voice;
    int64_t n_components = 0;             // rack instances with OLFX_FR_TOPOLOGY >= 2
    bool pre_changed = true;              // a reverb pre-delay changed since the flag was last cleared
    std::vector<olfx_voice_event> events; // queued for the next block (its frame 0)
    // The three pending lists: what the timed calls queued past frame 0, each stably ordered by frame in its queueing
    // order (frames count from the next launch's first frame).  An entry at frame 0 never gets here: it is applied
    // at the call, and one that reaches frame 0 in advance() is applied there.
    // `timed`: olfx_timed_events, or olfx_timed_notes' instrument notes, unrouted -- ev.inst is the instrument, and the
    // note is routed through Polyvoice / the VoiceMap when the engine reaches its frame (fold_segments, advance).
    // `tparams`: olfx_timed_params / olfx_timed_control (the voice kinds) in one order for both calls; a control is
    // held as the field and value it maps to (OLFX_FIELD_UPDATE_ONLY: Update() alone).
    // `iparams`: olfx_timed_instrument_params / _control (the synths and the drum kit), raw, in one order for both.
    std::vector<olfx_timed_event> timed;
    std::vector<olfx_timed_param> tparams;
    std::vector<TimedInst> iparams;
    std::vector<olfx_voice_event> routed; // fold_segments: one segment's notes as voice events
    // fold_segments: the launch's timed coefficient records.  `vrec`: the voice records [VCC_N] -- a voice kind's lane
    // is the voice, a synth's the instrument (the record reaches all its voices), a kit's the device voice slot
    // p * npad + kit.  `frec`: an instrument's rack records [TIF_N], lane = instrument.  Both empty without a fold
    // that had records.
    SegRecords<VCC_N> vrec;
    SegRecords<TIF_N> frec;
    // ... the dirty records as frame 0 has them, derived before the fold applied anything ([m][words] and, a kit's
    // voice slots, [m2][vwords], in fill_records' order; valid for the fold's own fill_records)
    std::vector<uint32_t> pre_words, pre_vwords;
    bool pre_valid = false;
    // ... and whether the fold made records that fill_records has yet to put back on the dirty lists: what a launch's
    // records change stays dirty, so its last record reaches the device arrays ahead of the next launch
    bool fold_fresh = false;
    // The last timed record of what the previous launch changed, so that the scatter ahead of the next launch derives
    // nothing twice: a voice kind's voice words per voice, an instrument's whole record, a kit voice slot's whole
    // record (hv = p * n + kit).  mark_dirty / mark_vdirty forget an entry, fill_records retires them all once they
    // have served and keeps the fresh fold's.
    KeptRecords kept_voice, kept_inst, kept_slot;
    // an instrument fold's scratch: the lanes one time touches; each rack record's whole FRC_N words; an instrument's
    // (a kit: voice slot hv's) latest voice record and an instrument's latest rack record (-1: none; all -1 between
    // folds); and what the records changed -- the instruments and (a kit) the voice slots hv, each once, with the
    // whole record of each as the launch's last time leaves it ([.][kd->words], [.][kd->vwords])
    std::vector<uint32_t> at_v, at_f, rack_full;
    std::vector<int32_t> last_v, last_f;
    std::vector<uint32_t> changed_inst, changed_inst_words, changed_slot, changed_slot_words;
    // fold_events / fold_segments: one record per voice and segment, segment by segment and by first
    // appearance; segment s is folded[seg_first[s] .. seg_first[s + 1]) and starts at frame seg_frame[s]
    std::vector<Folded> folded;
    std::vector<uint32_t> seg_frame, seg_first;
    // per segment and workgroup ([n_seg][groups]): records, first overflow record (crowded groups), records
    // written so far
    std::vector<uint32_t> ev_count, ev_more, ev_fill;
    uint32_t n_more = 0;                  // overflow records, all segments
    std::vector<int32_t> ev_slot;         // voice -> its record in `folded` during fold_events, else -1
    std::vector<uint32_t> h_words;        // scratch for a record
    // sample voices: the bank in use and every voice's Sample.  Configuration like the voice buses:
    // reset() keeps both (and makes every Sample fresh)
    BankPlan bank;
    std::vector<SampleAsg> samples;       // [n]
    // the synth: voices per instrument, n rounded up to 64, and every voice's Playing() ([voices][n]:
    // the last NoteOn's note, 0 after NoteOff; SynthVoice.h:245-260).  Voice p of instrument i is voice
    // slot p * npad + i of the event queue (SynthArgs, olfx_internal.h)
    uint32_t voices = 0, npad = 0;
    std::vector<uint8_t> playing;
    // the chorus kind: its kernel switch, the pitch and window words each instance's device coefficients
    // hold ([4][n]: what fill_records last delivered), and whether the packet just filled asks for the
    // chorus ring to be materialised ahead of its scatter (the engine clears it)
    RingFree rf;
    std::vector<uint32_t> pitch_sent;
    bool rf_materialise = false;
    char msg[160] = "";

    void init(int kind_, uint32_t n_, float sr_, uint32_t voices_ = kSynthDefaultVoices) {
        kind = kind_; n = n_; sr = sr_; kd = &kind_desc(kind_); n_params = kd->n_params;
        rf.depth = kind_ == OLFX_KIND_CHORUS ? chorus_history(sr_) : 0u;
        voices = instruments() ? voices_ : 0u;
        npad = instruments() ? (n_ + 63u) & ~63u : 0u;
        samples.assign(kd->has_sample ? n_voices() : 0u, SampleAsg{});
        note2voice.assign(kit() ? (size_t)128 * n_ : 0u, kNoVoice);
        chan2voice.assign(kit() ? (size_t)16 * n_ : 0u, kNoVoice);
    }
    bool kit() const { return kd->voice_slots != 0; }
    // the voices olfx_sample_voices addresses: the instances themselves, or a kit's (kit * voices + p)
    uint32_t n_voices() const { return kit() ? n * voices : n; }
    bool instruments() const { return kd->instances == KindDesc::INSTRUMENTS; }
    // the voice slots that note events address: the instances themselves, or the synth's voices
    uint32_t n_ev() const { return instruments() ? voices * npad : n; }
    // Every instance at the reference's defaults, unconfigured, all dirty; nothing queued.
    void reset();

    int set_range(uint32_t first, uint32_t count, uint32_t field0, uint32_t n_fields, const float *values);
    int set_list(uint32_t field, const uint32_t *inst, const float *values, uint32_t count);
    int set_member(uint32_t inst, uint32_t field, float value);
    int update(uint32_t first, uint32_t count);
    int control(const olfx_control_event *ev, uint32_t count);       // rack topology routing included
    int note_events(const olfx_event *ev, uint32_t count);
    int voice_events(const olfx_voice_event *ev, uint32_t count);
    int timed_events(const olfx_timed_event *ev, uint32_t count);
    int timed_notes(const olfx_timed_note *ev, uint32_t count);
    int timed_params(const olfx_timed_param *rec, uint32_t count);
    int timed_control(const struct olfx_timed_control *rec, uint32_t count);
    // the synths and the drum kit: records held raw, applied (and a control mapped) at their frame
    int timed_instrument_params(const olfx_timed_param *rec, uint32_t count);
    int timed_instrument_control(const struct olfx_timed_control *rec, uint32_t count);
    // The frames of the next launch of a block of n_frames: all of them, unless more than kSegCap distinct
    // times lie in it (frame 0 included, with or without events; a time is an event's or a timed parameter
    // record's) -- then up to the first time that does not fit.  Timed parameters bound the launch a second
    // way: its coefficient records (one per voice changed at a time) number at most n, so the launch ends
    // before the time whose records would exceed that; one time alone always fits.
    // Timed instrument records count as times too, and bound the launch twice more: it ends before a time that
    // holds a boundary record (is_boundary), which so lands at the next launch's frame 0, and before the time whose
    // raw records would make more than timed_instrument_cap of them (a time's own count at most the cap).
    uint32_t span(uint32_t n_frames) const;
    // a pending instrument record that the D role's launch-constant geometry rules out inside a launch: a write to
    // the delay fields or the topology, or a control that can map to one (CCs 35-39 to the rack)
    bool is_boundary(const TimedInst &r) const;
    // whether a launch of `span` frames has events
    bool has_events(uint32_t span_) const {
        return !events.empty() || (!timed.empty() && timed.front().frame < span_) || has_timed_params(span_) ||
               has_timed_inst(span_);
    }
    bool has_timed_inst(uint32_t span_) const { return !iparams.empty() && iparams.front().frame < span_; }
    // ... has timed parameter records (they are past frame 0: the launch is segmented)
    bool has_timed_params(uint32_t span_) const { return !tparams.empty() && tparams.front().frame < span_; }
    // After a launch of `span` frames: the pending events' frames count from the next launch (an event at
    // frame `span` is at its frame 0).  fold_segments(span) has taken the events below `span`.  An instrument
    // note that reaches frame 0 is routed here, ahead of anything queued from now on.
    void advance(uint32_t span_);
    int synth_playing(uint32_t inst, uint8_t *out);                  // [voices]
    // olfx_drumkit_map: VoiceMap::SetVoice records in order, judged on the state after the last
    int drumkit_map(const olfx_drumkit_voice *recs, uint32_t count);
    // a kit's sum order (DKC_ORDER): its mapped voices by ascending note, four bits each
    uint32_t order_word(uint32_t kit_) const;
    // the record of voice slot hv = p * n + kit: its coefficients from its own fields, then its Sample
    void derive_voice_record(uint32_t hv, uint32_t *w) const;
    bool uniform_predelay() const;        // reverb: every instance has the same pre-delay in samples
    // olfx_sample_bank in two steps, so that the engine can allocate and copy in between: the layout of
    // a valid bank (nothing changes), then the switch to it (every Sample fresh; assignments whose index
    // the new bank lacks become unassigned)
    int bank_plan(uint32_t n_samples, const uint64_t *offsets, const float *pcm, BankPlan *plan);
    void bank_commit(BankPlan &&plan);
    int sample_voices(const olfx_sample_voice *recs, uint32_t count);
    // voice i's Sample as the kernel reads it (SMC_* words)
    void sample_record(uint32_t i, uint32_t *w) const;

    // The coefficient record of instance i from its current parameters, in coef_segments' order.
    void derive_record(uint32_t i, uint32_t *w) const;
    // The queued events as one record per voice (`folded`) and their place in the event section.
    void fold_events();
    // The same for a launch of `span` frames: segment 0 is the frame-0 queue (it may be empty), then one
    // segment per distinct frame of the timed events below `span`, which leave the pending list.  Instrument
    // notes are routed here, frame by frame in (frame, queueing order), against Playing() as the earlier frames
    // left it and the VoiceMap in force now; a segment whose notes were all dropped is an empty segment.
    // The pending records below `span` (tparams, or iparams) are times too: each time's records land on the shadow
    // ahead of its events and make that segment's coefficient records (vrec, frec).
    void fold_segments(uint32_t span_);
    uint32_t n_seg() const { return (uint32_t)seg_frame.size(); }
    // the launch's chunks (VoiceArgs::n_chunks): each segment's frames in chunks of `chunk`
    uint32_t n_chunks(uint32_t span_, uint32_t chunk) const;
    PacketPlan plan(bool evs) const {
        const size_t nv = evs ? vrec.size() : 0u;         // a voice kind's section, or an instrument kind's
        return plan_packet(n, dirty_list.size(), kd->words, evs, n_more, n_ev(), vdirty_list.size(), kd->vwords,
                           evs ? n_seg() : 1u, instruments() ? 0u : nv, instruments() ? nv : 0u,
                           evs ? frec.size() : 0u, kit() ? voices * (npad >> 6) : npad >> 6, npad >> 6);
    }
    // The plan's instance list and field-major records into `buf`; clears the dirty lists, retires the kept
    // records, and puts what a fold's records changed back on the lists with its last record kept.
    void fill_records(const PacketPlan &pl, uint32_t *buf);
    // The chorus kind: whether the next block runs the ring-free kernel -- the switch's state unless a
    // dirty instance's pitch or window words differ from the delivered ones (the words, not the call:
    // setting the same value is no change)
    bool ring_free_next() const;
    // The folded records into the event section `fix` (buf + o_ev).
    void write_events(uint32_t *fix);
    // The timed coefficient section (pl.n_tc >= 1): the base table and the records into `buf`.
    void write_timed_coefs(const PacketPlan &pl, uint32_t *buf) const;
    // The timed instrument section (pl.n_iv + pl.n_if >= 1): both tables and both record arrays into `buf`.
    void write_timed_inst(const PacketPlan &pl, uint32_t *buf) const;

private:
    int fail(int code, const char *fmt, ...) __attribute__((format(printf, 3, 4)));
    const char *bad_value(uint32_t field, float v) const;
    void store_param(uint32_t field, uint32_t inst, float v);
    void mark_dirty(uint32_t first, uint32_t count);
    void mark_vdirty(uint32_t hv);
    // a write to fields [field0, field0 + n_fields) of instance inst: Update() of the voices it touches (a kit
    // kind: exactly those voice slots), and what must be re-derived
    void touched(uint32_t inst, uint32_t field0, uint32_t n_fields);
    // the kit's VoiceMap router (VoiceMap.h:27-43): a note event -> the event of the voice at that note
    void route_kit(std::vector<olfx_voice_event> &to, uint32_t inst, uint8_t type, uint8_t note, uint8_t velocity);
    // the synth's Polyvoice router (Polyvoice.h:35-77): one instrument event -> per-voice events
    void route_synth(std::vector<olfx_voice_event> &to, uint32_t inst, uint8_t type, uint8_t note, uint8_t velocity);
    // either, by the kind
    void route_note(std::vector<olfx_voice_event> &to, const olfx_voice_event &ev) {
        if (kit()) route_kit(to, ev.inst, ev.type, ev.note, ev.velocity);
        else route_synth(to, ev.inst, ev.type, ev.note, ev.velocity);
    }
    // a timed call's frame check: OLFX_OK, or the refusal of entry k (`what`: "event" or "record") of `call`
    int bad_frame(const char *call, const char *what, uint32_t k, uint32_t frame);
    // one segment's events onto `folded`, ev_count and ev_more; `coef`: the voices whose coefficients change at the
    // segment's start (VEV_COEF, alone or with the voice's events)
    void fold_one(const olfx_voice_event *ev, size_t count, size_t stride, const uint32_t *coef = nullptr, size_t n_coef = 0);
    // one validated parameter record on params / configured, as olfx_set_param (or, OLFX_FIELD_UPDATE_ONLY,
    // Update()) of that voice; `mark`: onto the dirty list as well
    void apply_param(const olfx_timed_param &r, bool mark);
    int queue_params(const olfx_timed_param *rec, size_t count);
    // validated instrument records: frame 0 now (set_range / control), the rest onto iparams
    void queue_inst(const std::vector<TimedInst> &recs);
    void apply_inst_now(const TimedInst &r);
    // fold_segments: one record on params / configured at its frame without touching the dirty lists; what needs a
    // voice or rack record at this time onto at_v / at_f, the instruments and kit voice slots it touched onto
    // changed_inst / changed_slot
    void apply_quiet(const olfx_timed_param &r);
    void apply_quiet(const TimedInst &r);
    void write_quiet(uint32_t inst, uint32_t field, float v);
    // fold_segments over the pending records of the kind (tparams or iparams)
    template <class R> void fold_with(std::vector<R> &pending, uint32_t span_);
    // ... its tail for the instrument kinds: changed_inst / changed_slot, each once, with their whole last records
    void keep_last_records();
    // fields [field0, field0 + n_fields) include a SynthVoice member (set_params implies Update())
    bool touches_voice(uint32_t field0, uint32_t n_fields) const {
        return kd->instances == KindDesc::VOICES || (n_fields && field0 < kd->voice_end && field0 + n_fields > kd->voice0);
    }
};

}  // namespace host
}  // namespace olfx
