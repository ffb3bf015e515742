// ol_dsp_amd/csrc/olfx_layout.h -- the layout that the host and the kernels of libolfx.so share:
// ring geometry, the coefficient / state word indices of every kind, and the note-event record
// format.  Plain C++ (no HIP header): olfx_internal.h includes it for the kernels, olfx_host.h for
// the host's control logic.
#pragma once
#include <stdint.h>

#include "../../include/olfx.h"

namespace olfx {

// ----------------------------------------------------------------------------------------------
// Dattorro plate: 13 power-of-two rings (reference libs/dattorro-verb/verb.cpp:65-98,173-212).
// ----------------------------------------------------------------------------------------------
enum DtLine {
    DT_PRE = 0, DT_IN0, DT_IN1, DT_IN2, DT_IN3,
    DT_AP1A, DT_DL1A, DT_AP2A, DT_DL2A,
    DT_AP1B, DT_DL1B, DT_AP2B, DT_DL2B,
    DT_NLINES
};
// nominal (TAP_MAIN) delay of each line
constexpr uint32_t kDtDelay[DT_NLINES] = {4800, 142, 107, 379, 277, 672, 4453, 1800, 3720,
                                          908, 4217, 2656, 3163};
// ring size = 2^(bit length of delay)
constexpr uint32_t dt_ring_size(uint32_t d) {
    uint32_t b = 0;
    while (d) { ++b; d >>= 1; }
    return 1u << b;
}
constexpr uint32_t kDtSize[DT_NLINES] = {
    dt_ring_size(4800), dt_ring_size(142), dt_ring_size(107), dt_ring_size(379),
    dt_ring_size(277), dt_ring_size(672), dt_ring_size(4453), dt_ring_size(1800),
    dt_ring_size(3720), dt_ring_size(908), dt_ring_size(4217), dt_ring_size(2656),
    dt_ring_size(3163)};
constexpr uint32_t dt_total_floats() {
    uint32_t s = 0;
    for (int l = 0; l < DT_NLINES; ++l) s += kDtSize[l];
    return s;
}
static_assert(dt_total_floats() == 42368, "dattorro ring geometry");

// Output tap delays (verb.cpp:187-212) and the stereo tap sums (verb.cpp:302-325).
// Left  = +DL1B.o1 +DL1B.o2 -AP2B.o2 +DL2B.o2 -DL1A.o3 -AP2A.o1 +DL2A.o1
// Right = +DL1A.o1 +DL1A.o2 -AP2A.o2 +DL2A.o2 -DL1B.o3 -AP2B.o1 +DL2B.o1
constexpr uint32_t kDl1A_o1 = 353, kDl1A_o2 = 3627, kDl1A_o3 = 1990;
constexpr uint32_t kAp2A_o1 = 187, kAp2A_o2 = 1228;
constexpr uint32_t kDl2A_o1 = 1066, kDl2A_o2 = 2673;
constexpr uint32_t kDl1B_o1 = 266, kDl1B_o2 = 2974, kDl1B_o3 = 2111;
constexpr uint32_t kAp2B_o1 = 335, kAp2B_o2 = 1913;
constexpr uint32_t kDl2B_o1 = 121, kDl2B_o2 = 1996;

// Derived per-instance coefficients (field-major [DTC_N][n] on the device).
// DTC_PREDELAY holds the per-instance pre-delay in samples (an integer 0..4800, exact in fp32).
enum { DTC_PREFILTER = 0, DTC_IN1, DTC_IN2, DTC_DD1, DTC_DAMPING, DTC_DECAY, DTC_DD2, DTC_PREDELAY, DTC_N };
// Per-instance recursive scalar state ([DTS_N][n]).
enum { DTS_LP_PRE = 0, DTS_LP_DAMP_A, DTS_LP_DAMP_B, DTS_N };
// Standalone reverb: the network for these pre-delays (dattorro.hip): v4 with the pre-delay ring
// position-major, v5 with it in rows ([8192/16][n][16])
enum { DT_NET_V4 = 0, DT_NET_V5 };

// ----------------------------------------------------------------------------------------------
// Chorus / pitch-shift (spec: DESIGN.md section 3, from modules/rnbo/patcher/mono-chorus.rnbopat
// and pitchshift.gendsp).  Per-instance rings are instance-major ([n][size]) because the taps are
// modulated per instance: each lane streams through its own ring.
// ----------------------------------------------------------------------------------------------
enum {
    // phasors are 64-bit fixed point (2^64 = one cycle), stored as a high and a low word
    CHC_LFO_INC = 0,    // high word of cycle~'s phase increment
    CHC_LFO_OFF,        // high word of cycle~'s phase offset
    CHC_PS_INC,         // high word of the pitch-shifter phasor's increment
    CHC_DEPTH,          // D = mstosamps(1 + 11 depth): high word of the double
    CHC_WINDOW,         // W = mstosamps(window) in 32.32 fixed point: integer part
    CHC_B0, CHC_B1, CHC_B2, CHC_A1, CHC_A2,   // lores~ (RBJ biquad LP, normalised by a0)
    CHC_MIX, CHC_DRY,   // mix, 1 - mix
    CHC_LFO_INC_LO, CHC_LFO_OFF_LO, CHC_PS_INC_LO,   // low words of the three above
    CHC_DEPTH_LO,       // low word of D
    CHC_WINDOW_LO,      // fraction of W (32.32)
    CHC_N
};
enum {
    CHS_LFO_ACC = 0,    // high word of cycle~'s 64-bit phase
    CHS_PS_ACC,         // high word of the pitch-shifter's 64-bit phase
    CHS_Z1L, CHS_Z2L, CHS_Z1R, CHS_Z2R,   // biquad TDF-II state per channel
    CHS_LFO_LO, CHS_PS_LO,                // low words of the two phases
    CHS_N
};

// ----------------------------------------------------------------------------------------------
// Voice (SynthVoice): registers only.
// ----------------------------------------------------------------------------------------------
enum {
    VCC_ATK_D0A = 0, VCC_ATK_TGT_A, VCC_DEC_D0A, VCC_REL_D0A, VCC_SUS_A,   // amp env
    VCC_ATK_D0F, VCC_ATK_TGT_F, VCC_DEC_D0F, VCC_REL_D0F, VCC_SUS_F,       // filter env
    VCC_AMP_AMT, VCC_CUTOFF, VCC_FENV_AMT,
    VCC_DAMP_RES,       // 2 * (1 - powf(res, 0.25))   (Svf::SetRes, computed on host)
    VCC_DRIVE,          // pre_drive * res
    VCC_PORT_COEF,      // expf(-1/(htime*sr))
    VCC_FC_MAX,         // sr / 3
    VCC_SR,             // sample rate
    VCC_INV_SR,         // Oscillator sr_recip_ = 1/sr
    VCC_N,
    // MoogFilter voices reuse the Svf-only slots for the daisysp::LadderFilter coefficients
    VCC_LADDER_K = VCC_DAMP_RES,      // 4 * clamp(res, 0, 1.8)        (LadderFilter::SetRes)
    VCC_LADDER_DRIVE = VCC_DRIVE,     // input drive_scaled_ (0.5: Init; MoogFilter::SetDrive is a no-op)
    VCC_LADDER_WREC = VCC_FC_MAX      // sr_int_recip_ = 1 / (4 sr)     (4x oversampling)
};
enum {
    VCS_PHASE = 0, VCS_PORT_Z, VCS_ENVA_X, VCS_ENVF_X, VCS_LOW, VCS_BAND, VCS_FREQ,
    VCS_FLAGS,          // bits 0-2 amp mode, 3-5 filt mode, 6 gate(amp prev), 7 gate(filt prev), 8 gate
    VCS_N,
    // MoogFilter voices append the LadderFilter state: z0_[4], z1_[4], oldinput_ (VCS_LOW/BAND unused)
    VCS_LZ0 = VCS_N, VCS_LZ1 = VCS_LZ0 + 4, VCS_LOLD = VCS_LZ1 + 4,
    VCS_N_MOOG
};
inline bool is_voice_kind(int k) {
    return k == OLFX_KIND_VOICE || k == OLFX_KIND_VOICE_MOOG || k == OLFX_KIND_VOICE_SAMPLE;
}
inline bool is_synth_kind(int k) { return k == OLFX_KIND_SYNTH || k == OLFX_KIND_SYNTH_SVF; }
// (a synth's voices: the Moog synth's are MoogFilter voices, the Svf synth's SvfFilter voices)
inline uint32_t voice_state_slots(int k) {
    return k == OLFX_KIND_VOICE_MOOG || k == OLFX_KIND_SYNTH ? (uint32_t)VCS_N_MOOG : (uint32_t)VCS_N;
}

// Note events of one block, folded per voice on the host (olfx_host.cpp fold_events) and applied
// by the voice kernel itself as its first act on the voice's state (SynthVoice.h:231-268: the
// events of a block compose field by field -- the last gate call wins, any NoteOn retriggers, the
// last NoteOn / SetFrequency sets the pitch).
enum : uint32_t {
    VEV_GATE_SET = 1u,          // gate := VEV_GATE_ON bit (NoteOn / GateOn / NoteOff / GateOff)
    VEV_GATE_ON = 2u,
    VEV_RETRIGGER = 4u,         // Adsr::Retrigger(true) on both envelopes: mode ATTACK, x = 0
    VEV_FREQ = 8u,              // freq_ := the record's frequency (mtof(note) for NoteOn, SetFrequency's Hz)
    VEV_SEEK = 0x10u,           // sample voices: Seek(0) (SampleSoundSource::GateOn, any NoteOn / GateOn of the block)
    // timed parameters (segments past the first): the voice's coefficients change at the segment's start; its
    // record is in the packet's timed coefficient section (VoiceArgs::tc).  May be a record's only bit
    VEV_COEF = 0x20u,
    VEV_MORE = 0x80u,           // (slot 0 of a crowded workgroup) its records are in the overflow list
};
// Event records, 8 B: x = (voice & 63) | VEV_* ops << 8, y = frequency bits; x = 0 is an empty slot.
// Workgroup g (64 voices) owns the kVevCap fixed slots ev[g kVevCap ..]: the kernel reads them in
// one host-link round trip without first reading where they are.  A workgroup with more than
// kVevCap records puts them all in the overflow list and marks slot 0:
// x = VEV_MORE << 8 | count << 16, y = first record in ev_more (a second round trip, for it only).
constexpr uint32_t kVevCap = 4;
// Timed events (olfx_timed_events): a launch's frames are up to kSegCap segments, each with fixed slots of
// its own -- [segments][groups][kVevCap], then one overflow list for all of them (a crowded slot 0's y
// counts from its start), then the segments' start frames (u32 each).  One segment is the layout above.
// 16: every quad of a 64-frame block, or the firmware's MIDI rate over a 64-frame host block, in one
// launch; the kernel stages all of a launch's records up front (16 fixed-slot reads in flight over the
// host link, 32 VGPRs before the envelopes are live) into 8 KB of LDS per workgroup, which leaves two
// workgroups per CU to the sample voice (54 KB + 8) as to the others.  A block with more distinct times
// runs as several launches (olfx_engine.cpp), and the worst packet stays kSegCap records per voice.
constexpr uint32_t kSegCap = 16;
// frames per chunk of the voice kernels (voice_roles.h kVcChunk): a segment's frames run in chunks of its own
constexpr uint32_t kVoiceChunk = 8;

// ----------------------------------------------------------------------------------------------
// Sample voices (sampler.hip): SynthVoice(SampleSoundSource<1>(Sample), SvfFilter).  The voice's
// coefficients and state are the Svf voice's; the oscillator's two state words hold the Sample.
// The bank is one device allocation: sample k starts at a multiple of kSmAlign floats and the
// allocation ends with kSmAlign floats of padding (zeros), so a 64-lane fetch that starts inside a
// sample stays inside the allocation.
// ----------------------------------------------------------------------------------------------
constexpr uint32_t kSmAlign = 64;           // floats: the fetch width (one voice's 256 contiguous bytes)
constexpr uint64_t kSmMaxBankFloats = (1ull << 30) - 2 * kSmAlign;   // 32-bit byte offsets into the bank
// A voice's Sample over the bank ([SMC_N][n] words, delivered like the coefficients).
enum {
    SMC_BASE = 0,       // the sample's first frame in the bank, in floats (0 when unassigned)
    SMC_LEN,            // its frames (0: unassigned -- nothing is ever read)
    SMC_LS,             // min(loop_start, len): where Seek(loop_start) puts the data cursor
    SMC_LE,             // loop_end where it can fire (0 < loop_end < len), else 0
    SMC_MODE,           // bit 0: Loop; bits 1..: the generation of this Sample object (a new one = a fresh Sample)
    SMC_N
};
// state words (the oscillator's, unused here): the data cursor; bit 0 playing, bits 1.. the generation seen
enum { VCS_SM_POS = VCS_PHASE, VCS_SM_FLAGS = VCS_PORT_Z };

// ----------------------------------------------------------------------------------------------
// Drum kit (drumkit.hip): P sample voices per kit behind a VoiceMap.  Every voice slot (p * npad + kit,
// like the synths' state planes) has its own coefficients [VCC_N], Sample [SMC_N] and state [VCS_N].
// A kit's sum order is one word ([n]): eight 4-bit voice slots in summing order (VoiceMap::Process: the
// mapped voices by ascending note), lowest nibble first, kDkOrderEnd = end of the list.
// ----------------------------------------------------------------------------------------------
constexpr uint32_t kDkMaxVoices = OLFX_DK_MAX_VOICES;
constexpr uint32_t kDkOrderEnd = 0xFu;
constexpr uint32_t kDkOrderEmpty = 0xFFFFFFFFu;     // a kit with an empty map: nothing is summed
enum { DKC_ORDER = 0, DKC_N };

// ----------------------------------------------------------------------------------------------
// Level meter (meter.hip): ol::core::Rms (corelib/ol_corelib.h:61-85) and the sandbox firmware's peak-hold
// follower (ol_daisy/workouts/sandbox/main.cpp:98-137) per signal; a signal is one channel plane of one
// instance.  State rows [MTS_N][planes * n], signal (plane p, instance i) at p * n + i; coefficients
// [MTC_N][n], shared by an instance's channels: the window Rms::Init resolved, and the hold count.
// ----------------------------------------------------------------------------------------------
enum { MTS_SUM = 0, MTS_COUNT, MTS_RMS, MTS_PEAK, MTS_PEAK_COUNT, MTS_N };
enum { MTC_WINDOW = 0, MTC_HOLD, MTC_N };
inline bool is_meter_kind(int k) { return k == OLFX_KIND_METER || k == OLFX_KIND_METER_MONO; }

// ----------------------------------------------------------------------------------------------
// Effect rack ol::fx::FxRack<2> (fxrack.hip): delay lines + two Svf (channel 0) + ReverbSc stub.
// ----------------------------------------------------------------------------------------------
constexpr uint32_t kFrMaxDelay = 48000;     // MAX_DELAY (modules/fxlib/Fx.h:23): ring positions
enum {
    FRC_DELAY = 0,      // uint: DelayLine delay_ (integer part, clamped to 47999)
    FRC_FRAC,           // DelayLine frac_
    FRC_FEEDBACK, FRC_DBAL,
    FRC_DFREQ, FRC_DDAMP, FRC_DDRIVE,       // DelayFx filter_ Svf (LowPass)
    FRC_RBAL,                               // ReverbFx balance
    FRC_FFREQ, FRC_FDAMP, FRC_FDRIVE,       // FxRack filter1 Svf
    FRC_FTYPE,          // uint: 0 low, 1 band, 2 high, 3 notch, 4 peak
    FRC_MASTER,
    FRC_TOPO,           // uint: OLFX_FR_TOPOLOGY (0..4)
    FRC_N
};
enum { FRS_DLOW = 0, FRS_DBAND, FRS_FLOW, FRS_FBAND, FRS_N };
// A timed rack record of the instrument kernels (olfx_timed_instrument_params): the words the F role reads, in
// FRC order -- word TIF_k is FRC_RBAL + k.  The delay words and the topology are the launch's (the D role).
enum { TIF_RBAL = 0, TIF_FFREQ, TIF_FDAMP, TIF_FDRIVE, TIF_FTYPE, TIF_MASTER, TIF_N };
static_assert(FRC_MASTER - FRC_RBAL + 1 == TIF_N, "the F role's words are consecutive");

}  // namespace olfx
