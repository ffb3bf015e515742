// ol_dsp_amd/csrc/olfx_internal.h -- kernel argument blocks, launchers and the host/device-shared
// scalar DSP helpers of libolfx.so (the ring geometry and the coefficient / state word indices:
// olfx_layout.h).
//
// Everything here is written for gfx950 (CDNA4, wave64) and compiled with -ffp-contract=off so
// that the device arithmetic is the exact IEEE single-precision sequence the CPU oracle uses.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/olfx.h"
#include "olfx_layout.h"

#define OLFX_HD __host__ __device__ __forceinline__

namespace olfx {

// ----------------------------------------------------------------------------------------------
// Dattorro plate (olfx_layout.h: DtLine, kDtDelay, kDtSize, the output taps, DTC_*, DTS_*).
// ----------------------------------------------------------------------------------------------
// Extra delay of both tank input all-passes at stream time t16 (verb.cpp:262-270): their read
// offset is decremented at every t16 = k*2048 < 32768 and incremented at every k*2048 >= 32768,
// *before* the sample at that t is processed.  For an instance created at t = 0 the count is
// closed-form, so every chunk can compute it without carrying the offset.
OLFX_HD uint32_t dt_ap1_extra(uint32_t t16) {
    uint32_t dec = ((t16 >> 11) < 15u ? (t16 >> 11) : 15u) + 1u;
    uint32_t inc = t16 >= 32768u ? ((t16 - 32768u) >> 11) + 1u : 0u;
    return dec - inc;
}

struct DattorroArgs {
    float *ring[DT_NLINES];     // ring l: [kDtSize[l]][n]   (position-major, instance fastest)
    float *state;               // [DTS_N][n]
    const float *coef;          // [DTC_N][n]
    const float *in;            // [2][..][n], channel planes `plane` floats apart
    float *out;                 // [2][..][n]
    uint64_t plane;             // floats between the channel planes of in / out (>= n_frames * n)
    uint32_t n;                 // instances
    uint32_t n_frames;
    uint32_t t0;                // stream time (frames since create) of the first frame, mod 2^16
    uint32_t in_ch;             // 1 or 2
    uint32_t cus;               // compute units of the device (olfx_create)
};
// Standalone reverb: the network (DT_NET_*) for these pre-delays (dattorro.hip)
int dattorro_network(uint32_t n, uint32_t cus, bool uniform);
const char *dattorro_network_name(int net);
// the pre-delay ring's content into the other layout (tmp: a device buffer of the ring's size)
hipError_t launch_dattorro_pre_layout(const DattorroArgs &a, float *tmp, bool to_rows, hipStream_t s);

// ----------------------------------------------------------------------------------------------
// Deterministic cos(2*pi*x): used by the chorus LFO (RNBO cycle~).  Branch-free (selects only, no
// lane divergence): reduce to b in [0, 1/4] exactly, then one minimax polynomial of cos in
// theta^2 on [0, pi/2] (degree 8, Remez, coefficients rounded to float; round 2 used the Taylor
// series to theta^14: the same accuracy class at twice the operations).  Only +, -, *, rint and
// compares in a fixed order, so the host (oracle) and gfx950 produce identical bits under
// -ffp-contract=off.  |err| < 3e-7 (measured 1.8e-7; tests/test_oracle.py).
// ----------------------------------------------------------------------------------------------
// Horner in fused multiply-adds (spec v3, round 6: IEEE fusedMultiplyAdd, C fmaf on the host)
OLFX_HD float cos_poly(float t2) {                 // cos(theta), t2 = theta^2, theta in [0, pi/2]
    float r = __builtin_fmaf(2.31943868129747e-05f, t2, -0.001385592739097774f);
    r = __builtin_fmaf(r, t2, 0.041663989424705505f);
    r = __builtin_fmaf(r, t2, -0.4999993145465851f);
    return __builtin_fmaf(r, t2, 1.0f);
}
OLFX_HD float sin_poly(float th, float t2) {       // sin(theta), theta in [0, pi/2]
    float r = __builtin_fmaf(2.6000548132287804e-06f, t2, -0.00019806614727713168f);
    r = __builtin_fmaf(r, t2, 0.008333017118275166f);
    r = __builtin_fmaf(r, t2, -0.16666656732559204f);
    return th * __builtin_fmaf(r, t2, 1.0f);
}
OLFX_HD float cos2pi(float x) {
    const float u = x - rintf(x);                  // exact, u in [-0.5, 0.5]
    const float a = u < 0.0f ? -u : u;             // cos is even
    const bool hi = a > 0.25f;
    const float b = hi ? 0.5f - a : a;             // exact (Sterbenz); cos(2pi(1/2-b)) = -cos(2pi b)
    const float th = b * 6.28318530717958647692f;
    const float r = cos_poly(th * th);
    return hi ? -r : r;
}
// The pitch-shifter's crossfade windows at phasor phase p in [0, 1) (pitchshift.gendsp: tap 0's
// gain cos((p - 1/2) pi), tap 1's cos((p1 - 1/2) pi) with p1 = (p + 1/2) mod 1) are sin(pi p) and
// |cos(pi p)|, i.e. sin(pi q) and cos(pi q) for q = min(p, 1 - p) in [0, 1/2] (1 - p is exact: p is
// a 24-bit fraction): one argument, two short polynomials.
OLFX_HD void win_gains(float p, float &g0, float &g1) {
    const float q = fminf(p, 1.0f - p);
    const float th = q * 3.14159265358979323846f;
    const float t2 = th * th;
    g0 = sin_poly(th, t2);
    g1 = cos_poly(t2);
}

// ----------------------------------------------------------------------------------------------
// Chorus / pitch-shift (olfx_layout.h: CHC_*, CHS_*).
// ----------------------------------------------------------------------------------------------
// Tap delays (spec v2, round 4).  Round 3 formed both delays in fp32 from the
// phasors' top 24 bits: the pitch delay p W (W up to 480 samples) to 2^-15 sample, the chorus delay
// D cos + D (D up to 576) from a cosine good to 2e-7, i.e. to ~1e-4 sample -- that, not the fp32
// signal arithmetic, was the spec's deviation from double precision (1.3e-4 / 1.6e-4 of the signal,
// tests/test_oracle.py test_chorus_deviation_by_stage).  Now:
//   pitch-shifter: d = p W in 32.32 fixed point, p = the phasor's high word / 2^32 and W in 32.32
//     (exact integer arithmetic), clamped to [1, pmax]; the fraction rounded once to fp32;
//   chorus: the LFO phase to 53 bits, cos(2 pi x) by a double Taylor polynomial (|err| < 4e-15),
//     d = cos D + D in double (D double), clamped to [0, cmax]; the fraction rounded once to fp32.
//     Spec v2.1 (round 4): the polynomial's Horner steps and cos D + D are fused multiply-adds.
// Gains, interpolation, lores~ and the mix stay fp32.  Host and gfx950 evaluate these identically
// (integer ops, IEEE double +, * and fma in a fixed order, no other contraction).
OLFX_HD void pitch_split(uint32_t ph, uint32_t wi, uint32_t wf, uint32_t pmax, uint32_t &di, float &fr) {
    const uint64_t d = (uint64_t)ph * wi + (((uint64_t)ph * wf) >> 32);     // p W, 32.32
    // clamp to [1, pmax] in 32.32 on the two words (the oracle clamps the 64-bit value; the same
    // result): below 1 or at / above pmax the fraction is 0, the integer part the bound
    const uint32_t dh = (uint32_t)(d >> 32);
    const bool inside = dh >= 1u && dh < pmax;
    di = dh < 1u ? 1u : (dh > pmax ? pmax : dh);
    fr = inside ? (float)(uint32_t)d * 2.3283064365386963e-10f : 0.0f;      // 2^-32: exact scaling
}
// r t2 + c as one v_fma_f64 with the constant in an SGPR pair: left to itself the compiler keeps the
// constants in VGPR pairs and emits v_fmac_f64 (destination = addend), i.e. a v_mov_b64 of the
// constant before each step -- 7 extra VALU per cosine, 8 cosines per lane and chunk in the chorus
OLFX_HD double fma_dc(double r, double t2, double c) {
#if defined(__HIP_DEVICE_COMPILE__)
    double d;
    asm("v_fma_f64 %0, %1, %2, %3" : "=v"(d) : "v"(r), "v"(t2), "s"(c));
    return d;
#else
    return __builtin_fma(r, t2, c);
#endif
}
// cos(2 pi x) for the 53-bit phase x = (phase >> 11) 2^-53 (the oracle's oracle_cos2pi_d(x), bit for
// bit), with the reduction u = x - rint(x), |u| <= 1/2, done in integers: u is the phase's high word
// read as SIGNED (u in [-1/2, 1/2); at x = 1/2, u = -1/2 where rint gives +1/2: the same |u|), and
// u = hi 2^-32 + (lo >> 11) 2^-53 is one exact fma (53 significant bits).  Round 5: 5 VALU instead
// of 8 for the conversion and reduction.  Then b = |u| folded into [0, 1/4] (cos(2pi(1/2 - b)) =
// -cos(2pi b)) and cos(th) = sum (-1)^k th^2k / (2k)!, k <= 9 (th = 2 pi b <= pi/2: truncation
// < 4e-15), Horner in th^2 with fused multiply-adds (IEEE fusedMultiplyAdd: C fma on the host,
// v_fma_f64 here -- the same bits; spec v2.1, round 4: half the double operations of the unfused
// Horner).
OLFX_HD double cos2pi_phase(uint64_t phase) {
    const int32_t sh = (int32_t)(uint32_t)(phase >> 32);
    const uint32_t lo = (uint32_t)phase >> 11;
    const double u = __builtin_fma((double)sh, 2.3283064365386963e-10, (double)lo * 1.1102230246251565e-16);
    const double a = __builtin_fabs(u);
    const bool hi = a > 0.25;
    const double b = hi ? 0.5 - a : a;             // exact
    const double th = b * 6.283185307179586;
    const double t2 = th * th;
    double r = -1.5619206968586225e-16;                        // -1 / 18!
    r = fma_dc(r, t2, 4.779477332387385e-14);                  //  1 / 16!
    r = fma_dc(r, t2, -1.1470745597729725e-11);                // -1 / 14!
    r = fma_dc(r, t2, 2.08767569878681e-09);                   //  1 / 12!
    r = fma_dc(r, t2, -2.755731922398589e-07);                 // -1 / 10!
    r = fma_dc(r, t2, 2.48015873015873e-05);                   //  1 / 8!
    r = fma_dc(r, t2, -0.001388888888888889);                  // -1 / 6!
    r = fma_dc(r, t2, 0.041666666666666664);                   //  1 / 4!
    r = __builtin_fma(r, t2, -0.5);
    r = __builtin_fma(r, t2, 1.0);
    return hi ? -r : r;
}
OLFX_HD double chorus_delay(uint64_t phase, double D, double cmax) {
    const double d = __builtin_fma(cos2pi_phase(phase), D, D);
    // clamp to [0, cmax] as min / max (one v_max_f64 + one v_min_f64; the compare-select form cost
    // two compares, four selects and their hazard waits): equal for every non-NaN d, and d is never
    // -0 (cos = -1 gives D - D = +0)
    return __builtin_fmin(__builtin_fmax(d, 0.0), cmax);
}
OLFX_HD void chorus_split(uint64_t phase, double D, double cmax, uint32_t &di, float &fr) {
    const double d = chorus_delay(phase, D, cmax);
    di = (uint32_t)d;
    fr = (float)(d - (double)di);                  // the subtraction is exact
}
// two chorus_splits with their Horner chains interleaved (each step's operand is two instructions
// back: no dependent double-precision pair back to back), the same operations per phase
OLFX_HD void chorus_split2(uint64_t ph0, uint64_t ph1, double D, double cmax, uint32_t &di0, float &fr0,
                           uint32_t &di1, float &fr1) {
    const int32_t s0 = (int32_t)(uint32_t)(ph0 >> 32), s1 = (int32_t)(uint32_t)(ph1 >> 32);
    const uint32_t l0 = (uint32_t)ph0 >> 11, l1 = (uint32_t)ph1 >> 11;
    const double u0 = __builtin_fma((double)s0, 2.3283064365386963e-10, (double)l0 * 1.1102230246251565e-16);
    const double u1 = __builtin_fma((double)s1, 2.3283064365386963e-10, (double)l1 * 1.1102230246251565e-16);
    const double a0 = __builtin_fabs(u0), a1 = __builtin_fabs(u1);
    const bool h0 = a0 > 0.25, h1 = a1 > 0.25;
    const double b0 = h0 ? 0.5 - a0 : a0, b1 = h1 ? 0.5 - a1 : a1;
    const double th0 = b0 * 6.283185307179586, th1 = b1 * 6.283185307179586;
    const double t0 = th0 * th0, t1 = th1 * th1;
    double r0 = -1.5619206968586225e-16, r1 = -1.5619206968586225e-16;
    r0 = fma_dc(r0, t0, 4.779477332387385e-14);    r1 = fma_dc(r1, t1, 4.779477332387385e-14);
    r0 = fma_dc(r0, t0, -1.1470745597729725e-11);  r1 = fma_dc(r1, t1, -1.1470745597729725e-11);
    r0 = fma_dc(r0, t0, 2.08767569878681e-09);     r1 = fma_dc(r1, t1, 2.08767569878681e-09);
    r0 = fma_dc(r0, t0, -2.755731922398589e-07);   r1 = fma_dc(r1, t1, -2.755731922398589e-07);
    r0 = fma_dc(r0, t0, 2.48015873015873e-05);     r1 = fma_dc(r1, t1, 2.48015873015873e-05);
    r0 = fma_dc(r0, t0, -0.001388888888888889);    r1 = fma_dc(r1, t1, -0.001388888888888889);
    r0 = fma_dc(r0, t0, 0.041666666666666664);     r1 = fma_dc(r1, t1, 0.041666666666666664);
    r0 = __builtin_fma(r0, t0, -0.5);              r1 = __builtin_fma(r1, t1, -0.5);
    r0 = __builtin_fma(r0, t0, 1.0);               r1 = __builtin_fma(r1, t1, 1.0);
    const double c0 = h0 ? -r0 : r0, c1 = h1 ? -r1 : r1;
    const double d0 = __builtin_fmin(__builtin_fmax(__builtin_fma(c0, D, D), 0.0), cmax);
    const double d1 = __builtin_fmin(__builtin_fmax(__builtin_fma(c1, D, D), 0.0), cmax);
    di0 = (uint32_t)d0;
    di1 = (uint32_t)d1;
    fr0 = (float)(d0 - (double)di0);
    fr1 = (float)(d1 - (double)di1);
}

struct ChorusArgs {
    float *pitch_ring;          // [n][psize][2]  (stereo-interleaved: L and R share every tap)
    float *chorus_ring;         // [n][csize][2]
    uint32_t *state;            // [CHS_N][n] (floats stored bitwise)
    const uint32_t *coef;       // [CHC_N][n]
    const float *in;            // [2][..][n], channel planes `plane` floats apart
    float *out;                 // [2][..][n]
    uint64_t plane;             // floats between the channel planes of in / out (>= n_frames * n)
    uint32_t n, n_frames;
    uint32_t t0;                // write position of the first frame (mod ring sizes)
    uint32_t psize, csize;      // ring sizes (powers of two)
    uint32_t mode;              // 0 = full chorus, 1 = pitch-shift stage only
    // the pitch delay clamp [1, pmax]: the pitch window's own bound (host::chorus_sizes' psize - 2),
    // whatever the depth of the x ring (the chorus kind's also holds the chorus history)
    uint32_t pmax;
};

// ----------------------------------------------------------------------------------------------
// Voice (SynthVoice): registers only (olfx_layout.h: VCC_*, VCS_*, the VEV_* event records).
// ----------------------------------------------------------------------------------------------
struct VoiceArgs {
    float *state;               // [VCS_N][n], MoogFilter voices [VCS_N_MOOG][n]
    const float *coef;          // [VCC_N][n]
    float *out;                 // [1][n_frames][n]
    uint32_t n, n_frames;
    uint32_t moog;              // 1: daisysp::LadderFilter (MoogFilter) in place of the Svf
    // this block's events (nullptr: none), at most one record per voice (kVevCap above)
    const uint2 *ev;            // [n_groups][kVevCap] fixed slots, n_groups = ceil(n / 64)
    const uint2 *ev_more;       // overflow list
    // sample voices (sampler.hip): each voice's Sample and the bank it plays from
    const uint32_t *smp;        // [SMC_N][n]
    const float *bank;          // bank_bytes bytes (nullptr / 0: no bank -- every SMC_LEN is 0 then)
    uint32_t bank_bytes;
    // timed events (olfx_layout.h kSegCap): n_seg >= 2 segments, segment s starting at frame seg[s]
    // (seg[0] = 0, ascending, multiples of 4 below n_frames) with the fixed slots ev[s n_groups kVevCap ..];
    // n_chunks: the launch's chunks, each segment's frames in chunks of its own (sum of ceil(L / kVcChunk)).
    // n_seg <= 1: one segment, the launch as it was
    uint32_t n_seg, n_chunks;
    const uint32_t *seg;
    // timed parameters (the segmented kernels; nullptr: none): tc_n coefficient records, field-major [VCC_N][tc_n],
    // segment by segment and by voice inside a segment; tc_base[s n_groups + g] = the number of group g's first
    // record of segment s.  A voice has a record in a segment iff its event record there has VEV_COEF; it is
    // record tc_base + (the group's lower voices with VEV_COEF in that segment)
    const uint32_t *tc_base;
    const uint32_t *tc;
    uint32_t tc_n;
};

// Coefficient records of the instances whose parameters changed (olfx_engine.cpp submit_control):
// word w of record r goes to dst[s][(w - first word of segment s) * stride[s] + inst[r]].  Field-
// major records ([w][m]) so consecutive threads write consecutive instances.
struct CoefScatterArgs {
    const uint32_t *inst;       // [m] instance of each record; nullptr = the identity (m == every instance)
    const uint32_t *val;        // [W][m]
    uint32_t m, W;
    uint32_t nseg;
    uint32_t *dst[3];
    uint32_t words[3];          // words of each segment (sum = W)
    uint32_t stride[3];         // instance stride of each segment's field-major array
};
hipError_t launch_coef_scatter(const CoefScatterArgs &a, hipStream_t s);

// ----------------------------------------------------------------------------------------------
// Effect rack ol::fx::FxRack<2> (fxrack.hip; olfx_layout.h: kFrMaxDelay, FRC_*, FRS_*).
// ----------------------------------------------------------------------------------------------
struct FxRackArgs {
    float *ring;                // [n][kFrMaxDelay][2] stereo-interleaved delay lines
    uint32_t *state;            // [FRS_N][n] (floats stored bitwise)
    const uint32_t *coef;       // [FRC_N][n]
    const float *in;            // [2][..][n]
    float *out;                 // [2][..][n]
    uint64_t plane;
    uint32_t n, n_frames;
    uint32_t t0;                // ring position of the first frame: frames since create mod 48000
    uint32_t components;        // some instance is a standalone component (topology 2..4)
};

// Launchers (defined in the .hip files).
hipError_t launch_fxrack(const FxRackArgs &a, hipStream_t s);
// The fused chain (chain.hip): chorus -> pitch-shift -> dattorro in one launch.  c1 / c2 / d
// carry each stage's rings, state and coefficients (their in / out fields are unused); the
// reverb stage's instance count d.n is n rounded up to 64 (padding instances compute harmlessly).
struct ChainArgs {
    ChorusArgs c1, c2;
    DattorroArgs d;
    const float *in;            // [2][..][n]
    float *out;                 // [2][..][n]
    uint64_t plane;             // floats between channel planes of in / out
    uint32_t n, n_frames;       // real instances; frames (multiple of 4)
    uint32_t cus;               // compute units of the device (the persistent grid), from olfx_create
};

// The plate rack (platerack.hip): the rack's delay stage -> dattorro -> balance mix, filter1 and
// master in one launch.  ring / state / coef are the rack's (FxRackArgs); d carries the plate's rings,
// state and coefficients (its in / out fields are unused, d.n is n rounded up to 64, d.t0 the
// plate's own clock).
struct PlateRackArgs {
    float *ring;                // [n][kFrMaxDelay][2]
    uint32_t *state;            // [FRS_N][n]
    const uint32_t *coef;       // [FRC_N][n]
    DattorroArgs d;
    const float *in;            // [2][..][n]
    float *out;                 // [2][..][n]
    uint64_t plane;
    uint32_t n, n_frames;
    uint32_t t0;                // rack ring position of the first frame: frames since create mod 48000
    uint32_t cus;               // compute units of the device (the persistent grid)
};
hipError_t launch_platerack(const PlateRackArgs &a, hipStream_t s);

// What the fused instrument kernels share (synth_pipeline.h): the rack's planes, the voices' planes, the
// output and the block.  Voice p of instrument i is voice slot p * npad + i of the state planes and the event
// slots (npad = n rounded up to 64: a 64-voice group is one voice slot of 64 consecutive instruments).
struct InstrumentArgs {
    float *ring;                // [n][kFrMaxDelay][2]
    uint32_t *fr_state;         // [FRS_N][n]
    const uint32_t *fr_coef;    // [FRC_N][n]
    float *vc_state;            // [..][voices * npad]: synth [VCS_N_MOOG], svf synth and drum kit [VCS_N]
    const float *vc_coef;       // synth: [VCC_N][n]; drum kit: [VCC_N][voices * npad]
    float *out;                 // [2][..][n]
    uint64_t plane;
    uint32_t n, n_frames;       // instruments; frames (multiple of 4)
    uint32_t t0;                // rack ring position of the first frame: frames since create mod 48000
    uint32_t voices, npad;
    const uint2 *ev;            // [voices * npad / 64][kVevCap] fixed slots (nullptr: no events)
    const uint2 *ev_more;
    // timed notes (olfx_timed_notes; olfx_layout.h kSegCap): n_seg >= 2 segments, segment s starting at frame
    // seg[s] (seg[0] = 0, ascending, multiples of 4 below n_frames) with the fixed slots
    // ev[s (voices npad / 64) kVevCap ..] -- the *_seg kernels.  n_seg <= 1: one segment, the launch as it was
    uint32_t n_seg;
    const uint32_t *seg;
};
// what both launches require of a non-empty block
inline bool instrument_args_ok(const InstrumentArgs &a, uint32_t max_voices) {
    return !(a.n_frames & 3u) && !(a.t0 & 1u) && a.t0 < kFrMaxDelay && a.voices >= 1u && a.voices <= max_voices &&
           a.npad == ((a.n + 63u) & ~63u) && a.plane >= (uint64_t)a.n_frames * a.n &&
           (a.n_seg <= 1u || (a.n_seg <= kSegCap && a.seg && a.ev));          // a segmented launch's table is there
}

// Timed instrument parameters (olfx_timed_instrument_params; the *_seg kernels alone take them, in an argument block
// of their own -- the unsegmented kernels' arguments are what they were).  The packet's section (host::PacketPlan):
// vtab [n_seg][gv] and ftab [n_seg][npad / 64], an entry {lane mask low, high, base, 0}: the lanes of a 64-lane
// group that have a record at segment s's start, the first of them record `base`, the others by rank among the
// mask's lower bits.  Voice records vrec, field-major [VCC_N][n_v]: a synth's group is 64 instruments (gv =
// npad / 64; the record reaches every voice of the instrument), a kit's voice slot p's kits (gv = voices npad / 64,
// group p (npad / 64) + g).  Rack records frec, field-major [TIF_N][n_f], lane = instrument.  vtab == nullptr: none.
struct InstrumentTimed {
    const uint4 *vtab;
    const uint4 *ftab;
    const float *vrec;
    const uint32_t *frec;
    uint32_t n_v, n_f, gv;
};

// The synth (synth.hip): `voices` MoogFilter SynthVoices per instrument, their Polyvoice sum, the
// rack's topology 1, in one launch.  The voice coefficients are the instrument's (Polyvoice fans
// every setter out to all its voices).
// svf = 1 (OLFX_KIND_SYNTH_SVF): SvfFilter voices (state planes [VCS_N]) and the rack at each instrument's
// topology, 0 or 1 (FRC_TOPO).
struct SynthArgs : InstrumentArgs {
    uint32_t svf;               // 1: synth_svf_block_v1
};
// what a launch requires of the section: none, or a segmented launch with both tables, the record arrays that have
// records, and the table width of the kind (per_slot: a kit)
inline bool instrument_timed_ok(const InstrumentArgs &a, const InstrumentTimed &t, bool per_slot) {
    if (!t.vtab) return true;
    return a.n_seg > 1u && t.ftab && (!t.n_v || t.vrec) && (!t.n_f || t.frec) &&
           t.gv == (per_slot ? a.voices : 1u) * (a.npad >> 6);
}
struct SynthSegArgs : SynthArgs {
    InstrumentTimed tp;
};
hipError_t launch_synth(const SynthSegArgs &a, hipStream_t s);

// The drum kit (drumkit.hip): `voices` sample voices per kit, their VoiceMap sum in the order the host
// derived from the kit's map (DKC_ORDER), the rack at each kit's topology (0 or 1), in one launch.  A voice
// slot has its own coefficients and Sample planes.
struct DrumkitArgs : InstrumentArgs {
    const uint32_t *smp;        // [SMC_N][voices * npad]
    const uint32_t *order;      // [n]
    const float *bank;          // bank_bytes bytes (nullptr / 0: no bank)
    uint32_t bank_bytes;
};
struct DrumkitSegArgs : DrumkitArgs {
    InstrumentTimed tp;
};
hipError_t launch_drumkit(const DrumkitSegArgs &a, hipStream_t s);

hipError_t launch_dattorro(const DattorroArgs &a, int net, hipStream_t s);
hipError_t launch_chain(const ChainArgs &a, hipStream_t s);
hipError_t launch_chorus(const ChorusArgs &a, hipStream_t s);
// The chorus kind (mode 0) without its chorus ring (chorus_stage_rf.h): valid while every instance's
// pitch and window coefficients have been in force for the whole chorus history (host::RingFree).
hipError_t launch_chorus_ringfree(const ChorusArgs &a, hipStream_t s);
// The last `history` positions of the chorus ring from the x ring, the phasors in a.state and the
// coefficients in a.coef (a.t0 = the next write position): the switch from ring-free to ring mode.
hipError_t launch_chorus_materialise(const ChorusArgs &a, uint32_t history, hipStream_t s);
hipError_t launch_voice(const VoiceArgs &a, hipStream_t s);
hipError_t launch_sampler(const VoiceArgs &a, hipStream_t s);

// ----------------------------------------------------------------------------------------------
// Voice buses (mix.hip): the Polyvoice / VoiceMap sums.  Bus b of frame f = out[f][b] plus the
// voices order[off[b] .. off[b+1]) of in[f][*], added one at a time in that order
// (modules/synthlib/Polyvoice.h:28-33, VoiceMap.h:64-73).
// ----------------------------------------------------------------------------------------------
struct MixArgs {
    const float *in;            // [n_frames][n] voice outputs
    float *out;                 // [n_frames][n_buses], accumulated into
    const uint32_t *off;        // [n_buses + 1]
    const uint32_t *order;      // [off[n_buses]] voice indices
    uint32_t n, n_buses, n_frames;
    // buses are contiguous voice runs in voice order (order[k] == k) on multiples of 4 voices
    // (voice_mix_v4's float4 runs), else 0 (voice_mix_v2)
    uint32_t quad;
};
hipError_t launch_mix(const MixArgs &a, hipStream_t s);

// ----------------------------------------------------------------------------------------------
// Level meter (meter.hip): per signal, the running RMS of ol::core::Rms and the sandbox firmware's
// peak-hold follower over n_frames frames of in.  out != null (envelope mode): out[p][f][i] = the rms
// after frame f; out == null (summary mode): the state alone advances.
// ----------------------------------------------------------------------------------------------
struct MeterArgs {
    const float *in;            // [planes][n_frames][n], planes `plane` floats apart
    float *out;                 // the same shape, or null
    float *state;               // [MTS_N][planes * n]
    const float *coef;          // [MTC_N][n]
    uint64_t plane;
    uint32_t n, n_frames, planes;
};
hipError_t launch_meter(const MeterArgs &a, hipStream_t s);

// host side: record a global error message (olfx_last_error(NULL))
void internal_set_error(const char *msg);

}  // namespace olfx
