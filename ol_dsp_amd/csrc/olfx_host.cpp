// ol_dsp_amd/csrc/olfx_host.cpp -- the HIP-free half of the host side (olfx_host.h): the kind
// tables, the coefficient derivation (the reference's setter semantics, at control rate), the
// parameter shadow with its validation, and the control packet's format.
#include "olfx_host.h"

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>

namespace olfx {
namespace host __attribute__((visibility("hidden"))) {      // as in olfx_host.h: not part of the ABI
namespace {

uint32_t pow2_at_least(uint32_t x) {
    uint32_t p = 1;
    while (p < x) p <<= 1;
    return p;
}

float clampf(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }

// a fraction of a cycle in [0, 1] as 64-bit fixed point (2^64 = one cycle); 1.0 wraps to 0
uint64_t fix64(double cycles) {
    constexpr double kTwo64 = 18446744073709551616.0;
    const double v = std::floor(cycles * kTwo64 + 0.5);
    return v <= 0 ? 0u : (v >= kTwo64 ? (uint64_t)(v - kTwo64) : (uint64_t)v);
}

uint32_t as_u32(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

size_t up4(size_t x) { return (x + 3) & ~(size_t)3; }

}  // namespace

// ol::core::scale (modules/corelib/ol_corelib.h:27-44), t_sample = float
float core_scale(float in, float inlow, float inhigh, float outlow, float outhigh, float power) {
    const float denom = inhigh - inlow;
    const float inscale = denom == 0.f ? 0.f : (float)(1.f / denom);
    const float outdiff = outhigh - outlow;
    float value = (in - inlow) * inscale;
    if (value > 0.0f) value = powf(value, power);
    else if (value < 0.0f) value = -powf(-value, power);
    return (value * outdiff) + outlow;
}

// ---- the components' defaults (the reference's, of the user-facing parameters) ----
namespace {

void plate_defaults(float *p) {
    // verb.cpp:215-221
    p[OLFX_DT_PREDELAY] = (float)0.1;
    p[OLFX_DT_PREFILTER] = (float)0.85;
    p[OLFX_DT_INPUT_DIFFUSION1] = (float)0.75;
    p[OLFX_DT_INPUT_DIFFUSION2] = (float)0.625;
    p[OLFX_DT_DECAY_DIFFUSION] = (float)0.70;
    p[OLFX_DT_DECAY] = (float)0.75;
    p[OLFX_DT_DAMPING] = (float)0.95;
}

void chorus_defaults(float *p) {
    // mono-chorus.rnbopat param boxes (:431,1772,2226,2660,3420,3854,4353)
    p[OLFX_CH_PITCH] = 0.0f;
    p[OLFX_CH_MIX] = 0.5f;
    p[OLFX_CH_Q] = 0.5f;
    p[OLFX_CH_CUTOFF] = 0.3f;
    p[OLFX_CH_PHASE] = 1.0f;
    p[OLFX_CH_DEPTH] = 0.5f;
    p[OLFX_CH_RATE] = 0.2f;
    p[OLFX_CH_WINDOW] = 10.0f;
}

void pitch_defaults(float *p) {
    p[OLFX_PS_SHIFT] = 0.0f;
    p[OLFX_PS_WINDOW] = 10.0f;
}

void voice_defaults(float *p) {
    // SynthVoice member defaults (SynthVoice.h:285-311); Config order (Voice.h:14-31)
    p[OLFX_VC_FILTER_CUTOFF] = 0.0f;
    p[OLFX_VC_FILTER_RESONANCE] = 0.0f;
    p[OLFX_VC_FILTER_DRIVE] = 0.0f;
    p[OLFX_VC_FILTER_ENV_AMOUNT] = 1.0f;
    p[OLFX_VC_FILTER_ATTACK] = 0.0f;
    p[OLFX_VC_FILTER_ATTACK_SHAPE] = 1.0f;
    p[OLFX_VC_FILTER_DECAY] = 0.2f;
    p[OLFX_VC_FILTER_SUSTAIN] = 0.0f;
    p[OLFX_VC_FILTER_RELEASE] = 0.0f;
    p[OLFX_VC_AMP_ENV_AMOUNT] = 0.8f;
    p[OLFX_VC_AMP_ATTACK] = 0.01f;
    p[OLFX_VC_AMP_ATTACK_SHAPE] = 1.0f;
    p[OLFX_VC_AMP_DECAY] = 0.0f;
    p[OLFX_VC_AMP_SUSTAIN] = 1.0f;
    p[OLFX_VC_AMP_RELEASE] = 0.01f;
    p[OLFX_VC_PORTAMENTO] = 0.0f;
}

void rack_defaults(float *p) {
    // Fx.h member defaults; DelayFx::Init sets its filter through UpdateMidiControl(CC, 64 / 24)
    p[OLFX_FR_DELAY_TIME] = 0.5f;
    p[OLFX_FR_DELAY_FEEDBACK] = 0.5f;
    p[OLFX_FR_DELAY_BALANCE] = 0.33f;
    p[OLFX_FR_DELAY_CUTOFF] = core_scale(64.f, 0.f, 127.f, 0.f, 20000.f, 1.f);
    p[OLFX_FR_DELAY_RESONANCE] = core_scale(24.f, 0.f, 127.f, 0.f, 1.f, 1.f);
    p[OLFX_FR_REVERB_BALANCE] = 0.1f;
    p[OLFX_FR_FILTER_CUTOFF] = 20000.f;
    p[OLFX_FR_FILTER_RESONANCE] = 0.f;
    p[OLFX_FR_FILTER_DRIVE] = 0.f;
    p[OLFX_FR_FILTER_TYPE] = 0.f;
    p[OLFX_FR_MASTER_VOLUME] = 0.8f;
    p[OLFX_FR_TOPOLOGY] = 0.f;
}

void meter_defaults(float *p) {
    p[OLFX_MT_WINDOW] = 0.0f;                // Rms::Init's default argument (ol_corelib.h:71)
    p[OLFX_MT_PEAK_HOLD] = 2 * 48000;        // sandbox/main.cpp:101, a literal
}

}  // namespace

void chorus_sizes(float sr, uint32_t *psize, uint32_t *csize) {
    // pitch ring: delays up to W = 10 ms plus the interpolation neighbour
    *psize = pow2_at_least((uint32_t)std::ceil(10.0 * sr / 1000.0) + 2);
    // chorus ring: delays up to 2 D, D <= 12 ms (delay~ @maxsize samplerate*2 is never reached)
    *csize = pow2_at_least(2u * (uint32_t)std::ceil(12.0 * sr / 1000.0) + 2);
}

uint32_t chorus_history(float sr) { return 2u * (uint32_t)std::ceil(12.0 * sr / 1000.0) + 2u; }
uint32_t chorus_x_size(float sr) {
    // the oldest x a ring-free launch reads lies the chorus's largest delay, the psv window's tail, the
    // pitch delay clamp + 1 and a line's 15 positions back, while the next chunk's input (up to 31
    // positions ahead) is already stored: 64 covers those
    uint32_t ps, cs;
    chorus_sizes(sr, &ps, &cs);
    return pow2_at_least(chorus_history(sr) - 2u + (ps - 2u) + 64u);
}

// ---------------------------------------------------------------------------------------------
// Coefficient derivation (control rate, host).  These restate the reference setters.
// ---------------------------------------------------------------------------------------------
uint32_t dattorro_predelay_samples(float v) {
    // verb.cpp:137-139: uint16(value * 4800.f) into DelayBuffer_setDelay, whose read offset
    // mask + 1 - delay (verb.cpp:59-61) on the 8192-sample pre-delay ring makes the effective delay
    // uint16(value * 4800) mod 8192 (olfx_set_params accepts value * 4800 in [0, 65536))
    float d = v * 4800.0f;
    return d <= 0.0f ? 0u : ((uint32_t)(uint16_t)d & (kDtSize[DT_PRE] - 1u));
}

// plate: p = [OLFX_DT_*], c = [DTC_*] (floats, as u32 words)
void derive_dattorro(const float *p, uint32_t *c) {
    c[DTC_PREFILTER] = as_u32(p[OLFX_DT_PREFILTER]);
    c[DTC_IN1] = as_u32(p[OLFX_DT_INPUT_DIFFUSION1]);
    c[DTC_IN2] = as_u32(p[OLFX_DT_INPUT_DIFFUSION2]);
    c[DTC_DD1] = as_u32(p[OLFX_DT_DECAY_DIFFUSION]);
    c[DTC_DAMPING] = as_u32(p[OLFX_DT_DAMPING]);
    c[DTC_DECAY] = as_u32(p[OLFX_DT_DECAY]);
    // verb.cpp:49,162-165: clamp(t_sample x, ...) narrows value+0.15 to float
    float x = (float)((double)p[OLFX_DT_DECAY] + 0.15);
    c[DTC_DD2] = as_u32(x < 0.25f ? 0.25f : (x > 0.5f ? 0.5f : x));
    c[DTC_PREDELAY] = as_u32((float)dattorro_predelay_samples(p[OLFX_DT_PREDELAY]));
}

// chorus: p = [OLFX_CH_*], c = [CHC_*] (u32 words)
void derive_chorus(const float *p, double sr, uint32_t *c) {
    const double pitch = clampf(p[OLFX_CH_PITCH], 0.0f, 3.0f);
    const double mix = clampf(p[OLFX_CH_MIX], 0.0f, 1.0f);
    const double q = clampf(p[OLFX_CH_Q], 0.0f, 1.0f);
    const double cutoff = clampf(p[OLFX_CH_CUTOFF], 0.0f, 1.0f);
    const double phase = clampf(p[OLFX_CH_PHASE], 0.0f, 1.0f);
    const double depth = clampf(p[OLFX_CH_DEPTH], 0.08f, 1.0f);
    const double rate = clampf(p[OLFX_CH_RATE], 0.01f, 1.0f);
    const double window = clampf(p[OLFX_CH_WINDOW], 4.0f, 10.0f);

    const double rate_hz = 0.01 + rate * (0.5 - 0.01);           // scale 0 1 0.01 0.5 (:3935)
    const double depth_ms = 1.0 + depth * (12.0 - 1.0);          // scale 0 1 1 12 1   (:3436)
    const double fc = 300.0 + cutoff * (15000.0 - 300.0);         // scale 0 1 300 15000 1 (:2242)
    // 64-bit phasors: the increment rounding drifts a phase by < 2^-64 cycle per sample
    const uint64_t lfo_inc = fix64(rate_hz / sr), lfo_off = fix64(phase), ps_inc = fix64(pitch / sr);
    c[CHC_LFO_INC] = (uint32_t)(lfo_inc >> 32);
    c[CHC_LFO_INC_LO] = (uint32_t)lfo_inc;
    c[CHC_LFO_OFF] = (uint32_t)(lfo_off >> 32);                   // phase 1.0 wraps to 0
    c[CHC_LFO_OFF_LO] = (uint32_t)lfo_off;
    c[CHC_PS_INC] = (uint32_t)(ps_inc >> 32);
    c[CHC_PS_INC_LO] = (uint32_t)ps_inc;
    // D = mstosamps (:3897) as a double; W = mstosamps(window) in 32.32 fixed point (spec v2,
    // olfx_internal.h pitch_split / chorus_split)
    const double D = depth_ms * sr / 1000.0;
    uint64_t Dbits;
    std::memcpy(&Dbits, &D, 8);
    c[CHC_DEPTH] = (uint32_t)(Dbits >> 32);
    c[CHC_DEPTH_LO] = (uint32_t)Dbits;
    const uint64_t Wfix = (uint64_t)std::floor(window * sr / 1000.0 * 4294967296.0 + 0.5);
    c[CHC_WINDOW] = (uint32_t)(Wfix >> 32);
    c[CHC_WINDOW_LO] = (uint32_t)Wfix;
    // lores~ -> RBJ biquad low-pass, Q = 1/sqrt(2) + 20 q^3 (declared)
    const double Q = 0.70710678118654752 + 20.0 * q * q * q;
    const double w0 = 2.0 * 3.14159265358979323846 * fc / sr;
    const double cw = std::cos(w0), sw = std::sin(w0);
    const double alpha = sw / (2.0 * Q);
    const double a0 = 1.0 + alpha;
    c[CHC_B0] = as_u32((float)((1.0 - cw) * 0.5 / a0));
    c[CHC_B1] = as_u32((float)((1.0 - cw) / a0));
    c[CHC_B2] = as_u32((float)((1.0 - cw) * 0.5 / a0));
    c[CHC_A1] = as_u32((float)(-2.0 * cw / a0));
    c[CHC_A2] = as_u32((float)((1.0 - alpha) / a0));
    const float mixf = (float)mix;
    c[CHC_MIX] = as_u32(mixf);
    c[CHC_DRY] = as_u32(1.0f - mixf);                             // !- 1 (:1176)
}

// pitch-shift stage only: reuse the chorus coefficient block (mode 1 ignores the rest)
void derive_pitchshift(const float *p, double sr, uint32_t *c) {
    float cp[OLFX_CH_NPARAMS];
    chorus_defaults(cp);
    cp[OLFX_CH_PITCH] = p[OLFX_PS_SHIFT];
    cp[OLFX_CH_WINDOW] = p[OLFX_PS_WINDOW];
    derive_chorus(cp, sr, c);
}

namespace {

// DaisySP Adsr coefficient setters (restated; DaisySP is absent from the reference tree, see
// DESIGN.md "parity unpinned"): SetAttackTime / SetTimeConstant.
float adsr_attack_d0(float T, float shape, float sr, float *target_out) {
    float target = 9.f * powf(shape, 10.f) + 0.3f * shape + 1.01f;
    *target_out = target;
    if (T > 0.f) {
        float logTarget = logf(1.f - (1.f / target));
        return 1.f - expf(logTarget / (T * sr));
    }
    return 1.f;
}
float adsr_time_d0(float T, float sr) {
    if (T > 0.f) {
        const float target = logf((float)(1. / M_E));
        return 1.f - expf(target / (T * sr));
    }
    return 1.f;
}
float adsr_sustain(float s) { return (s <= 0.f) ? -0.01f : (s > 1.f ? 1.f : s); }

// FxRack<2> (modules/fxlib/Fx.h:398-492): DelayLine::SetDelay(scale(time, 0,1, 0,48000, 1)),
// and FilterFx::Update = Svf SetFreq, SetRes, SetDrive (DaisySP restated, as oracle/fxrack_ref.c)
void svf_coef(float cutoff, float res_in, float drive_in, float sr, float *freq, float *damp, float *drive) {
    const float fc = clampf(cutoff, 1.0e-6f, sr / 3.f);
    const float f = 2.0f * sinf(3.1415927410125732f * std::min(0.25f, fc / (sr * 2.0f)));
    const float res = clampf(res_in, 0.f, 1.f);
    *freq = f;
    *damp = std::min(2.0f * (1.0f - powf(res, 0.25f)), std::min(2.0f, 2.0f / f - f * 0.5f));
    *drive = clampf(drive_in * 0.1f, 0.f, 1.f) * res;
}

}  // namespace

void derive_fxrack(const float *p, float sr, uint32_t *c) {
    auto put = [&](int k, float v) { std::memcpy(&c[k], &v, 4); };
    const float dly = core_scale(p[OLFX_FR_DELAY_TIME], 0.f, 1.f, 0.f, (float)kFrMaxDelay, 1.f);
    const int32_t id = (int32_t)dly;
    c[FRC_DELAY] = (uint32_t)id < kFrMaxDelay ? (uint32_t)id : kFrMaxDelay - 1;
    put(FRC_FRAC, dly - (float)id);
    put(FRC_FEEDBACK, p[OLFX_FR_DELAY_FEEDBACK]);
    put(FRC_DBAL, p[OLFX_FR_DELAY_BALANCE]);
    float f, d, dr;
    svf_coef(p[OLFX_FR_DELAY_CUTOFF], p[OLFX_FR_DELAY_RESONANCE], 0.f, sr, &f, &d, &dr);
    put(FRC_DFREQ, f); put(FRC_DDAMP, d); put(FRC_DDRIVE, dr);
    put(FRC_RBAL, p[OLFX_FR_REVERB_BALANCE]);
    svf_coef(p[OLFX_FR_FILTER_CUTOFF], p[OLFX_FR_FILTER_RESONANCE], p[OLFX_FR_FILTER_DRIVE], sr, &f, &d, &dr);
    put(FRC_FFREQ, f); put(FRC_FDAMP, d); put(FRC_FDRIVE, dr);
    c[FRC_FTYPE] = (uint32_t)(int32_t)p[OLFX_FR_FILTER_TYPE];
    const uint32_t topo = (uint32_t)p[OLFX_FR_TOPOLOGY];     // 0..4 (validated by olfx_set_params)
    c[FRC_TOPO] = topo;
    put(FRC_MASTER, topo ? 1.0f : p[OLFX_FR_MASTER_VOLUME]);   // x 1.0f is exact: no FxRack, no master
}

// Voice: `configured` = false reproduces SynthVoice::Init without any Update()
// (SynthVoice.h:31-39): DaisySP Init defaults in the envelopes and the Svf.
void derive_voice(const float *p, bool configured, bool moog, float sr, uint32_t *w) {
    float c[VCC_N], tgt;
    if (!configured) {
        // daisysp::Adsr::Init: attack 0.1 s shape 0, decay 0.1 s, release 0.1 s, sustain 0.7
        c[VCC_ATK_D0A] = adsr_attack_d0(0.1f, 0.0f, sr, &tgt); c[VCC_ATK_TGT_A] = tgt;
        c[VCC_DEC_D0A] = adsr_time_d0(0.1f, sr);
        c[VCC_REL_D0A] = adsr_time_d0(0.1f, sr);
        c[VCC_SUS_A] = 0.7f;
        c[VCC_ATK_D0F] = c[VCC_ATK_D0A]; c[VCC_ATK_TGT_F] = tgt;
        c[VCC_DEC_D0F] = c[VCC_DEC_D0A];
        c[VCC_REL_D0F] = c[VCC_REL_D0A];
        c[VCC_SUS_F] = 0.7f;
        // daisysp::Svf::Init: res 0.5, drive 0.5
        c[VCC_DAMP_RES] = 2.0f * (1.0f - powf(0.5f, 0.25f));
        c[VCC_DRIVE] = 0.5f;
    } else {
        c[VCC_ATK_D0A] = adsr_attack_d0(p[OLFX_VC_AMP_ATTACK], p[OLFX_VC_AMP_ATTACK_SHAPE], sr, &tgt);
        c[VCC_ATK_TGT_A] = tgt;
        c[VCC_DEC_D0A] = adsr_time_d0(p[OLFX_VC_AMP_DECAY], sr);
        c[VCC_REL_D0A] = adsr_time_d0(p[OLFX_VC_AMP_RELEASE], sr);
        c[VCC_SUS_A] = adsr_sustain(p[OLFX_VC_AMP_SUSTAIN]);
        c[VCC_ATK_D0F] = adsr_attack_d0(p[OLFX_VC_FILTER_ATTACK], p[OLFX_VC_FILTER_ATTACK_SHAPE], sr, &tgt);
        c[VCC_ATK_TGT_F] = tgt;
        c[VCC_DEC_D0F] = adsr_time_d0(p[OLFX_VC_FILTER_DECAY], sr);
        c[VCC_REL_D0F] = adsr_time_d0(p[OLFX_VC_FILTER_RELEASE], sr);
        c[VCC_SUS_F] = adsr_sustain(p[OLFX_VC_FILTER_SUSTAIN]);
        // Svf::SetRes then Svf::SetDrive (SynthVoice::Update, SynthVoice.h:82-83)
        float res = fminf(fmaxf(p[OLFX_VC_FILTER_RESONANCE], 0.f), 1.f);
        float pre_drive = fminf(fmaxf(p[OLFX_VC_FILTER_DRIVE] * 0.1f, 0.f), 1.f);
        c[VCC_DAMP_RES] = 2.0f * (1.0f - powf(res, 0.25f));
        c[VCC_DRIVE] = pre_drive * res;
    }
    c[VCC_AMP_AMT] = p[OLFX_VC_AMP_ENV_AMOUNT];
    c[VCC_CUTOFF] = p[OLFX_VC_FILTER_CUTOFF];
    c[VCC_FENV_AMT] = p[OLFX_VC_FILTER_ENV_AMOUNT];
    // daisysp::Port (in-tree stub, Portamento.h:223-226): SynthVoice::Init passes the member
    // portamento_htime (SynthVoice.h:37), Update SetHtime(portamento_htime): either way the member
    float htime = p[OLFX_VC_PORTAMENTO];
    c[VCC_PORT_COEF] = expf(-1.0f / (htime * sr));
    c[VCC_FC_MAX] = sr / 3.f;
    c[VCC_SR] = sr;
    c[VCC_INV_SR] = 1.0f / sr;
    if (moog) {
        // daisysp::LadderFilter: Init -> SetRes(0.2), SetInputDrive(0.5) (drive <= 1: drive_scaled =
        // drive), sr_int_recip_ = 1 / (sr * 4); Update -> MoogFilter::SetRes -> SetRes(res):
        // K = 4 * clamp(res, 0, kMaxResonance 1.8); MoogFilter::SetDrive is a no-op
        const float res = configured ? p[OLFX_VC_FILTER_RESONANCE] : 0.2f;
        c[VCC_LADDER_K] = 4.0f * fminf(fmaxf(res, 0.0f), 1.8f);
        c[VCC_LADDER_DRIVE] = 0.5f;
        c[VCC_LADDER_WREC] = 1.0f / (sr * 4);
    }
    std::memcpy(w, c, sizeof c);
}

// Rms::Init (ol_corelib.h:71-73): window_ = window != 0 ? window : sample_rate / 375, in t_sample; the
// firmware's peak_hold as it is
void derive_meter(const float *p, float sr, uint32_t *c) {
    const float window = p[OLFX_MT_WINDOW];
    c[MTC_WINDOW] = as_u32(window != 0 ? window : sr / 375);
    c[MTC_HOLD] = as_u32(p[OLFX_MT_PEAK_HOLD]);
}

// ---------------------------------------------------------------------------------------------
// The components and the kind table: each kind is stated once, here.  The per-kind functions below, the
// shadow (through the row it looks up in init) and olfx_engine.cpp (scatter destinations, plane
// addressing, plate padding, kernel name) read the row.  Adding a kind that composes existing components
// takes one row here and a `launch` case in olfx_engine.cpp.  It takes a line in `carve` where no kind
// has that set of device arrays yet.  Its field names go into include/olfx.h and engine.py's PARAMS.
// ---------------------------------------------------------------------------------------------
namespace {

struct Component {
    uint32_t n_params, words;                    // user-facing parameters, coefficient words
    void (*defaults)(float *p);                  // the reference's defaults; null: no parameters
    // instance i's coefficient words from the component's parameters p
    void (*derive)(const float *p, const Shadow &s, uint32_t i, uint32_t *w);
};
constexpr Component kComponents[CP_COUNT] = {
    /* CP_PLATE  */ {OLFX_DT_NPARAMS, DTC_N, plate_defaults,
                     [](const float *p, const Shadow &, uint32_t, uint32_t *w) { derive_dattorro(p, w); }},
    /* CP_CHORUS */ {OLFX_CH_NPARAMS, CHC_N, chorus_defaults,
                     [](const float *p, const Shadow &s, uint32_t, uint32_t *w) { derive_chorus(p, s.sr, w); }},
    /* CP_PITCH  */ {OLFX_PS_NPARAMS, CHC_N, pitch_defaults,
                     [](const float *p, const Shadow &s, uint32_t, uint32_t *w) { derive_pitchshift(p, s.sr, w); }},
    /* CP_VOICE  */ {OLFX_VC_NPARAMS, VCC_N, voice_defaults,
                     [](const float *p, const Shadow &s, uint32_t i, uint32_t *w) {
                         derive_voice(p, s.configured[i] != 0, s.kd->moog, s.sr, w);
                     }},
    /* CP_RACK   */ {OLFX_FR_NPARAMS, FRC_N, rack_defaults,
                     [](const float *p, const Shadow &s, uint32_t, uint32_t *w) { derive_fxrack(p, s.sr, w); }},
    // the voice's Sample assignment: no parameters, its words come from olfx_sample_voices
    /* CP_SAMPLE */ {0, SMC_N, nullptr,
                     [](const float *, const Shadow &s, uint32_t i, uint32_t *w) { s.sample_record(i, w); }},
    // a kit's sum order: no parameters, its word comes from olfx_drumkit_map
    /* CP_ORDER  */ {0, DKC_N, nullptr,
                     [](const float *, const Shadow &s, uint32_t i, uint32_t *w) { w[DKC_ORDER] = s.order_word(i); }},
    /* CP_METER  */ {OLFX_MT_NPARAMS, MTC_N, meter_defaults,
                     [](const float *p, const Shadow &s, uint32_t, uint32_t *w) { derive_meter(p, s.sr, w); }},
};

constexpr size_t kKinds = OLFX_KIND_METER_MONO + 1;       // kind numbers 0 .. the last; 0, 9 and 13 are no kinds

constexpr std::array<KindDesc, kKinds> kKindTable = [] {
    std::array<KindDesc, kKinds> t{};
    auto row = [&t](int kind, std::initializer_list<Part> parts, const char *kernel, double bytes, double read_bytes)
        -> KindDesc & {
        KindDesc &k = t[(size_t)kind];
        for (const Part &p : parts) {
            k.parts[k.nparts++] = p;
            k.n_params += kComponents[p.comp].n_params;
            k.words += kComponents[p.comp].words;
            if (p.comp == CP_PLATE) k.pre_field = p.field0 + OLFX_DT_PREDELAY;
            if (p.comp == CP_RACK) k.topo_field = p.field0 + OLFX_FR_TOPOLOGY;
            if (p.comp == CP_VOICE) k.voice0 = p.field0, k.voice_end = p.field0 + OLFX_VC_NPARAMS;
            if (p.comp == CP_SAMPLE) k.has_sample = true;
        }
        k.kernel = kernel;
        k.bytes_per_frame = bytes;
        k.read_bytes_per_frame = read_bytes;
        return k;
    };
    // The two figures of a row: DESIGN.md section 4 / SURVEY.md section 8d, B = 256: compulsory ring
    // traffic + I/O; then its read share (the north star's "HBM-read roofline"): every tap read of data
    // older than the block, counted once, plus the input.
    KindDesc *k = nullptr;
    // no fixed kernel: the network of the last block (dattorro.hip dattorro_network)
    row(OLFX_KIND_DATTORRO, {{CP_PLATE, 0, TO_DT}}, nullptr,
        164.6,                            // 148.6 state + 8 in + 8 out (stereo in)
        6445.0 * 4.0 / 256.0 + 8.0);      // 27 taps: sum min(d, 256) = 6,445 floats; + 8 in
    k = &row(OLFX_KIND_CHORUS, {{CP_CHORUS, 0, TO_CH}}, "chorus_block_v11",
             56.0,                        // 2 x (pitch w + 2 taps + chorus w + tap) x 4 + 16 I/O
             32.0);                       // 2 x (2 pitch taps + chorus tap) x 4 + 8 in
    k->planes_32bit = true;
    // alone, the pitch-shifter runs the chorus kernel over the chorus arrays
    k = &row(OLFX_KIND_PITCHSHIFT, {{CP_PITCH, 0, TO_CH}}, "chorus_block_v11",
             40.0,                        // 2 x (w + 2 taps) x 4 + 16 I/O
             24.0);                       // 2 x 2 taps x 4 + 8 in
    k->planes_32bit = true;
    k = &row(OLFX_KIND_VOICE, {{CP_VOICE, 0, TO_VC}}, "voice_block_v5",
             5.4,                         // 4 B out + per-block state
             0.7);                        // per-block state and coefficients
    k->in_ch = 0; k->out_ch = 1; k->instances = KindDesc::VOICES;
    k = &row(OLFX_KIND_VOICE_MOOG, {{CP_VOICE, 0, TO_VC}}, "voice_block_v4",
             5.7,                         // 4 B out + per-block state (9 more state words)
             0.85);
    k->in_ch = 0; k->out_ch = 1; k->instances = KindDesc::VOICES; k->moog = true;
    // the voice, its Sample (the bank is the caller's data, not state)
    k = &row(OLFX_KIND_VOICE_SAMPLE, {{CP_VOICE, 0, TO_VC}, {CP_SAMPLE, OLFX_VC_NPARAMS, TO_SM}}, "sampler_block_v1",
             8.0,                         // 4 B of the sample read + 4 B out
             4.0);                        // the sample
    k->in_ch = 0; k->out_ch = 1; k->instances = KindDesc::VOICES;
    // chorus, pitch-shift, reverb; in the chain the pitch-shifter has arrays of its own
    k = &row(OLFX_KIND_CHAIN,
             {{CP_CHORUS, OLFX_CN_CHORUS0, TO_CH}, {CP_PITCH, OLFX_CN_PITCH0, TO_PS}, {CP_PLATE, OLFX_CN_VERB0, TO_DT}},
             "chain_block_v5", 228.6,
             8.0 + 24.0 + 16.0 + 6445.0 * 4.0 / 256.0);   // 148.7
    k->planes_32bit = true; k->pad_plate = true;
    k = &row(OLFX_KIND_FXRACK, {{CP_RACK, 0, TO_FR}}, "fxrack_block_v3",
             32.0,                        // ring write 8 + ring read 8 + I/O 16 per stereo frame
             16.0);                       // ring read 8 + in 8
    k->planes_32bit = true; k->topologies = 0x1F; k->topology_msg = "rack topology must be 0, 1, 2, 3 or 4";
    // rack, plate
    k = &row(OLFX_KIND_PLATERACK, {{CP_RACK, OLFX_PR_RACK0, TO_FR}, {CP_PLATE, OLFX_PR_VERB0, TO_DT}}, "platerack_block_v1",
             32.0 + 164.6 - 16.0,                // rack + plate - the plate's own I/O (in LDS now)
             16.0 + 6445.0 * 4.0 / 256.0);       // rack + the plate's taps (its input is in LDS)
    k->planes_32bit = true; k->pad_plate = true; k->state_counts_padding = true;
    // the plate as ReverbFx::Init -> Update() would set it through the glue of ReverbFx.cpp:29-37
    // (members Fx.h:274-281) where the member lies in the setter's domain; `cutoff` (12000 Hz, for
    // ReverbSc) does not and setPreDelay is never called: verb.cpp:215-221 for those two
    k->set[k->nset++] = {OLFX_PR_VERB0 + OLFX_DT_PREFILTER, 0.5f};          // pre_cutoff
    k->set[k->nset++] = {OLFX_PR_VERB0 + OLFX_DT_INPUT_DIFFUSION1, 0.5f};   // input_diffusion1
    k->set[k->nset++] = {OLFX_PR_VERB0 + OLFX_DT_INPUT_DIFFUSION2, 0.5f};   // input_diffusion2
    k->set[k->nset++] = {OLFX_PR_VERB0 + OLFX_DT_DECAY_DIFFUSION, 0.5f};    // decay_diffusion
    k->set[k->nset++] = {OLFX_PR_VERB0 + OLFX_DT_DECAY, 0.5f};              // decay_time
    // the components alone (2..4) are the firmware's objects around the ReverbSc stub: no plate in them
    k->topologies = 0x3; k->topology_msg = "plate rack topology must be 0 or 1";
    // the firmware's objects (main.cpp:49-67): SynthVoice members, then delay_fx / reverb_fx /
    // filter_fx as the rack's members, in the callback's topology
    k = &row(OLFX_KIND_SYNTH, {{CP_VOICE, OLFX_SY_VOICE0, TO_VC}, {CP_RACK, OLFX_SY_RACK0, TO_FR}}, "synth_block_v1",
             32.0 - 8.0,                  // the rack at topology 1 with no input read: ring 8 + 8, out 8
             16.0 - 8.0);                 // the ring read; the input never leaves LDS
    k->in_ch = 0; k->instances = KindDesc::INSTRUMENTS; k->moog = true;
    k->set[k->nset++] = {OLFX_SY_RACK0 + OLFX_FR_TOPOLOGY, 1.f};
    // the firmware's callback is the only chain the synth kernel runs
    k->topologies = 0x2; k->topology_msg = "synth rack topology must be 1";
    // the library's default-constructed SynthVoice behind the same rack, the firmware's callback first
    k = &row(OLFX_KIND_SYNTH_SVF, {{CP_VOICE, OLFX_SY_VOICE0, TO_VC}, {CP_RACK, OLFX_SY_RACK0, TO_FR}}, "synth_svf_block_v1",
             32.0 - 8.0,                  // as the synth (topology 0 stores its zero channel too: the same)
             16.0 - 8.0);
    k->in_ch = 0; k->instances = KindDesc::INSTRUMENTS;
    k->set[k->nset++] = {OLFX_SY_RACK0 + OLFX_FR_TOPOLOGY, 1.f};
    // the Svf synth runs the rack proper (0) as well; the components alone (2..4) have no voices in front
    k->topologies = 0x3; k->topology_msg = "svf synth rack topology must be 0 or 1";
    // the reference's drum machine: the rack and the sum order are the kit's record; eight slots of sample-voice
    // fields in front of the rack's, each slot a record of its own (voice coefficients, then its Sample)
    k = &row(OLFX_KIND_DRUMKIT, {{CP_RACK, OLFX_DK_RACK0, TO_FR}, {CP_ORDER, 0, TO_ORD}}, "drumkit_block_v1",
             32.0 - 8.0,                  // as the synths; the engine adds 4 B of sample read per voice of the kit
             16.0 - 8.0);
    k->in_ch = 0; k->instances = KindDesc::INSTRUMENTS;
    k->voice_slots = kDkMaxVoices;
    k->vparts[k->nvparts++] = {CP_VOICE, OLFX_DK_VOICE0, TO_VC};
    k->vparts[k->nvparts++] = {CP_SAMPLE, OLFX_DK_VOICE0, TO_SM};
    k->vwords = kComponents[CP_VOICE].words + kComponents[CP_SAMPLE].words;
    k->n_params += kDkMaxVoices * OLFX_VC_NPARAMS;
    k->voice0 = OLFX_DK_VOICE0; k->voice_end = OLFX_DK_RACK0;
    k->has_sample = true;
    k->set[k->nset++] = {OLFX_DK_RACK0 + OLFX_FR_TOPOLOGY, 1.f};
    k->topologies = 0x3; k->topology_msg = "drum kit rack topology must be 0 or 1";
    // the level meters: a pure stream.  The figures are the envelope mode's; summary mode (out == NULL) writes
    // nothing and moves the read share alone, half of the row's figure
    k = &row(OLFX_KIND_METER, {{CP_METER, 0, TO_MT}}, "meter_block_v1",
             16.0,                        // 2 x (4 B in + 4 B rms out)
             8.0);                        // the input
    k->no_controls = true; k->reset_keeps_params = true;
    k = &row(OLFX_KIND_METER_MONO, {{CP_METER, 0, TO_MT}}, "meter_block_v1",
             8.0,                         // 4 B in + 4 B rms out
             4.0);
    k->in_ch = 1; k->out_ch = 1; k->no_controls = true; k->reset_keeps_params = true;
    return t;
}();

// the most parameters a kind has (an instance's parameters on the stack)
constexpr uint32_t kMaxParams = [] {
    uint32_t m = 0;
    for (const KindDesc &k : kKindTable) m = std::max(m, k.n_params);
    return m;
}();

}  // namespace

const KindDesc &kind_desc(int kind) { return kKindTable[(size_t)kind < kKinds ? (size_t)kind : 0]; }

uint32_t n_params_of(int kind) { return kind_desc(kind).n_params; }
uint32_t in_channels(int kind) { return kind_desc(kind).in_ch; }
uint32_t out_channels(int kind) { return kind_desc(kind).out_ch; }
bool takes_note_events(int kind) { return kind_desc(kind).takes_note_events(); }
uint32_t max_segments(int kind) { return kind_desc(kind).instances == KindDesc::VOICES ? kSegCap : 1u; }
uint32_t max_note_segments(int kind) { return kind_desc(kind).instances == KindDesc::INSTRUMENTS ? kSegCap : 1u; }
double algorithmic_bytes_per_frame(int kind) { return kind_desc(kind).bytes_per_frame; }
double algorithmic_read_bytes_per_frame(int kind) { return kind_desc(kind).read_bytes_per_frame; }

void default_params(int kind, float *p) {
    const KindDesc &k = kind_desc(kind);
    for (uint32_t j = 0; j < k.nparts; ++j)
        if (const auto defaults = kComponents[k.parts[j].comp].defaults) defaults(p + k.parts[j].field0);
    for (uint32_t slot = 0; slot < k.voice_slots; ++slot)
        for (uint32_t j = 0; j < k.nvparts; ++j)
            if (const auto defaults = kComponents[k.vparts[j].comp].defaults)
                defaults(p + k.vparts[j].field0 + slot * OLFX_VC_NPARAMS);
    for (uint32_t j = 0; j < k.nset; ++j) p[k.set[j].field] = k.set[j].value;
}

Segments coef_segments(int kind) {
    const KindDesc &k = kind_desc(kind);
    Segments sg{k.nparts, {0, 0, 0}};
    for (uint32_t j = 0; j < k.nparts; ++j) sg.words[j] = kComponents[k.parts[j].comp].words;
    return sg;
}

Segments voice_segments(int kind) {
    const KindDesc &k = kind_desc(kind);
    Segments sg{k.nvparts, {0, 0, 0}};
    for (uint32_t j = 0; j < k.nvparts; ++j) sg.words[j] = kComponents[k.vparts[j].comp].words;
    return sg;
}

// The figure olfx_kind_info_get publishes: every part's rings, state and coefficient words.  Not what the
// engine allocates: the chain's second stage is counted with a chorus ring it does not have, and its plate
// without the padding to 64 instances.
uint64_t state_bytes(int kind, uint32_t n, float sr) {
    const KindDesc &k = kind_desc(kind);
    uint32_t ps, cs;
    chorus_sizes(sr, &ps, &cs);
    const uint64_t voices = k.instances == KindDesc::INSTRUMENTS ? kSynthDefaultVoices : 1u;
    uint64_t bytes = 0;
    for (uint32_t j = 0; j < k.nparts; ++j)
        switch (k.parts[j].comp) {
        case CP_PLATE:
            bytes += ((uint64_t)dt_total_floats() * 4 + DTS_N * 4 + DTC_N * 4) * (k.state_counts_padding ? (n + 63u) & ~63u : n);
            break;
        case CP_CHORUS:
        case CP_PITCH: bytes += ((uint64_t)2 * (ps + cs) * 4 + CHS_N * 4 + CHC_N * 4) * n; break;
        // one set of voice coefficients, every voice's state
        case CP_VOICE: bytes += ((uint64_t)VCC_N * 4 + voices * (k.moog ? VCS_N_MOOG : VCS_N) * 4) * n; break;
        case CP_RACK: bytes += ((uint64_t)kFrMaxDelay * 2 * 4 + FRS_N * 4 + FRC_N * 4) * n; break;
        case CP_SAMPLE: bytes += (uint64_t)SMC_N * 4 * n; break;
        // every channel's five floats, one set of coefficients per instance
        case CP_METER: bytes += ((uint64_t)MTS_N * k.in_ch + MTC_N) * 4 * n; break;
        default: break;
        }
    // a kit's voices: each its own state, coefficients and Sample words
    for (uint32_t j = 0; j < k.nvparts; ++j)
        bytes += voices * (kComponents[k.vparts[j].comp].words + (k.vparts[j].comp == CP_VOICE ? (uint64_t)VCS_N : 0u)) * 4 * n;
    return bytes;
}

void Shadow::derive_record(uint32_t i, uint32_t *w) const {
    // (an instrument whose last timed record still stands: the whole record, fold_segments derived it)
    if (const uint32_t *kept = kept_inst.find(i)) {
        std::memcpy(w, kept, (size_t)kd->words * 4);
        return;
    }
    float p[kMaxParams];
    for (uint32_t f = 0; f < n_params; ++f) p[f] = params[(size_t)f * n + i];
    // (a voice whose last timed record still stands: those words, fold_segments derived them)
    const uint32_t *const kept = kept_voice.find(i);
    for (uint32_t j = 0; j < kd->nparts; ++j) {
        const Component &c = kComponents[kd->parts[j].comp];
        if (kept && kd->parts[j].comp == CP_VOICE) std::memcpy(w, kept, (size_t)VCC_N * 4);
        else c.derive(p + kd->parts[j].field0, *this, i, w);
        w += c.words;
    }
}

void Shadow::derive_voice_record(uint32_t hv, uint32_t *w) const {
    if (const uint32_t *kept = kept_slot.find(hv)) {      // (as derive_record: the slot's last timed record stands)
        std::memcpy(w, kept, (size_t)kd->vwords * 4);
        return;
    }
    const uint32_t p = hv / n, i = hv % n;
    float v[OLFX_VC_NPARAMS];
    for (uint32_t f = 0; f < OLFX_VC_NPARAMS; ++f) v[f] = params[(size_t)(kd->voice0 + p * OLFX_VC_NPARAMS + f) * n + i];
    derive_voice(v, configured[hv] != 0, kd->moog, sr, w);
    sample_record(i * voices + p, w + VCC_N);
}

// VoiceMap::Process (VoiceMap.h:64-73) visits the notes in ascending order; a valid map holds each voice once
uint32_t Shadow::order_word(uint32_t kit_) const {
    uint32_t word = kDkOrderEmpty, k = 0;
    for (uint32_t note = 0; note < 128 && k < 8; ++note) {
        const uint8_t v = note2voice[(size_t)note * n + kit_];
        if (v == kNoVoice) continue;
        word = (word & ~(0xFu << (4 * k))) | (uint32_t)v << (4 * k);
        ++k;
    }
    return word;
}

// ---------------------------------------------------------------------------------------------
// The parameter shadow: validation and bookkeeping
// ---------------------------------------------------------------------------------------------
int Shadow::fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(msg, sizeof msg, fmt, ap);
    va_end(ap);
    return code;
}

void Shadow::reset() {
    // (a meter's window and hold outlive a reset, as its owner's Init and peak_hold outlive a cleared level)
    if (!kd->reset_keeps_params || params.size() != (size_t)n_params * n) {
        params.assign((size_t)n_params * n, 0.f);
        float d[kMaxParams];
        default_params(kind, d);
        for (uint32_t f = 0; f < n_params; ++f)
            std::fill(params.begin() + (size_t)f * n, params.begin() + (size_t)(f + 1) * n, d[f]);
    }
    const size_t slots = kit() ? (size_t)voices * n : 0u;
    configured.assign(kit() ? slots : n, 0);
    kept_voice.init(kd->instances == KindDesc::VOICES ? n : 0u, VCC_N);
    kept_inst.init(instruments() ? n : 0u, kd->words);
    kept_slot.init(slots, kd->vwords);
    vdirty_list.clear();
    vdirty_mark.assign(slots, 0);
    for (uint32_t hv = 0; hv < slots; ++hv) mark_vdirty(hv);
    n_components = 0;
    pre_changed = true;
    events.clear();
    timed.clear();
    tparams.clear();
    iparams.clear();
    vrec.clear();
    frec.clear();
    pre_valid = false;
    fold_fresh = false;
    changed_inst.clear();
    changed_slot.clear();
    last_v.assign(kit() ? slots : instruments() ? n : 0u, -1);
    last_f.assign(instruments() ? n : 0u, -1);
    ev_slot.assign(n_ev(), -1);
    playing.assign((size_t)voices * n, 0);
    dirty_list.clear();
    dirty_mark.assign(n, 0);
    mark_dirty(0, n);                        // every coefficient is derived at the first block
    rf.reset();
    rf_materialise = false;
    pitch_sent.assign(kind == OLFX_KIND_CHORUS ? (size_t)4 * n : 0u, 0u);
}

void Shadow::mark_dirty(uint32_t first, uint32_t count) {
    for (uint32_t k = first; k < first + count; ++k) {
        kept_voice.forget(k);                             // whatever is written now, a kept timed record is stale
        kept_inst.forget(k);
        if (!dirty_mark[k]) {
            dirty_mark[k] = 1;
            dirty_list.push_back(k);
        }
    }
}

void Shadow::mark_vdirty(uint32_t hv) {
    kept_slot.forget(hv);
    if (!vdirty_mark[hv]) {
        vdirty_mark[hv] = 1;
        vdirty_list.push_back(hv);
    }
}

void Shadow::touched(uint32_t inst, uint32_t field0, uint32_t n_fields) {
    if (!kit()) {
        if (touches_voice(field0, n_fields)) configured[inst] = 1;
        mark_dirty(inst, 1);
        return;
    }
    // the voice slots whose sixteen fields the range meets (slots past the kit's voices are read by nothing)
    for (uint32_t p = 0; p < voices; ++p) {
        const uint32_t lo = kd->voice0 + p * OLFX_VC_NPARAMS;
        if (n_fields && field0 < lo + OLFX_VC_NPARAMS && field0 + n_fields > lo) {
            configured[(size_t)p * n + inst] = 1;
            mark_vdirty(p * n + inst);
        }
    }
    if (field0 + n_fields > kd->voice_end) mark_dirty(inst, 1);       // the rack's
}

// A parameter value the reference's setter gives a meaning to (nullptr) or why not.
const char *Shadow::bad_value(uint32_t field, float v) const {
    if (!std::isfinite(v)) return "non-finite value";
    // the reference converts value * MAX_PREDELAY (4800) to uint16 (verb.cpp:137-139): values whose
    // product leaves [0, 65536) have no defined meaning there
    if (field == kd->pre_field && !(v >= 0.f && v * 4800.0f < 65536.0f)) return "pre-delay outside [0, 65536/4800)";
    // a whole number 0..4 that the kind's rack runs
    if (field == kd->topo_field && !(v >= 0.f && v <= 4.f && v == (float)(int)v && (kd->topologies >> (int)v & 1)))
        return kd->topology_msg;
    return nullptr;
}

// One parameter of one instance; the rack's count of standalone components (topology >= 2, the
// kernel variant that serves them) follows its topology field.
void Shadow::store_param(uint32_t field, uint32_t inst, float v) {
    float &slot = params[(size_t)field * n + inst];
    // (only the standalone reverb, the kind without a fixed kernel, picks its network by the pre-delays)
    if (field == kd->pre_field && !kd->kernel) pre_changed = true;
    if (field == kd->topo_field) n_components += (v >= 2.f ? 1 : 0) - (slot >= 2.f ? 1 : 0);
    slot = v;
}

int Shadow::set_range(uint32_t first, uint32_t count, uint32_t field0, uint32_t n_fields, const float *values) {
    if (!values || (uint64_t)first + count > n || (uint64_t)field0 + n_fields > n_params)
        return fail(OLFX_E_ARG, "olfx_set_params: range out of bounds");
    // validate everything first: a rejected call changes nothing
    for (uint32_t f = 0; f < n_fields; ++f)
        for (uint32_t k = 0; k < count; ++k)
            if (const char *why = bad_value(field0 + f, values[(size_t)f * count + k]))
                return fail(OLFX_E_ARG, "olfx_set_params: %s", why);
    for (uint32_t f = 0; f < n_fields; ++f)
        for (uint32_t k = 0; k < count; ++k) store_param(field0 + f, first + k, values[(size_t)f * count + k]);
    for (uint32_t k = 0; k < count; ++k) touched(first + k, field0, n_fields);
    return OLFX_OK;
}

int Shadow::set_list(uint32_t field, const uint32_t *inst, const float *values, uint32_t count) {
    if (count && (!inst || !values)) return fail(OLFX_E_ARG, "olfx_set_param_list: null list");
    if (field >= n_params) return fail(OLFX_E_ARG, "olfx_set_param_list: field out of range");
    for (uint32_t k = 0; k < count; ++k) {
        if (inst[k] >= n) return fail(OLFX_E_ARG, "olfx_set_param_list: instance %u out of range", inst[k]);
        if (const char *why = bad_value(field, values[k])) return fail(OLFX_E_ARG, "olfx_set_param_list: %s", why);
    }
    for (uint32_t k = 0; k < count; ++k) {
        store_param(field, inst[k], values[k]);
        touched(inst[k], field, 1);
    }
    return OLFX_OK;
}

int Shadow::set_member(uint32_t inst, uint32_t field, float value) {
    // (the synth: a voice field is the member of all its voices, a rack field is olfx_set_param)
    if (!touches_voice(field, 1)) return set_range(inst, 1, field, 1, &value);
    if (inst >= n || field >= n_params) return fail(OLFX_E_ARG, "olfx_set_member: out of range");
    if (const char *why = bad_value(field, value)) return fail(OLFX_E_ARG, "olfx_set_member: %s", why);
    // SynthVoice::Process reads filter_cutoff, filter_env_amount and amp_env_amount itself every
    // sample (SynthVoice.h:42-52): writing them takes effect at once, Update()d or not.  Re-deriving
    // at the next block changes nothing else, since every other member still holds the value the
    // last Update() saw (they change only through olfx_set_params, i.e. with an Update()).
    const uint32_t vf = (field - kd->voice0) % OLFX_VC_NPARAMS, slot = (field - kd->voice0) / OLFX_VC_NPARAMS;
    const bool process_reads = vf == OLFX_VC_FILTER_CUTOFF || vf == OLFX_VC_FILTER_ENV_AMOUNT ||
                               vf == OLFX_VC_AMP_ENV_AMOUNT;
    if (kit()) {
        // the member of voice slot `slot` alone; a slot past the kit's voices is stored and read by nothing
        if (slot < voices) {
            if (configured[(size_t)slot * n + inst] && !process_reads)
                return fail(OLFX_E_STATE, "olfx_set_member: voice %u of kit %u is already Update()d (use olfx_set_params)",
                            slot, inst);
            mark_vdirty(slot * n + inst);
        }
        store_param(field, inst, value);
        return OLFX_OK;
    }
    // the other members feed the components only through Update() (SynthVoice.h:66-98); written
    // after the first Update() they would take effect at the next block as if Update() had run,
    // which SynthVoice does not do: refused instead of silently diverging
    if (configured[inst] && !process_reads)
        return fail(OLFX_E_STATE, "olfx_set_member: instance %u is already Update()d (use olfx_set_params)", inst);
    store_param(field, inst, value);                    // no Update(): `configured` unchanged
    mark_dirty(inst, 1);
    return OLFX_OK;
}

int Shadow::update(uint32_t first, uint32_t count) {
    if ((uint64_t)first + count > n) return fail(OLFX_E_ARG, "olfx_update: range out of bounds");
    if (kit()) {                            // every voice of those kits, and their racks
        for (uint32_t p = 0; p < voices; ++p)
            for (uint32_t k = 0; k < count; ++k) {
                configured[(size_t)p * n + first + k] = 1;
                mark_vdirty(p * n + first + k);
            }
    } else if (kd->takes_note_events()) {
        for (uint32_t k = 0; k < count; ++k) configured[first + k] = 1;
    }
    mark_dirty(first, count);
    return OLFX_OK;
}

// ---- sample voices ----
int Shadow::bank_plan(uint32_t n_samples, const uint64_t *offsets, const float *pcm, BankPlan *plan) {
    if (!kd->has_sample) return fail(OLFX_E_STATE, "olfx_sample_bank: not a sample-voice engine");
    plan->base.clear();
    plan->len.clear();
    plan->floats = 0;
    if (!n_samples) return OLFX_OK;
    if (!offsets || offsets[0] != 0) return fail(OLFX_E_ARG, "olfx_sample_bank: offsets must start at 0");
    uint64_t at = 0;
    for (uint32_t k = 0; k < n_samples; ++k) {
        if (offsets[k + 1] < offsets[k]) return fail(OLFX_E_ARG, "olfx_sample_bank: offsets decrease at sample %u", k);
        const uint64_t len = offsets[k + 1] - offsets[k];
        if (len >= 0xFFFFFFFFull) return fail(OLFX_E_ARG, "olfx_sample_bank: sample %u has 2^32 - 1 frames or more", k);
        if (at + len > kSmMaxBankFloats) return fail(OLFX_E_ARG, "olfx_sample_bank: the bank exceeds %llu frames",
                                                     (unsigned long long)kSmMaxBankFloats);
        plan->base.push_back((uint32_t)at);
        plan->len.push_back((uint32_t)len);
        at = (at + len + kSmAlign - 1) / kSmAlign * kSmAlign;
    }
    if (offsets[n_samples] && !pcm) return fail(OLFX_E_ARG, "olfx_sample_bank: null pcm");
    plan->floats = at + kSmAlign;           // the padded tail: a fetch that starts inside a sample ends inside the bank
    return OLFX_OK;
}

void Shadow::bank_commit(BankPlan &&plan) {
    bank = std::move(plan);
    for (SampleAsg &a : samples) {
        if (a.sample != OLFX_NO_SAMPLE && a.sample >= bank.len.size()) a = SampleAsg{OLFX_NO_SAMPLE, 0, 0, 0, a.gen};
        ++a.gen;                            // a fresh Sample over the new data
    }
    if (kit())
        for (uint32_t hv = 0; hv < voices * n; ++hv) mark_vdirty(hv);
    else
        mark_dirty(0, n);
}

int Shadow::sample_voices(const olfx_sample_voice *recs, uint32_t count) {
    if (!kd->has_sample) return fail(OLFX_E_STATE, "olfx_sample_voices: not a sample-voice engine");
    if (count && !recs) return fail(OLFX_E_ARG, "olfx_sample_voices: null records");
    for (uint32_t k = 0; k < count; ++k) {
        if (recs[k].inst >= n_voices()) return fail(OLFX_E_ARG, "olfx_sample_voices: record %u: voice out of range", k);
        if (recs[k].sample != OLFX_NO_SAMPLE && recs[k].sample >= bank.len.size())
            return fail(OLFX_E_ARG, "olfx_sample_voices: record %u: sample %u of %zu", k, recs[k].sample, bank.len.size());
        if (recs[k].play_mode > OLFX_SAMPLE_LOOP) return fail(OLFX_E_ARG, "olfx_sample_voices: record %u: bad play mode", k);
    }
    for (uint32_t k = 0; k < count; ++k) {
        SampleAsg &a = samples[recs[k].inst];
        if (a.sample != recs[k].sample) ++a.gen;       // another sample (or none): a new Sample object
        a.sample = recs[k].sample;
        a.mode = recs[k].play_mode;
        a.loop_start = recs[k].loop_start;
        a.loop_end = recs[k].loop_end;
        if (kit()) mark_vdirty((recs[k].inst % voices) * n + recs[k].inst / voices);   // inst = kit * voices + p
        else mark_dirty(recs[k].inst, 1);
    }
    return OLFX_OK;
}

// The Sample's members reduced to what Sample::Process can observe over a len-frame source: Seek(k)
// puts the data cursor at min(k, len), and the frame count is compared with loop_end only after a
// read, where it equals the data cursor (<= len): a loop_end >= len never fires, like 0.
void Shadow::sample_record(uint32_t i, uint32_t *w) const {
    const SampleAsg &a = samples[i];
    const bool has = a.sample != OLFX_NO_SAMPLE && a.sample < bank.len.size();
    const uint32_t len = has ? bank.len[a.sample] : 0u;
    w[SMC_BASE] = has ? bank.base[a.sample] : 0u;
    w[SMC_LEN] = len;
    w[SMC_LS] = (uint32_t)std::min<uint64_t>(a.loop_start, len);
    w[SMC_LE] = a.loop_end < len ? (uint32_t)a.loop_end : 0u;
    w[SMC_MODE] = (a.mode == OLFX_SAMPLE_LOOP ? 1u : 0u) | a.gen << 1;
}

bool Shadow::uniform_predelay() const {
    if (kd->pre_field == kNoField) return true;
    const float *pd = params.data() + (size_t)kd->pre_field * n;
    const uint32_t d0 = dattorro_predelay_samples(pd[0]);
    for (uint32_t i = 1; i < n; ++i)
        if (dattorro_predelay_samples(pd[i]) != d0) return false;
    return true;
}

// ---- control changes (corelib/cc_map.h) ----
namespace {
enum : uint8_t {
    CC_CTL_PORTAMENTO = 5, CC_CTL_VOLUME = 7,
    CC_REVERB_TIME = 32, CC_REVERB_CUTOFF = 33, CC_REVERB_BALANCE = 34,
    CC_EARLY_PREDELAY = 50, CC_REVERB_PREDELAY = 52, CC_REVERB_PREFILTER = 53,
    CC_REVERB_INPUT_DIFFUSION_1 = 54, CC_REVERB_INPUT_DIFFUSION_2 = 55, CC_REVERB_DECAY_DIFFUSION = 56,
    CC_DELAY_TIME = 35, CC_DELAY_FEEDBACK = 36, CC_DELAY_CUTOFF = 37, CC_DELAY_RESONANCE = 38,
    CC_DELAY_BALANCE = 39,
    CC_FILTER_CUTOFF = 41, CC_FILTER_RESONANCE = 42, CC_FILTER_DRIVE = 44,
    CC_FX_FILTER_CUTOFF = 45, CC_FX_FILTER_RESONANCE = 46, CC_FX_FILTER_TYPE = 47, CC_FX_FILTER_DRIVE = 48,
    CC_ENV_FILT_AMT = 73, CC_ENV_FILT_A = 74, CC_ENV_FILT_D = 75, CC_ENV_FILT_S = 76, CC_ENV_FILT_R = 77,
    CC_ENV_AMP_A = 108, CC_ENV_AMP_D = 109, CC_ENV_AMP_S = 110, CC_ENV_AMP_R = 111,
    CC_OSC_1_VOLUME = 114,
};
// the controls ReverbFx's handlers take (Fx.h:313-391)
bool is_reverb_cc(uint8_t c) {
    return (c >= CC_REVERB_TIME && c <= CC_REVERB_BALANCE) || c == CC_EARLY_PREDELAY ||
           (c >= CC_REVERB_PREDELAY && c <= CC_REVERB_DECAY_DIFFUSION);
}
}  // namespace

namespace {

// A control's value as the handlers scale it.  MIDI: ol::core::scale(val, 0, 127, lo, hi, power);
// hardware: scale(value, 0, 1, ...) or the raw value.
struct CcValue {
    bool midi;
    float value;
    uint32_t *field;                             // what a table's entry sets, and to what
    float *param_value;
    int put(uint32_t f, float v) const { *field = f; *param_value = v; return OLFX_OK; }
    float sc(float hi, float power) const {
        return midi ? core_scale(value, 0.f, 127.f, 0.f, hi, power) : core_scale(value, 0.f, 1.f, 0.f, hi, power);
    }
    float unit() const { return midi ? core_scale(value, 0.f, 127.f, 0.f, 1.f, 1.f) : value; }   // `scaled` / raw value
};

// The components' control tables: the reference's handlers, restated.  Each gives the component's own
// field (or OLFX_FIELD_UPDATE_ONLY) and returns OLFX_OK, or OLFX_IGNORED.
int voice_cc(uint8_t control, const CcValue &x) {     // SynthVoice.h:100-229
    switch (control) {
    case CC_CTL_VOLUME: return x.put(OLFX_VC_AMP_ENV_AMOUNT, x.unit());
    case CC_CTL_PORTAMENTO: return x.put(OLFX_VC_PORTAMENTO, x.sc(1.f, 4.f));
    case CC_FILTER_CUTOFF: return x.put(OLFX_VC_FILTER_CUTOFF, x.sc(20000.f, 2.5f));
    case CC_FILTER_RESONANCE: return x.put(OLFX_VC_FILTER_RESONANCE, x.unit());
    case CC_FILTER_DRIVE: return x.put(OLFX_VC_FILTER_DRIVE, x.unit());
    case CC_ENV_FILT_AMT: return x.put(OLFX_VC_FILTER_ENV_AMOUNT, x.unit());
    case CC_ENV_FILT_A: return x.put(OLFX_VC_FILTER_ATTACK, x.unit());
    case CC_ENV_FILT_D: return x.put(OLFX_VC_FILTER_DECAY, x.sc(1.f, 3.f));
    case CC_ENV_FILT_S: return x.put(OLFX_VC_FILTER_SUSTAIN, x.unit());
    case CC_ENV_FILT_R: return x.put(OLFX_VC_FILTER_RELEASE, x.unit());
    case CC_ENV_AMP_A: return x.put(OLFX_VC_AMP_ATTACK, x.unit());
    case CC_ENV_AMP_D: return x.put(OLFX_VC_AMP_DECAY, x.unit());
    case CC_ENV_AMP_S: return x.put(OLFX_VC_AMP_SUSTAIN, x.unit());
    case CC_ENV_AMP_R: return x.put(OLFX_VC_AMP_RELEASE, x.unit());
    case CC_OSC_1_VOLUME: return x.put(OLFX_FIELD_UPDATE_ONLY, x.unit());   // osc_1_mix: unused by Process
    default: return OLFX_IGNORED;
    }
}

// The plate as a rack's reverb: ReverbFx::UpdateMidiControl / UpdateHardwareControl (Fx.h:313-391)
// composed with the plate glue (ReverbFx.cpp:29-37)
int reverbfx_cc(uint8_t control, const CcValue &x) {
    switch (control) {
    case CC_REVERB_TIME: return x.put(OLFX_DT_DECAY, x.unit());
    case CC_REVERB_PREFILTER: return x.put(OLFX_DT_PREFILTER, x.unit());
    case CC_REVERB_INPUT_DIFFUSION_1: return x.put(OLFX_DT_INPUT_DIFFUSION1, x.unit());
    case CC_REVERB_DECAY_DIFFUSION:
    case CC_REVERB_INPUT_DIFFUSION_2:          // the reference's quirk (Fx.h:323-324), kept
        return x.put(OLFX_DT_DECAY_DIFFUSION, x.unit());
    case CC_REVERB_CUTOFF: return x.put(OLFX_DT_DAMPING, x.unit());   // the 0..1 form (Fx.h:328)
    case CC_REVERB_PREDELAY:
    case CC_EARLY_PREDELAY: return x.put(OLFX_FIELD_UPDATE_ONLY, x.unit());   // members the glue never forwards
    default: return OLFX_IGNORED;
    }
}

int rack_cc(uint8_t control, const CcValue &x) {      // FxRack -> FilterFx / DelayFx / ReverbFx
    switch (control) {
    case CC_FX_FILTER_CUTOFF: return x.put(OLFX_FR_FILTER_CUTOFF, x.midi ? x.sc(20000.f, 1.f) : x.sc(20000.f, 1.02f));
    case CC_FX_FILTER_RESONANCE: return x.put(OLFX_FR_FILTER_RESONANCE, x.unit());
    case CC_FX_FILTER_DRIVE: return x.put(OLFX_FR_FILTER_DRIVE, x.unit());
    case CC_FX_FILTER_TYPE: return x.put(OLFX_FR_FILTER_TYPE, (float)(int32_t)x.sc(5.f, 1.f));   // FilterType(float)
    case CC_DELAY_TIME: return x.put(OLFX_FR_DELAY_TIME, x.unit());
    case CC_DELAY_FEEDBACK: return x.put(OLFX_FR_DELAY_FEEDBACK, x.unit());
    case CC_DELAY_BALANCE: return x.put(OLFX_FR_DELAY_BALANCE, x.unit());
    case CC_DELAY_CUTOFF:                      // DelayFx handles these in MIDI only (Fx.h:253-260)
        return x.midi ? x.put(OLFX_FR_DELAY_CUTOFF, x.sc(20000.f, 1.f)) : OLFX_IGNORED;
    case CC_DELAY_RESONANCE: return x.midi ? x.put(OLFX_FR_DELAY_RESONANCE, x.unit()) : OLFX_IGNORED;
    case CC_REVERB_BALANCE: return x.put(OLFX_FR_REVERB_BALANCE, x.unit());
    case CC_CTL_VOLUME: return x.put(OLFX_FR_MASTER_VOLUME, x.unit());
    default: return OLFX_IGNORED;              // incl. the reverb CCs that reach only the ReverbSc stub
    }
}

// One control through a kind's parts, in order, with its rack at `topology`: the 0 to 2 (field, value)
// pairs it sets, or an error.  Voices take their controls whatever the topology (handleMidi,
// ol_daisy/app/synth/main.cpp:201-207: the voices, then delay_fx, reverb_fx, filter_fx).  Topology 0 is
// FxRack with its own handlers (Fx.h:451-489).  At the others there is no FxRack around the components
// (main.cpp sends every CC to delay_fx, reverb_fx and filter_fx directly): CC_FILTER_* (41-44) reach a
// FilterFx's own handler (Fx.h:116-139), which the rack's table reaches as CC_FX_FILTER_* (45-48);
// FxRack's own CC_FX_FILTER_* and master volume (CC 7) reach nothing.  A component alone (2..4) takes only
// its own controls: DelayFx 35-39 (Fx.h:218-267), ReverbFx the reverb CCs (of which only the balance, 34,
// is audible through the ReverbSc stub; a plate behind the rack is its ReverbFx and takes them all),
// FilterFx 41-44.  A plate without a rack has no handlers.
int route_control(const KindDesc &kd, uint32_t topology, uint8_t control, int source, float value, uint32_t field[2],
                  float param_value[2]) {
    if (!kd.nparts) return OLFX_E_KIND;
    const bool filter_cc = control >= CC_FILTER_CUTOFF && control <= CC_FILTER_DRIVE;
    const bool delay_cc = control >= CC_DELAY_TIME && control <= CC_DELAY_BALANCE;
    const bool has_rack = kd.topo_field != kNoField;
    int hits = 0;
    for (uint32_t j = 0; j < kd.nparts; ++j) {
        const Part &pt = kd.parts[j];
        uint8_t as = control;
        if (topology && pt.comp == CP_RACK) {
            const bool takes = topology == 1u   ? filter_cc || delay_cc || control == CC_REVERB_BALANCE
                               : topology == 2u ? delay_cc
                               : topology == 3u ? control == CC_REVERB_BALANCE
                                                : filter_cc;
            if (!takes) continue;
            if (filter_cc) as = (uint8_t)(control - CC_FILTER_CUTOFF + CC_FX_FILTER_CUTOFF);
        }
        if (topology && pt.comp == CP_PLATE && !(topology == 1u && is_reverb_cc(control))) continue;
        if (source != OLFX_CTL_MIDI && source != OLFX_CTL_HARDWARE) return OLFX_E_ARG;
        uint32_t f = 0;
        float v = 0.f;
        const CcValue x{source == OLFX_CTL_MIDI, value, &f, &v};
        int rc = OLFX_IGNORED;
        if (pt.comp == CP_VOICE) rc = voice_cc(as, x);
        else if (pt.comp == CP_RACK) rc = rack_cc(as, x);
        else if (pt.comp == CP_PLATE && has_rack) rc = reverbfx_cc(as, x);
        if (rc == OLFX_OK && hits < 2) {
            field[hits] = f == OLFX_FIELD_UPDATE_ONLY ? f : pt.field0 + f;
            param_value[hits++] = v;
        }
    }
    return hits;
}

}  // namespace

int Shadow::control(const olfx_control_event *ev, uint32_t count) {
    if (kd->no_controls) return fail(OLFX_E_KIND, "olfx_control: no control maps to this kind");
    if (count && !ev) return fail(OLFX_E_ARG, "olfx_control: null events");
    for (uint32_t k = 0; k < count; ++k) {
        if (ev[k].inst >= n) return fail(OLFX_E_ARG, "olfx_control: event %u: instance out of range", k);
        if (kit() && ev[k].pad != OLFX_DK_CHANNEL_RACK) {
            // VoiceMap::UpdateMidiControl (VoiceMap.h:75-82): the voice at channel2voice[channel], alone
            if (ev[k].source != OLFX_CTL_MIDI && ev[k].source != OLFX_CTL_HARDWARE) return fail(OLFX_E_ARG, "olfx_control: event %u", k);
            const uint8_t p = ev[k].pad < 16 ? chan2voice[(size_t)ev[k].pad * n + ev[k].inst] : kNoVoice;
            if (p == kNoVoice) continue;                  // an empty entry, or no channel at all
            uint32_t f = 0;
            float v = 0.f;
            if (voice_cc(ev[k].control, CcValue{ev[k].source == OLFX_CTL_MIDI, ev[k].value, &f, &v}) != OLFX_OK) continue;
            if (f == OLFX_FIELD_UPDATE_ONLY) {
                configured[(size_t)p * n + ev[k].inst] = 1;
                mark_vdirty(p * n + ev[k].inst);
            } else if (const int r2 = set_range(ev[k].inst, 1, kd->voice0 + p * OLFX_VC_NPARAMS + f, 1, &v)) {
                return r2;
            }
            continue;
        }
        const uint32_t topology = kd->topo_field == kNoField ? 0u : (uint32_t)params[(size_t)kd->topo_field * n + ev[k].inst];
        uint32_t fields[2];
        float vals[2];
        const int hits = route_control(*kd, topology, ev[k].control, ev[k].source, ev[k].value, fields, vals);
        if (hits < 0) return fail(hits, "olfx_control: event %u", k);
        for (int h = 0; h < hits; ++h) {
            if (fields[h] == OLFX_FIELD_UPDATE_ONLY) {    // Update() with unchanged members (the voices': now configured)
                if (kd->takes_note_events() && !kit()) configured[ev[k].inst] = 1;
                mark_dirty(ev[k].inst, 1);
            } else if (const int r2 = set_range(ev[k].inst, 1, fields[h], 1, &vals[h])) {
                return r2;
            }
        }
    }
    return OLFX_OK;
}

int Shadow::note_events(const olfx_event *ev, uint32_t count) {
    if (!kd->takes_note_events()) return fail(OLFX_E_STATE, "olfx_note_events: not a voice engine");
    if (count && !ev) return fail(OLFX_E_ARG, "olfx_note_events: null events");
    for (uint32_t k = 0; k < count; ++k) {
        if (ev[k].inst >= n || ev[k].note > 127 || ev[k].type > OLFX_EV_GATE_OFF)
            return fail(OLFX_E_ARG, "olfx_note_events: bad event %u", k);
        if (kit() && ev[k].type > OLFX_EV_NOTE_ON)
            return fail(OLFX_E_ARG, "olfx_note_events: event %u: a drum kit takes NOTE_ON and NOTE_OFF only", k);
    }
    for (uint32_t k = 0; k < count; ++k) {
        if (kit()) route_kit(events, ev[k].inst, ev[k].type, ev[k].note, ev[k].velocity);
        else if (instruments()) route_synth(events, ev[k].inst, ev[k].type, ev[k].note, ev[k].velocity);
        else events.push_back(olfx_voice_event{ev[k].inst, ev[k].type, ev[k].note, ev[k].velocity, 0, 0.f});
    }
    return OLFX_OK;
}

int Shadow::voice_events(const olfx_voice_event *ev, uint32_t count) {
    if (!kd->takes_note_events()) return fail(OLFX_E_STATE, "olfx_voice_events: not a voice engine");
    if (count && !ev) return fail(OLFX_E_ARG, "olfx_voice_events: null events");
    for (uint32_t k = 0; k < count; ++k) {
        if (ev[k].inst >= n || ev[k].note > 127 || ev[k].type > OLFX_EV_SET_FREQUENCY ||
            (ev[k].type == OLFX_EV_SET_FREQUENCY && !std::isfinite(ev[k].value)))
            return fail(OLFX_E_ARG, "olfx_voice_events: bad event %u", k);
        if (kit() && ev[k].type > OLFX_EV_NOTE_ON)
            return fail(OLFX_E_ARG, "olfx_voice_events: event %u: a drum kit takes NOTE_ON and NOTE_OFF only", k);
    }
    if (kit()) {
        for (uint32_t k = 0; k < count; ++k) route_kit(events, ev[k].inst, ev[k].type, ev[k].note, ev[k].velocity);
        return OLFX_OK;
    }
    if (instruments()) {
        for (uint32_t k = 0; k < count; ++k) route_synth(events, ev[k].inst, ev[k].type, ev[k].note, ev[k].velocity);
        return OLFX_OK;
    }
    events.insert(events.end(), ev, ev + count);
    return OLFX_OK;
}

// ---- the timed calls: one discipline for the three pending lists (olfx_host.h) ----
int Shadow::bad_frame(const char *call, const char *what, uint32_t k, uint32_t frame) {
    if (!(frame & 3u) && frame < 0x80000000u) return OLFX_OK;
    return fail(OLFX_E_ARG, "%s: %s %u: frame %u (a multiple of 4 below 2^31)", call, what, k, frame);
}

namespace {

// `count` validated entries, entry(k) the k-th: one at frame 0 happens now (the untimed path: one order of arrival
// for both), the rest go onto the pending list, stably by frame and behind the queued ones of their frame -- both
// steps keep call order among ties
template <class T, class Entry, class Now>
void queue_by_frame(std::vector<T> &pending, size_t count, Entry &&entry, Now &&now) {
    const size_t old = pending.size();
    for (size_t k = 0; k < count; ++k) {
        const T x = entry(k);
        if (x.frame == 0u) now(x);
        else pending.push_back(x);
    }
    const auto by_frame = [](const T &x, const T &y) { return x.frame < y.frame; };
    std::stable_sort(pending.begin() + (ptrdiff_t)old, pending.end(), by_frame);
    std::inplace_merge(pending.begin(), pending.begin() + (ptrdiff_t)old, pending.end(), by_frame);
}

// After a launch of `span` frames: the pending frames count from the next launch, and the entries that reached
// frame 0 happen now, in order, and leave the list (`now` queues nothing onto it)
template <class T, class Now>
void shift_and_pop(std::vector<T> &pending, uint32_t span, Now &&now) {
    for (T &x : pending) x.frame = x.frame > span ? x.frame - span : 0u;
    size_t due = 0;
    for (; due < pending.size() && !pending[due].frame; ++due) now(pending[due]);
    pending.erase(pending.begin(), pending.begin() + (ptrdiff_t)due);
}

// The ascending union of the event times and the record times below `limit` (all past frame 0): per time,
// f(t, e0, e1, r0, r1) with that time's events [e0, e1) and records [r0, r1); f returns false to stop ahead of that
// time.  Returns the time it stopped at, or `limit`.
template <class R, class F>
uint32_t walk_times(const std::vector<olfx_timed_event> &ev, const std::vector<R> &rec, uint32_t limit, F &&f) {
    const uint32_t none = 0xFFFFFFFFu;
    for (size_t e = 0, r = 0;;) {
        const uint32_t te = e < ev.size() ? ev[e].frame : none, tr = r < rec.size() ? rec[r].frame : none;
        const uint32_t t = te < tr ? te : tr;
        if (t >= limit) return limit;
        size_t e1 = e, r1 = r;
        while (e1 < ev.size() && ev[e1].frame == t) ++e1;
        while (r1 < rec.size() && rec[r1].frame == t) ++r1;
        if (!f(t, e, e1, r, r1)) return t;
        e = e1;
        r = r1;
    }
}

// the lanes one time touches, each once and ascending (they mostly arrive that way)
void sort_unique(std::vector<uint32_t> &v) {
    if (!std::is_sorted(v.begin(), v.end())) std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
}

}  // namespace

int Shadow::timed_events(const olfx_timed_event *ev, uint32_t count) {
    if (!kd->takes_note_events()) return fail(OLFX_E_STATE, "olfx_timed_events: not a voice engine");
    // voice-addressed events; an instrument's notes are routed, at their frame: olfx_timed_notes
    if (instruments()) return fail(OLFX_E_KIND, "olfx_timed_events: the synth kinds and the drum kit take olfx_timed_notes");
    if (count && !ev) return fail(OLFX_E_ARG, "olfx_timed_events: null events");
    for (uint32_t k = 0; k < count; ++k) {
        const olfx_voice_event &v = ev[k].ev;
        if (const int rc = bad_frame("olfx_timed_events", "event", k, ev[k].frame)) return rc;
        if (v.inst >= n || v.note > 127 || v.type > OLFX_EV_SET_FREQUENCY ||
            (v.type == OLFX_EV_SET_FREQUENCY && !std::isfinite(v.value)))
            return fail(OLFX_E_ARG, "olfx_timed_events: bad event %u", k);
    }
    queue_by_frame(timed, count, [&](size_t k) { return ev[k]; }, [&](const olfx_timed_event &t) { events.push_back(t.ev); });
    return OLFX_OK;
}

// Timed notes of the synths and the drum kit.  A note is routed when the engine reaches its frame: a note at
// frame 0 here, as olfx_note_events routes it; a later one stays pending, unrouted (fold_segments, advance).
int Shadow::timed_notes(const olfx_timed_note *ev, uint32_t count) {
    if (!kd->takes_note_events()) return fail(OLFX_E_STATE, "olfx_timed_notes: not a synth or drum kit engine");
    if (!instruments()) return fail(OLFX_E_KIND, "olfx_timed_notes: the voice kinds take olfx_timed_events");
    if (count && !ev) return fail(OLFX_E_ARG, "olfx_timed_notes: null events");
    for (uint32_t k = 0; k < count; ++k) {
        const olfx_event &v = ev[k].ev;
        if (const int rc = bad_frame("olfx_timed_notes", "event", k, ev[k].frame)) return rc;
        if (v.inst >= n || v.note > 127 || v.type > OLFX_EV_GATE_OFF) return fail(OLFX_E_ARG, "olfx_timed_notes: bad event %u", k);
        if (kit() && v.type > OLFX_EV_NOTE_ON)
            return fail(OLFX_E_ARG, "olfx_timed_notes: event %u: a drum kit takes NOTE_ON and NOTE_OFF only", k);
    }
    queue_by_frame(
        timed, count,
        [&](size_t k) {
            return olfx_timed_event{ev[k].frame, olfx_voice_event{ev[k].ev.inst, ev[k].ev.type, ev[k].ev.note, ev[k].ev.velocity, 0, 0.f}};
        },
        [&](const olfx_timed_event &t) { route_note(events, t.ev); });
    return OLFX_OK;
}

// Timed parameter and control changes of the voice kinds.  A record at frame 0 is olfx_set_param / olfx_control
// now; a later one stays pending until the engine reaches its frame (fold_segments, advance).
void Shadow::apply_param(const olfx_timed_param &r, bool mark) {
    if (r.field != OLFX_FIELD_UPDATE_ONLY) store_param(r.field, r.inst, r.value);
    configured[r.inst] = 1;                               // a voice kind: every write implies Update()
    if (mark) mark_dirty(r.inst, 1);
}

int Shadow::queue_params(const olfx_timed_param *rec, size_t count) {
    queue_by_frame(tparams, count, [&](size_t k) { return rec[k]; }, [&](const olfx_timed_param &r) { apply_param(r, true); });
    return OLFX_OK;
}

int Shadow::timed_params(const olfx_timed_param *rec, uint32_t count) {
    if (kd->instances != KindDesc::VOICES) return fail(OLFX_E_KIND, "olfx_timed_params: the three voice kinds only");
    if (count && !rec) return fail(OLFX_E_ARG, "olfx_timed_params: null records");
    for (uint32_t k = 0; k < count; ++k) {
        if (const int rc = bad_frame("olfx_timed_params", "record", k, rec[k].frame)) return rc;
        if (rec[k].inst >= n || rec[k].field >= n_params) return fail(OLFX_E_ARG, "olfx_timed_params: record %u out of range", k);
        if (const char *why = bad_value(rec[k].field, rec[k].value)) return fail(OLFX_E_ARG, "olfx_timed_params: record %u: %s", k, why);
    }
    return queue_params(rec, count);
}

int Shadow::timed_control(const struct olfx_timed_control *rec, uint32_t count) {
    if (kd->instances != KindDesc::VOICES) return fail(OLFX_E_KIND, "olfx_timed_control: the three voice kinds only");
    if (count && !rec) return fail(OLFX_E_ARG, "olfx_timed_control: null records");
    // a voice's controls map the same at every frame (no topology): mapped here, held as parameter records
    std::vector<olfx_timed_param> mapped;
    mapped.reserve(count);
    for (uint32_t k = 0; k < count; ++k) {
        const olfx_control_event &ev = rec[k].ev;
        if (const int rc = bad_frame("olfx_timed_control", "record", k, rec[k].frame)) return rc;
        if (ev.inst >= n) return fail(OLFX_E_ARG, "olfx_timed_control: record %u: instance out of range", k);
        uint32_t fields[2];
        float vals[2];
        const int hits = route_control(*kd, 0u, ev.control, ev.source, ev.value, fields, vals);
        if (hits < 0) return fail(OLFX_E_ARG, "olfx_timed_control: record %u", k);
        for (int h = 0; h < hits; ++h) {                  // (none: a control the reference ignores)
            if (fields[h] != OLFX_FIELD_UPDATE_ONLY)
                if (const char *why = bad_value(fields[h], vals[h])) return fail(OLFX_E_ARG, "olfx_timed_control: record %u: %s", k, why);
            mapped.push_back(olfx_timed_param{rec[k].frame, ev.inst, fields[h], vals[h]});
        }
    }
    return queue_params(mapped.data(), mapped.size());
}


// Timed parameter and control changes of the synths and the drum kit.  A record at frame 0 is olfx_set_param /
// olfx_control now; a later one stays pending, raw, until the engine reaches its frame (fold_segments, advance):
// a control is mapped there, under the instrument's topology and the kit's channel2voice of that moment.
bool Shadow::is_boundary(const TimedInst &r) const {
    if (r.ctl) return r.ev.control >= CC_DELAY_TIME && r.ev.control <= CC_DELAY_BALANCE && (!kit() || r.ev.pad == OLFX_DK_CHANNEL_RACK);
    if (kd->topo_field == kNoField || r.p.field < kd->topo_field - OLFX_FR_TOPOLOGY) return false;
    const uint32_t rf = r.p.field - (kd->topo_field - OLFX_FR_TOPOLOGY);
    return rf <= OLFX_FR_DELAY_RESONANCE || rf == OLFX_FR_TOPOLOGY;
}

void Shadow::apply_inst_now(const TimedInst &r) {
    // (validated when it was queued: neither call refuses it)
    if (r.ctl) (void)control(&r.ev, 1);
    else (void)set_range(r.p.inst, 1, r.p.field, 1, &r.p.value);
}

void Shadow::queue_inst(const std::vector<TimedInst> &recs) {
    queue_by_frame(iparams, recs.size(), [&](size_t k) { return recs[k]; }, [&](const TimedInst &r) { apply_inst_now(r); });
}

int Shadow::timed_instrument_params(const olfx_timed_param *rec, uint32_t count) {
    if (kd->instances == KindDesc::VOICES) return fail(OLFX_E_KIND, "olfx_timed_instrument_params: the voice kinds take olfx_timed_params");
    if (!instruments()) return fail(OLFX_E_STATE, "olfx_timed_instrument_params: not a synth or drum kit engine");
    if (count && !rec) return fail(OLFX_E_ARG, "olfx_timed_instrument_params: null records");
    std::vector<TimedInst> recs;
    recs.reserve(count);
    for (uint32_t k = 0; k < count; ++k) {
        if (const int rc = bad_frame("olfx_timed_instrument_params", "record", k, rec[k].frame)) return rc;
        if (rec[k].inst >= n || rec[k].field >= n_params) return fail(OLFX_E_ARG, "olfx_timed_instrument_params: record %u out of range", k);
        if (const char *why = bad_value(rec[k].field, rec[k].value))
            return fail(OLFX_E_ARG, "olfx_timed_instrument_params: record %u: %s", k, why);
        recs.push_back(TimedInst{rec[k].frame, false, rec[k], olfx_control_event{}});
    }
    queue_inst(recs);
    return OLFX_OK;
}

int Shadow::timed_instrument_control(const struct olfx_timed_control *rec, uint32_t count) {
    if (kd->instances == KindDesc::VOICES) return fail(OLFX_E_KIND, "olfx_timed_instrument_control: the voice kinds take olfx_timed_control");
    if (!instruments()) return fail(OLFX_E_STATE, "olfx_timed_instrument_control: not a synth or drum kit engine");
    if (count && !rec) return fail(OLFX_E_ARG, "olfx_timed_instrument_control: null records");
    std::vector<TimedInst> recs;
    recs.reserve(count);
    for (uint32_t k = 0; k < count; ++k) {
        const olfx_control_event &ev = rec[k].ev;
        if (const int rc = bad_frame("olfx_timed_instrument_control", "record", k, rec[k].frame)) return rc;
        if (ev.inst >= n) return fail(OLFX_E_ARG, "olfx_timed_instrument_control: record %u: instance out of range", k);
        // the mapping waits for the frame, so the record is judged under every mapping it can get there: a record
        // that olfx_control would refuse under one of them is refused now
        uint32_t fields[2];
        float vals[2];
        if (kit() && ev.pad != OLFX_DK_CHANNEL_RACK) {
            if (ev.source != OLFX_CTL_MIDI && ev.source != OLFX_CTL_HARDWARE) return fail(OLFX_E_ARG, "olfx_timed_instrument_control: record %u", k);
            if (voice_cc(ev.control, CcValue{ev.source == OLFX_CTL_MIDI, ev.value, &fields[0], &vals[0]}) == OLFX_OK &&
                fields[0] != OLFX_FIELD_UPDATE_ONLY)
                if (const char *why = bad_value(kd->voice0 + fields[0], vals[0]))
                    return fail(OLFX_E_ARG, "olfx_timed_instrument_control: record %u: %s", k, why);
        } else {
            for (uint32_t t = 0; t <= 4u; ++t) {
                if (!(kd->topologies >> t & 1)) continue;
                const int hits = route_control(*kd, t, ev.control, ev.source, ev.value, fields, vals);
                if (hits < 0) return fail(OLFX_E_ARG, "olfx_timed_instrument_control: record %u", k);
                for (int h = 0; h < hits; ++h)
                    if (fields[h] != OLFX_FIELD_UPDATE_ONLY)
                        if (const char *why = bad_value(fields[h], vals[h]))
                            return fail(OLFX_E_ARG, "olfx_timed_instrument_control: record %u: %s", k, why);
            }
        }
        recs.push_back(TimedInst{rec[k].frame, true, olfx_timed_param{}, ev});
    }
    queue_inst(recs);
    return OLFX_OK;
}

// olfx_set_param's bookkeeping (store_param, touched) with logs in place of the dirty lists
void Shadow::write_quiet(uint32_t inst, uint32_t field, float v) {
    store_param(field, inst, v);
    if (field >= kd->voice0 && field < kd->voice_end) {
        if (!kit()) {                                     // UpdateConfig + Update() of every voice of the instrument
            configured[inst] = 1;
            at_v.push_back(inst);
            changed_inst.push_back(inst);
            return;
        }
        const uint32_t p = (field - kd->voice0) / OLFX_VC_NPARAMS;
        if (p < voices) {                                 // (a slot past the kit's voices is read by nothing)
            configured[(size_t)p * n + inst] = 1;
            at_v.push_back(p * n + inst);
            changed_slot.push_back(p * n + inst);
        }
        return;
    }
    at_f.push_back(inst);
    changed_inst.push_back(inst);
}

// a voice kind's record: olfx_set_param of that voice, which implies Update()
void Shadow::apply_quiet(const olfx_timed_param &r) {
    apply_param(r, false);
    at_v.push_back(r.inst);
}

// Shadow::control's fan-out for one event, likewise
void Shadow::apply_quiet(const TimedInst &r) {
    if (!r.ctl) {
        write_quiet(r.p.inst, r.p.field, r.p.value);
        return;
    }
    const olfx_control_event &ev = r.ev;
    if (kit() && ev.pad != OLFX_DK_CHANNEL_RACK) {
        const uint8_t p = ev.pad < 16 ? chan2voice[(size_t)ev.pad * n + ev.inst] : kNoVoice;
        if (p == kNoVoice) return;
        uint32_t f = 0;
        float v = 0.f;
        if (voice_cc(ev.control, CcValue{ev.source == OLFX_CTL_MIDI, ev.value, &f, &v}) != OLFX_OK) return;
        if (f == OLFX_FIELD_UPDATE_ONLY) {
            configured[(size_t)p * n + ev.inst] = 1;
            at_v.push_back(p * n + ev.inst);
            changed_slot.push_back(p * n + ev.inst);
        } else {
            write_quiet(ev.inst, kd->voice0 + p * OLFX_VC_NPARAMS + f, v);
        }
        return;
    }
    const uint32_t topology = kd->topo_field == kNoField ? 0u : (uint32_t)params[(size_t)kd->topo_field * n + ev.inst];
    uint32_t fields[2];
    float vals[2];
    const int hits = route_control(*kd, topology, ev.control, ev.source, ev.value, fields, vals);
    for (int h = 0; h < hits; ++h) {
        if (fields[h] == OLFX_FIELD_UPDATE_ONLY) {        // Update() with unchanged members
            if (!kit()) {
                configured[ev.inst] = 1;
                at_v.push_back(ev.inst);
            }
            changed_inst.push_back(ev.inst);
        } else {
            write_quiet(ev.inst, fields[h], vals[h]);
        }
    }
}

uint32_t timed_instrument_cap(int kind, uint32_t n, uint32_t voices) {
    const KindDesc &kd = kind_desc(kind);
    if (kd.instances != KindDesc::INSTRUMENTS) return 0;
    return kd.voice_slots ? voices * n : n;
}

namespace {
constexpr size_t kEndsLaunch = ~(size_t)0;

// span() over the pending events and the kind's pending records: segment 0 starts at frame 0, events or none, and
// every later time takes a segment.  adds(r0, r1): the coefficient records that a time's records [r0, r1) add to
// the launch, of which it holds `cap`, or kEndsLaunch.
template <class R, class Adds>
uint32_t span_over(const std::vector<olfx_timed_event> &ev, const std::vector<R> &rec, uint32_t n_frames, size_t cap, Adds &&adds) {
    uint32_t segs = 1;
    size_t recs = 0;
    return walk_times(ev, rec, n_frames, [&](uint32_t, size_t, size_t, size_t r0, size_t r1) {
        if (segs == kSegCap) return false;
        if (r1 > r0) {
            const size_t c = adds(r0, r1);
            if (c == kEndsLaunch || recs + c > cap) return false;      // (never a launch's first time: c <= cap)
            recs += c;
        }
        ++segs;
        return true;
    });
}
}  // namespace

uint32_t Shadow::span(uint32_t n_frames) const {
    const bool notes = !timed.empty() && timed.front().frame < n_frames;
    if (!notes && !has_timed_params(n_frames) && !has_timed_inst(n_frames)) return n_frames;      // nothing past frame 0
    if (instruments()) {
        // a time's raw records, at most the cap (a time changes at most `cap` lanes, however many records); a
        // boundary record ends the launch ahead of its time: the next one starts there, with it at frame 0
        const size_t cap = timed_instrument_cap(kind, n, voices);
        return span_over(timed, iparams, n_frames, cap, [&](size_t r0, size_t r1) {
            for (size_t r = r0; r < r1; ++r)
                if (is_boundary(iparams[r])) return kEndsLaunch;
            return std::min(r1 - r0, cap);
        });
    }
    // a voice kind: a time adds a record per voice it changes (n records or fewer below the block: the bound cannot
    // bite, whatever voices they name)
    size_t below = 0;
    while (below <= n && below < tparams.size() && tparams[below].frame < n_frames) ++below;
    const bool count_voices = below > n;
    std::vector<uint32_t> at;
    return span_over(timed, tparams, n_frames, n, [&](size_t r0, size_t r1) {
        if (!count_voices) return (size_t)0;
        at.clear();
        for (size_t r = r0; r < r1; ++r) at.push_back(tparams[r].inst);
        sort_unique(at);
        return at.size();
    });
}

void Shadow::advance(uint32_t span_) {
    // parameter records first: at a frame they precede the events, and one that reaches frame 0 lands now, ahead of
    // anything set from now on; an instrument note that reaches frame 0 is routed now
    shift_and_pop(tparams, span_, [&](const olfx_timed_param &r) { apply_param(r, true); });
    shift_and_pop(iparams, span_, [&](const TimedInst &r) { apply_inst_now(r); });
    shift_and_pop(timed, span_, [&](const olfx_timed_event &t) {
        if (instruments()) route_note(events, t.ev);
        else events.push_back(t.ev);
    });
}

uint32_t Shadow::n_chunks(uint32_t span_, uint32_t chunk) const {
    uint32_t c = 0;
    for (size_t s = 0; s < seg_frame.size(); ++s)
        c += ((s + 1 < seg_frame.size() ? seg_frame[s + 1] : span_) - seg_frame[s] + chunk - 1) / chunk;
    return c;
}

// ol::synth::Polyvoice's calls on instrument `inst` (Polyvoice.h:35-77) as events of its voices (voice
// slot p * npad + inst).  Playing() changes here, at the call, as SynthVoice's does (SynthVoice.h:
// 245-260: NoteOn stores the note, NoteOff stores 0).  The reference's quirks follow from the same
// tests: NoteOn(0) leaves Playing() at 0, so the voice is gated yet still "free"; NoteOff(0) matches
// the first voice with Playing() == 0.
void Shadow::route_synth(std::vector<olfx_voice_event> &to, uint32_t inst, uint8_t type, uint8_t note, uint8_t velocity) {
    auto push = [&](uint32_t p) {
        to.push_back(olfx_voice_event{p * npad + inst, type, note, velocity, 0, 0.f});
    };
    uint8_t *pl = playing.data() + inst;                 // voice p: pl[p * n]
    switch (type) {
    case OLFX_EV_NOTE_ON:
        for (uint32_t p = 0; p < voices; ++p)
            if (!pl[(size_t)p * n]) {
                push(p);
                pl[(size_t)p * n] = note;
                break;
            }
        break;                                            // none free: dropped
    case OLFX_EV_NOTE_OFF:
        for (uint32_t p = 0; p < voices; ++p)
            if (pl[(size_t)p * n] == note) {
                push(p);
                pl[(size_t)p * n] = 0;
                break;
            }
        break;
    case OLFX_EV_GATE_ON:
    case OLFX_EV_GATE_OFF:
        for (uint32_t p = 0; p < voices; ++p) push(p);
        break;
    default: break;                                       // SetFrequency: a nop (Polyvoice.h:77)
    }
}

// ol::synth::VoiceMap's NoteOn / NoteOff on kit `inst` (VoiceMap.h:27-43): the voice at note2voice[note] gets the
// call, a note nobody sits at is ignored.  Playing() as in route_synth.
void Shadow::route_kit(std::vector<olfx_voice_event> &to, uint32_t inst, uint8_t type, uint8_t note, uint8_t velocity) {
    const uint8_t p = note2voice[(size_t)note * n + inst];
    if (p == kNoVoice) return;
    to.push_back(olfx_voice_event{p * npad + inst, type, note, velocity, 0, 0.f});
    playing[(size_t)p * n + inst] = type == OLFX_EV_NOTE_ON ? note : 0;
}

int Shadow::drumkit_map(const olfx_drumkit_voice *recs, uint32_t count) {
    if (!kit()) return fail(OLFX_E_STATE, "olfx_drumkit_map: not a drum kit engine");
    if (count && !recs) return fail(OLFX_E_ARG, "olfx_drumkit_map: null records");
    for (uint32_t k = 0; k < count; ++k) {
        const olfx_drumkit_voice &r = recs[k];
        if (r.kit >= n) return fail(OLFX_E_ARG, "olfx_drumkit_map: record %u: kit out of range", k);
        if (r.voice != OLFX_DK_NO_VOICE && r.voice >= voices)
            return fail(OLFX_E_ARG, "olfx_drumkit_map: record %u: voice %u of %u", k, r.voice, voices);
        if (r.note != OLFX_DK_NO_NOTE && r.note > 127) return fail(OLFX_E_ARG, "olfx_drumkit_map: record %u: note out of range", k);
        if (r.channel != OLFX_DK_NO_CHANNEL && r.channel > 15)
            return fail(OLFX_E_ARG, "olfx_drumkit_map: record %u: channel out of range", k);
    }
    // apply in order, remembering what each write replaced; judge the result; undo on refusal
    struct Undo { uint8_t *at; uint8_t was; };
    std::vector<Undo> undo;
    std::vector<uint32_t> kits;
    auto put = [&](uint8_t &slot, uint8_t v) {
        undo.push_back(Undo{&slot, slot});
        slot = v;
    };
    for (uint32_t k = 0; k < count; ++k) {
        const olfx_drumkit_voice &r = recs[k];
        const uint8_t v = r.voice == OLFX_DK_NO_VOICE ? kNoVoice : (uint8_t)r.voice;
        if (r.note != OLFX_DK_NO_NOTE) put(note2voice[(size_t)r.note * n + r.kit], v);
        if (r.channel != OLFX_DK_NO_CHANNEL) put(chan2voice[(size_t)r.channel * n + r.kit], v);
        kits.push_back(r.kit);
    }
    std::sort(kits.begin(), kits.end());
    kits.erase(std::unique(kits.begin(), kits.end()), kits.end());
    for (const uint32_t i : kits) {
        uint32_t seen = 0;
        for (uint32_t note = 0; note < 128; ++note) {
            const uint8_t v = note2voice[(size_t)note * n + i];
            if (v == kNoVoice) continue;
            if (seen >> v & 1u) {
                // the reference would tick the voice twice per frame (as a voice listed twice, olfx_mix_config)
                for (size_t u = undo.size(); u-- > 0;) *undo[u].at = undo[u].was;
                return fail(OLFX_E_ARG, "olfx_drumkit_map: voice %u of kit %u would sit at two notes", (unsigned)v, i);
            }
            seen |= 1u << v;
        }
    }
    for (const uint32_t i : kits) mark_dirty(i, 1);       // the sum order
    return OLFX_OK;
}

int Shadow::synth_playing(uint32_t inst, uint8_t *out) {
    if (!instruments()) return fail(OLFX_E_STATE, "olfx_synth_playing: not a synth engine");
    if (inst >= n || !out) return fail(OLFX_E_ARG, "olfx_synth_playing: bad argument");
    for (uint32_t p = 0; p < voices; ++p) out[p] = playing[(size_t)p * n + inst];
    return OLFX_OK;
}

// ---------------------------------------------------------------------------------------------
// The control packet (parameters and note events at the block boundary; JUCE-host pattern,
// modules/juce/host/host.cpp:646-653)
// ---------------------------------------------------------------------------------------------
namespace {
// daisysp::mtof of a MIDI note, from a table of the same expression (notes are 0..127; one powf
// per NoteOn had been the largest host cost of a block with note events)
float mtof_note(uint8_t note) {
    static const std::array<float, 128> t = [] {
        std::array<float, 128> r{};
        for (int k = 0; k < 128; ++k) r[(size_t)k] = powf(2.f, ((float)k - 69.0f) / 12.0f) * 440.0f;
        return r;
    }();
    return t[note & 127u];
}
}  // namespace

// The block's note events, one record per voice, in order of first appearance (VEV_*,
// olfx_layout.h).  Calls on one voice compose field by field, as their in-order application does
// (SynthVoice.h:231-268): NoteOn = GateOn + freq_ = mtof(note) + Retrigger(true) on both
// envelopes (:245-251); NoteOff / GateOff = gate off (:236-239, :253-256); GateOn = gate on
// (:231-234); SetFrequency = freq_ (:264-267).  The last gate call decides the gate, any NoteOn
// retriggers (gate calls do not touch the envelope modes), the last NoteOn / SetFrequency the pitch.
// Sample voices: SynthVoice::GateOn / GateOff also reach the sound source (SynthVoice.h:231-239), where
// GateOn = Seek(0) + Play() and GateOff = Pause() (SampleSoundSource.h:21-26): any NoteOn / GateOn of
// the block seeks to 0 (VEV_SEEK), and `playing` follows the last gate call like the gate itself.
void Shadow::fold_events() {
    folded.clear();
    ev_count.clear();
    ev_more.clear();
    n_more = 0;
    seg_frame.assign(1, 0u);
    seg_first.assign(1, 0u);
    fold_one(events.data(), events.size(), sizeof(olfx_voice_event));
    events.clear();
    seg_first.push_back((uint32_t)folded.size());
}

// Timed events: every segment folds on its own, as the queue of a block that started at its frame would.
// Timed records (a voice kind's tparams, an instrument kind's iparams): a time's records are applied to the shadow
// here, in queueing order -- an instrument's control mapped there -- and ahead of that time's events.  Every voice
// (a synth: instrument; a kit: voice slot) whose voice fields they touch gets one voice record for the segment
// (derive_voice on the shadow as that time leaves it), every instrument whose rack fields they touch one rack
// record.  A voice kind's voice has VEV_COEF in its folded record; an instrument kind's tables say who has one.
// The dirty records are derived first, as frame 0 has them: fill_records runs after this fold and would see the
// later values.
template <class R>
void Shadow::fold_with(std::vector<R> &pending, uint32_t span_) {
    const bool recs = !pending.empty() && pending.front().frame < span_;
    vrec.clear();
    frec.clear();
    pre_valid = fold_fresh = recs;
    if (recs) {
        const size_t m = dirty_list.size(), W = kd->words, m2 = vdirty_list.size(), W2 = kd->vwords;
        pre_words.resize(m * W);
        for (size_t r = 0; r < m; ++r) derive_record(m == n ? (uint32_t)r : dirty_list[r], pre_words.data() + r * W);
        pre_vwords.resize(m2 * W2);
        for (size_t r = 0; r < m2; ++r) derive_voice_record(vdirty_list[r], pre_vwords.data() + r * W2);
        vrec.open();
        frec.open();
        rack_full.clear();
        changed_inst.clear();
        changed_slot.clear();
    }
    fold_events();                                        // segment 0: the frame-0 queue
    size_t n_ev_done = 0, n_rec_done = 0;
    walk_times(timed, pending, span_, [&](uint32_t t, size_t e0, size_t e1, size_t r0, size_t r1) {
        seg_frame.push_back(t);
        at_v.clear();
        at_f.clear();
        for (size_t r = r0; r < r1; ++r) apply_quiet(pending[r]);
        sort_unique(at_v);
        sort_unique(at_f);
        float p[std::max<uint32_t>(OLFX_FR_NPARAMS, OLFX_VC_NPARAMS)];
        for (const uint32_t v : at_v) {                   // a voice, a synth's instrument, a kit's hv = slot * n + kit
            const uint32_t slot = kit() ? v / n : 0u, i = kit() ? v % n : v;
            for (uint32_t f = 0; f < OLFX_VC_NPARAMS; ++f) p[f] = params[(size_t)(kd->voice0 + slot * OLFX_VC_NPARAMS + f) * n + i];
            if (instruments()) last_v[v] = (int32_t)vrec.size();
            derive_voice(p, configured[v] != 0, kd->moog, sr, vrec.add(kit() ? slot * npad + i : i));
        }
        for (const uint32_t i : at_f) {
            const uint32_t rack0 = kd->topo_field - OLFX_FR_TOPOLOGY;
            uint32_t fw[FRC_N];
            for (uint32_t f = 0; f < OLFX_FR_NPARAMS; ++f) p[f] = params[(size_t)(rack0 + f) * n + i];
            derive_fxrack(p, sr, fw);
            last_f[i] = (int32_t)frec.size();
            std::memcpy(frec.add(i), fw + FRC_RBAL, (size_t)TIF_N * 4);
            rack_full.insert(rack_full.end(), fw, fw + FRC_N);
        }
        if (instruments()) {                              // routed now, against Playing() as the frames before left it
            routed.clear();
            for (size_t e = e0; e < e1; ++e) route_note(routed, timed[e].ev);
            fold_one(routed.data(), routed.size(), sizeof(olfx_voice_event));
        } else {
            fold_one(e1 > e0 ? &timed[e0].ev : nullptr, e1 - e0, sizeof(olfx_timed_event), at_v.data(), at_v.size());
        }
        seg_first.push_back((uint32_t)folded.size());
        if (recs) {
            vrec.close_segment();
            frec.close_segment();
        }
        n_ev_done = e1;
        n_rec_done = r1;
        return true;
    });
    timed.erase(timed.begin(), timed.begin() + (ptrdiff_t)n_ev_done);
    pending.erase(pending.begin(), pending.begin() + (ptrdiff_t)n_rec_done);
    if (recs && instruments()) keep_last_records();
}

void Shadow::fold_segments(uint32_t span_) {
    if (instruments()) fold_with(iparams, span_);
    else fold_with(tparams, span_);
}

// The whole last records of what an instrument fold changed: an instrument's (a slot's) latest voice record and
// latest rack record of the fold are its voice and rack words as the launch leaves them -- nothing is derived a
// second time; the parts no record of the fold covers are derived here.
void Shadow::keep_last_records() {
    const size_t W = kd->words, W2 = kd->vwords;
    sort_unique(changed_inst);
    sort_unique(changed_slot);
    changed_inst_words.resize(changed_inst.size() * W);
    float all[kMaxParams];
    for (size_t r = 0; r < changed_inst.size(); ++r) {
        const uint32_t i = changed_inst[r];
        uint32_t *w = changed_inst_words.data() + r * W;
        bool have = false;
        for (uint32_t j = 0; j < kd->nparts; ++j) {
            const Part &pt = kd->parts[j];
            const Component &c = kComponents[pt.comp];
            if (pt.comp == CP_VOICE && last_v[i] >= 0) {
                std::memcpy(w, vrec.words.data() + (size_t)last_v[i] * VCC_N, (size_t)VCC_N * 4);
            } else if (pt.comp == CP_RACK && last_f[i] >= 0) {
                std::memcpy(w, rack_full.data() + (size_t)last_f[i] * FRC_N, (size_t)FRC_N * 4);
            } else {
                if (!have)
                    for (uint32_t f = 0; f < n_params; ++f) all[f] = params[(size_t)f * n + i];
                have = true;
                c.derive(all + pt.field0, *this, i, w);
            }
            w += c.words;
        }
    }
    changed_slot_words.resize(changed_slot.size() * W2);
    for (size_t r = 0; r < changed_slot.size(); ++r) {    // (a listed slot has a voice record in this fold)
        const uint32_t hv = changed_slot[r];
        uint32_t *w = changed_slot_words.data() + r * W2;
        std::memcpy(w, vrec.words.data() + (size_t)last_v[hv] * VCC_N, (size_t)VCC_N * 4);
        sample_record(hv % n * voices + hv / n, w + VCC_N);
    }
    for (const uint32_t i : changed_inst) last_f[i] = -1;
    for (const uint32_t v : kit() ? changed_slot : changed_inst) last_v[v] = -1;
}

// `count` events `stride` bytes apart
void Shadow::fold_one(const olfx_voice_event *evs, size_t count, size_t stride, const uint32_t *coef, size_t n_coef) {
    const uint32_t seek = kd->has_sample ? (uint32_t)VEV_SEEK : 0u;
    const size_t first = folded.size();
    for (size_t c = 0; c < n_coef; ++c) {                 // (distinct voices) the events below join these records
        ev_slot[coef[c]] = (int32_t)folded.size();
        folded.push_back(Folded{coef[c], VEV_COEF, 0u, 0u});
    }
    for (size_t e = 0; e < count; ++e) {
        const olfx_voice_event &ev = *reinterpret_cast<const olfx_voice_event *>(reinterpret_cast<const char *>(evs) + e * stride);
        int32_t &k = ev_slot[ev.inst];
        if (k < 0) {
            k = (int32_t)folded.size();
            folded.push_back(Folded{ev.inst, 0u, 0u, 0u});
        }
        Folded &r = folded[(size_t)k];
        switch (ev.type) {
        case OLFX_EV_NOTE_ON: {
            r.op |= VEV_GATE_SET | VEV_GATE_ON | VEV_RETRIGGER | VEV_FREQ | seek;
            const float hz = mtof_note(ev.note);                              // daisysp::mtof
            std::memcpy(&r.freq, &hz, 4);
            break;
        }
        case OLFX_EV_GATE_ON: r.op |= VEV_GATE_SET | VEV_GATE_ON | seek; break;
        case OLFX_EV_SET_FREQUENCY:
            r.op |= VEV_FREQ;
            std::memcpy(&r.freq, &ev.value, 4);
            break;
        default: r.op = (r.op | VEV_GATE_SET) & ~VEV_GATE_ON; break;   // NoteOff / GateOff
        }
    }
    // records per workgroup (64 voices); crowded workgroups (more than kVevCap records) get a run
    // of the overflow list each, in group order
    const uint32_t groups = (n_ev() + 63u) / 64u;
    const size_t g0 = ev_count.size();                    // this segment's groups
    ev_count.resize(g0 + groups, 0u);
    for (size_t r = first; r < folded.size(); ++r) {
        ev_count[g0 + (folded[r].inst >> 6)]++;
        ev_slot[folded[r].inst] = -1;
    }
    ev_more.resize(g0 + groups, 0u);
    for (size_t g = g0; g < g0 + groups; ++g)
        if (ev_count[g] > kVevCap) {
            ev_more[g] = n_more;
            n_more += ev_count[g];
        }
}

// The folded records into a packet's event section (VoiceArgs::ev layout, olfx_internal.h):
// `fix` = [groups][kVevCap] 8-B slots, then the overflow list.  Segments (fold_segments): the slots of every
// segment, [n_seg][groups][kVevCap], one overflow list, and -- two segments or more -- their start frames.
void Shadow::write_events(uint32_t *fix) {
    const size_t groups = ev_count.size();                // every segment's
    std::memset(fix, 0, groups * kVevCap * 8);
    uint32_t *more = fix + groups * kVevCap * 2;
    ev_fill.assign(groups, 0u);
    const size_t per_seg = (n_ev() + 63u) / 64u;
    for (size_t sgm = 0; sgm + 1 < seg_first.size(); ++sgm)
        for (size_t f = seg_first[sgm]; f < seg_first[sgm + 1]; ++f) {
            const Folded &r = folded[f];
            const size_t g = sgm * per_seg + (r.inst >> 6);
            const uint32_t k = ev_fill[g]++;
            uint32_t *rec = ev_count[g] <= kVevCap ? fix + 2 * (g * kVevCap + k) : more + 2 * ((size_t)ev_more[g] + k);
            rec[0] = (r.inst & 63u) | r.op << 8;
            rec[1] = r.freq;
        }
    for (size_t g = 0; g < groups; ++g)
        if (ev_count[g] > kVevCap) {
            fix[2 * g * kVevCap] = VEV_MORE << 8 | ev_count[g] << 16;
            fix[2 * g * kVevCap + 1] = ev_more[g];
        }
    if (seg_frame.size() > 1) {
        uint32_t *tab = more + 2 * (size_t)n_more;
        for (size_t sgm = 0; sgm < seg_frame.size(); ++sgm) tab[sgm] = seg_frame[sgm];
        if (seg_frame.size() & 1u) tab[seg_frame.size()] = 0u;       // the section is whole 8-B records
    }
}

PacketPlan plan_packet(uint32_t n, size_t m, uint32_t W, bool evs, uint32_t n_more, uint32_t n_ev, size_t m2, uint32_t W2,
                       uint32_t n_seg, size_t n_tc, size_t n_iv, size_t n_if, uint32_t gv, uint32_t gf) {
    PacketPlan pl;
    pl.dense = m == n;                                   // every instance: no instance list
    pl.o_inst = 0;
    pl.o_val = pl.o_inst + (pl.dense ? 0 : up4(m));
    pl.o_ev = up4(pl.o_val + (size_t)W * m);
    if (m2) {                                            // a kit kind's voice-slot records
        pl.m2 = m2;
        pl.o_inst2 = pl.o_ev;
        pl.o_val2 = pl.o_inst2 + up4(m2);
        pl.o_ev = up4(pl.o_val2 + (size_t)W2 * m2);
    }
    pl.n_seg = n_seg ? n_seg : 1u;
    pl.words = pl.o_ev + (evs ? 2 * (pl.n_seg * (size_t)(((n_ev ? n_ev : n) + 63u) / 64u) * kVevCap + n_more) : 0);
    if (evs && pl.n_seg > 1) {                            // the segments' start frames
        pl.o_seg = pl.words;
        pl.words += (pl.n_seg + 1u) & ~(size_t)1u;
    }
    if (evs && pl.n_seg > 1 && n_tc) {                    // timed parameters: the base table, the records
        pl.n_tc = n_tc;
        pl.o_tcb = up4(pl.words);
        pl.o_tc = up4(pl.o_tcb + pl.n_seg * (size_t)(((n_ev ? n_ev : n) + 63u) / 64u));
        pl.words = pl.o_tc + (size_t)VCC_N * n_tc;
    }
    if (evs && pl.n_seg > 1 && n_iv + n_if) {             // timed instrument records: two tables, two record arrays
        pl.n_iv = n_iv;
        pl.n_if = n_if;
        pl.gv = gv;
        pl.gf = gf;
        pl.o_ivt = up4(pl.words);
        pl.o_ift = pl.o_ivt + 4 * pl.n_seg * (size_t)gv;
        pl.o_iv = pl.o_ift + 4 * pl.n_seg * (size_t)gf;
        pl.o_if = up4(pl.o_iv + (size_t)VCC_N * n_iv);
        pl.words = pl.o_if + (size_t)TIF_N * n_if;
    }
    return pl;
}

size_t max_timed_param_words(int kind, uint32_t n) {
    if (kind_desc(kind).instances != KindDesc::VOICES) return 0;
    // the section's alignment (up to 3 words), the base table of a full launch rounded up to the records', n records
    return 3 + up4((size_t)kSegCap * ((n + 63u) / 64u)) + (size_t)VCC_N * n;
}

size_t max_timed_instrument_words(int kind, uint32_t n, uint32_t voices) {
    const size_t cap = timed_instrument_cap(kind, n, voices);
    if (!cap) return 0;
    const size_t g = (n + 63u) / 64u, gv = kind_desc(kind).voice_slots ? voices * g : g;
    // the section's alignment, both tables of a full launch, `cap` voice records, alignment, `cap` rack records
    return 3 + 4 * (size_t)kSegCap * (gv + g) + (size_t)VCC_N * cap + 3 + (size_t)TIF_N * cap;
}

namespace {
// Per segment and 64-lane group of `rec`, in order: f(s, g, r0, r1), the group's run of records [r0, r1) (ascending
// lanes: a group's run starts where the group before it ends)
template <class Rec, class F>
void for_group_runs(const Rec &rec, size_t groups, F &&f) {
    for (size_t s = 0; s + 1 < rec.first.size(); ++s) {
        size_t r = rec.first[s];
        for (size_t g = 0; g < groups; ++g) {
            const size_t r0 = r;
            while (r < rec.first[s + 1] && (rec.lane[r] >> 6) == g) ++r;
            f(s, g, r0, r);
        }
    }
}
}  // namespace

void Shadow::write_timed_inst(const PacketPlan &pl, uint32_t *buf) const {
    // a table: per segment and group, the lanes that have a record and the number of the first
    auto table = [&](uint32_t *tab, size_t groups, const auto &rec) {
        std::memset(tab, 0, 4 * pl.n_seg * groups * 4);
        for_group_runs(rec, groups, [&](size_t s, size_t g, size_t r0, size_t r1) {
            uint32_t *e = tab + 4 * (s * groups + g);
            e[2] = (uint32_t)r0;
            for (size_t r = r0; r < r1; ++r) e[(rec.lane[r] & 63u) >> 5] |= 1u << (rec.lane[r] & 31u);
        });
    };
    table(buf + pl.o_ivt, pl.gv, vrec);
    table(buf + pl.o_ift, pl.gf, frec);
    vrec.write_field_major(buf + pl.o_iv);
    for (size_t w = pl.o_iv + (size_t)VCC_N * pl.n_iv; w < pl.o_if; ++w) buf[w] = 0u;
    frec.write_field_major(buf + pl.o_if);
}

void Shadow::write_timed_coefs(const PacketPlan &pl, uint32_t *buf) const {
    const size_t groups = (n_ev() + 63u) / 64u;
    uint32_t *base = buf + pl.o_tcb;
    for_group_runs(vrec, groups, [&](size_t s, size_t g, size_t r0, size_t) { base[s * groups + g] = (uint32_t)r0; });
    vrec.write_field_major(buf + pl.o_tc);
}

size_t max_packet_words(int kind, uint32_t n_inst, uint32_t n_ev, uint32_t n_seg) {
    const size_t n = n_inst, W = coef_segments(kind).total(), nv = n_ev ? n_ev : n_inst;
    // (timed events: a launch's segments and their start frames)
    const size_t segs = n_seg ? n_seg : 1;
    const size_t ev = takes_note_events(kind) ? 2 * segs * ((nv + 63) / 64 * kVevCap + nv) + (segs > 1 ? segs : 0) : 0;
    // a kit kind: every voice slot's list entry and record as well (n_ev = voices x n rounded up to 64)
    const KindDesc &kd = kind_desc(kind);
    const size_t nslots = kd.voice_slots ? nv / ((n + 63) / 64 * 64) * n : 0;
    return n + W * n + nslots * (1 + kd.vwords) + ev + (nslots ? 24 : 16);
}

// the words psv depends on (chorus_stage_rf.h): the pitch phasor's increment and the window
static const uint32_t kPitchWords[4] = {CHC_PS_INC, CHC_PS_INC_LO, CHC_WINDOW, CHC_WINDOW_LO};

bool Shadow::ring_free_next() const {
    if (kind != OLFX_KIND_CHORUS || !rf.active()) return false;
    if (!rf.seen) return true;
    std::vector<uint32_t> w(kd->words);
    for (const uint32_t i : dirty_list) {
        derive_record(i, w.data());
        for (uint32_t k = 0; k < 4; ++k)
            if (w[kPitchWords[k]] != pitch_sent[(size_t)k * n + i]) return false;
    }
    return true;
}

void Shadow::fill_records(const PacketPlan &pl, uint32_t *buf) {
    // the dirty instances' records, then a kit kind's dirty voice slots' (listed by device slot p * npad + kit):
    // frame 0's where a fold derived them ahead of its records
    const size_t m = dirty_list.size();
    const uint32_t W = kd->words, W2 = kd->vwords;
    h_words.resize(std::max(W, W2));
    bool pitch_changed = false;
    for (size_t r = 0; r < m; ++r) {
        const uint32_t i = pl.dense ? (uint32_t)r : dirty_list[r];
        if (!pl.dense) buf[pl.o_inst + r] = i;
        if (pre_valid) std::memcpy(h_words.data(), pre_words.data() + r * W, (size_t)W * 4);
        else derive_record(i, h_words.data());
        if (kind == OLFX_KIND_CHORUS)
            for (uint32_t k = 0; k < 4; ++k) {
                uint32_t &sent = pitch_sent[(size_t)k * n + i];
                pitch_changed |= sent != h_words[kPitchWords[k]];
                sent = h_words[kPitchWords[k]];
            }
        for (uint32_t w = 0; w < W; ++w) buf[pl.o_val + (size_t)w * m + r] = h_words[w];
    }
    for (size_t r = 0; r < pl.m2; ++r) {
        const uint32_t hv = vdirty_list[r];
        buf[pl.o_inst2 + r] = hv / n * npad + hv % n;
        if (pre_valid) std::memcpy(h_words.data(), pre_vwords.data() + r * W2, (size_t)W2 * 4);
        else derive_voice_record(hv, h_words.data());
        for (uint32_t w = 0; w < W2; ++w) buf[pl.o_val2 + (size_t)w * pl.m2 + r] = h_words[w];
    }
    pre_valid = false;
    for (const uint32_t i : dirty_list) dirty_mark[i] = 0;
    dirty_list.clear();
    for (const uint32_t hv : vdirty_list) vdirty_mark[hv] = 0;
    vdirty_list.clear();
    // the previous launch's kept records have served (nothing to do where there are none)
    kept_voice.forget_all();
    kept_inst.forget_all();
    kept_slot.forget_all();
    // what the fold's records changed stays dirty, with its last record kept: the device arrays get it ahead of the
    // next launch (the kernels never write the coefficient arrays).  Once per fold: a later packet without a fold of
    // its own must not see this launch's records again
    if (fold_fresh && instruments()) {
        for (const uint32_t i : changed_inst) mark_dirty(i, 1);
        for (const uint32_t hv : changed_slot) mark_vdirty(hv);
        kept_inst.keep(changed_inst, changed_inst_words);
        kept_slot.keep(changed_slot, changed_slot_words);
        changed_inst.clear();
        changed_slot.clear();
    } else if (fold_fresh) {
        for (const uint32_t v : vrec.lane) mark_dirty(v, 1);
        kept_voice.keep(vrec.lane, vrec.words);
    }
    fold_fresh = false;
    if (pitch_changed && rf.changed()) rf_materialise = true;
}

}  // namespace host
}  // namespace olfx

// =============================================================================================
// C-ABI: the one entry point that needs no engine
// =============================================================================================
// A kind's control table as it stands, without topology routing: its parts' tables (route_control at topology 0)
extern "C" int olfx_control_map(int kind, uint8_t control, int source, float value, uint32_t *field, float *param_value) {
    using namespace olfx::host;
    if (!field || !param_value || (source != OLFX_CTL_MIDI && source != OLFX_CTL_HARDWARE)) return OLFX_E_ARG;
    const KindDesc &kd = kind_desc(kind);
    // the synths' controls can hit two fields: olfx_synth_control_map / olfx_synth_control_map_at; the drum
    // kit's need a channel
    if (kd.instances == KindDesc::INSTRUMENTS || kd.no_controls) return OLFX_E_KIND;
    uint32_t f[2];
    float v[2];
    const int hits = route_control(kd, 0u, control, source, value, f, v);
    if (hits <= 0) return hits ? hits : OLFX_IGNORED;
    *field = f[0];
    *param_value = v[0];
    return OLFX_OK;
}

// handleMidi's fan-out (main.cpp:201-207): the voices' handler, then the rack's at topology 1 as
// olfx_control routes it (route_control)
extern "C" int olfx_synth_control_map(uint8_t control, int source, float value, uint32_t field[2], float param_value[2]) {
    return olfx_synth_control_map_at(OLFX_KIND_SYNTH, 1u, control, source, value, field, param_value);
}

// The same for either synth kind at a rack topology the kind accepts: the kind's voice table, then the
// rack's as olfx_control routes an OLFX_KIND_FXRACK instance of that topology
extern "C" int olfx_synth_control_map_at(int kind, uint32_t topology, uint8_t control, int source, float value,
                                         uint32_t field[2], float param_value[2]) {
    using namespace olfx::host;
    const KindDesc &kd = kind_desc(kind);
    // (a drum kit routes by channel: the voice kind's map for a voice, the rack kind's for the rack)
    if (kd.instances != KindDesc::INSTRUMENTS || kd.voice_slots) return OLFX_E_KIND;
    if (!field || !param_value || (source != OLFX_CTL_MIDI && source != OLFX_CTL_HARDWARE)) return OLFX_E_ARG;
    if (topology > 4u || !(kd.topologies >> topology & 1)) return OLFX_E_ARG;
    return route_control(kd, topology, control, source, value, field, param_value);
}
