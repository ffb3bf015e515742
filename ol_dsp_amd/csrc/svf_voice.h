// ol_dsp_amd/csrc/svf_voice.h -- the per-sample arithmetic of the library's own voice,
// SynthVoice(OscillatorSoundSource, SvfFilter) (SynthVoice.h:41-53), for a lane that runs a whole voice
// by itself: the fused Svf synth (synth.hip synth_svf_block_v1) and, with the Sample in the oscillator's place,
// the drum kit (drumkit.hip drumkit_block_v1).  voice_block_v5 (voice.hip) spreads the
// same voice over four role waves; svf_voice_tick is its four roles' per-sample forms in one lane, built
// from the same pieces (voice_roles.h: Env::step, svf_fc, sin_quarter, neg_damp; moog_voice.h: polyblep,
// saw_out), operation for operation.  In the order the code runs them -- OSC in svf_voice_tick, which hands
// its sample to svf_voice_tick_src for the other three (OSC and ENV do not depend on each other):
//   OSC  : Port::Process, Oscillator::SetFreq / Process (WAVE_POLYBLEP_SAW, amp 0.5)
//   ENV  : amp = Adsr * (amp_env_amount / 2); fc = svf_fc(fma(Adsr * 20000, filter_env_amount, cutoff))
//   FREQ : Svf::SetFreq(fc): (-damp, fq) with sin_quarter and the hardware reciprocal
//   FILT : the two Svf passes, Low() * amp
// voice_block_v5's full chunks run ENV, OSC and FREQ in packed pairs and the envelopes speculatively;
// those are the same IEEE operations per sample (no contraction: -ffp-contract=off), which its own
// ragged-block tests hold it to, so the per-sample forms below give its bits for every block length.
// Everything is forced inline.
#pragma once
#include "moog_voice.h"

namespace olfx {
namespace {

// the voice's coefficients as the roles read them (VCC_*): amp_half = 0.5f * VCC_AMP_AMT (FILT's Low()
// halving folded in, an exact scaling), inv_2sr = 1.0f / (VCC_SR * 2.0f)
struct SvfVoiceCoef {
    float amp_half, port_c, inv_sr, cutoff, fenv_amt, fc_max, drive, damp_res, inv_2sr;
};

// The voice around a source sample `src` handed in: ENV, FREQ and FILT.  The sample voice (drumkit.hip) calls it
// with the Sample's frame: SynthVoice(SampleSoundSource<1>, SvfFilter) runs neither Port nor Oscillator.
__device__ __forceinline__ float svf_voice_tick_src(Env &ea, Env &ef, float &low, float &band, float src,
                                                    const SvfVoiceCoef &k) {
    // ---- ENV (voice_role_env) ----
    const float amp = ea.step() * k.amp_half;
    const float fe = ef.step();
    const float fc = svf_fc(__builtin_fmaf(fe * 20000.0f, k.fenv_amt, k.cutoff), k.fc_max);
    // ---- FREQ (voice_role_freq) ----
    const float fcn = fc * k.inv_2sr;
    const float arg = __builtin_fminf(fcn, 0.25f);
    const float s1 = sin_quarter(3.1415927410125732f * arg), fq = s1 + s1;
    const float lim = __builtin_amdgcn_rcpf(s1) - s1;     // 2 / fq - fq / 2 = 1 / s - s
    const float ndamp = neg_damp(k.damp_res, lim);
    // ---- FILT (voice_role_filt): contracted except the notch ----
    float notch = src + ndamp * band;
    low = __builtin_fmaf(fq, band, low);
    float high = notch - low;
    band = __builtin_fmaf(-((k.drive * band) * band), band, __builtin_fmaf(fq, high, band));
    const float low1 = low;
    notch = src + ndamp * band;
    low = __builtin_fmaf(fq, band, low);
    high = notch - low;
    band = __builtin_fmaf(-((k.drive * band) * band), band, __builtin_fmaf(fq, high, band));
    // Low() = 0.5 low1 + 0.5 low2, times amp: (low1 + low2) (amp / 2), the same rounding (halvings exact)
    return (low1 + low) * amp;
}

__device__ __forceinline__ float svf_voice_tick(Env &ea, Env &ef, float &port_z, float &phase, float &low, float &band,
                                                float freq, const SvfVoiceCoef &k) {
    // ---- OSC (voice_block_v5's role 1) ----
    port_z = freq + k.port_c * (port_z - freq);          // Port::Process (Portamento.h:218-221)
    const float inc = port_z * k.inv_sr;                  // Oscillator::SetFreq
    const float t = phase;                                // Oscillator::Process reads, then advances
    phase += inc;
    phase = phase > 1.0f ? phase - 1.0f : phase;
    return svf_voice_tick_src(ea, ef, low, band, saw_out(t, polyblep(inc, t)), k);
}

}  // namespace
}  // namespace olfx
