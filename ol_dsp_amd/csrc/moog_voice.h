// ol_dsp_amd/csrc/moog_voice.h -- the per-sample arithmetic of the MoogFilter SynthVoice
// (SynthVoice(OscillatorSoundSource, MoogFilter), ol_daisy/app/synth/main.cpp:49-52), shared by the
// voice kernel (voice.hip voice_block_v4) and the fused synth (synth.hip synth_block_v1), so both run
// the same operations in the same order:
//   moog_amp_tick : amp envelope, portamento, the polyBLEP saw        -> (src * drive, amp)
//   moog_cut_tick : filter envelope, cutoff sum, LadderFilter::SetFreq -> (alpha, Qadjust)
//   ladder_tick   : LadderFilter::Process (4x oversampled, LP24), x amp
// Everything is forced inline: a tick is compiled into its kernel exactly as when it was written
// there (voice_roles.h does the same for the Svf voice's roles).
//
// Contraction.  The voice's continuous stages are contracted into FMAs where the firmware's
// compiler would contract a * b + c (GCC's default -ffp-contract=fast in GNU C++): the polyBLEP
// quadratics, Svf::SetFreq's sine polynomial and damping limit, the Svf's low/band updates, the
// ladder's stages, feedback sum and SetAlpha polynomials.  Not the envelope updates, the
// portamento or the phase accumulator (their segment ends and the phase wrap are discontinuous:
// contracting them moved a segment end or a wrap by a sample, up to 2.8e-2 from the unfused
// oracle) nor the Svf's notch (2.7e-5 on a default-parameter voice).  Measured on the CPU
// restatement, the contracted stages together stay < 2e-6 from the unfused oracle; the voice's
// parity tolerance is 1e-5 of max(|ref|, rms) (tests/test_gpu_parity.py).  MI355X: the Svf voice
// 0.0358 -> 0.0333 ms, the Moog voice 0.1226 -> 0.0664 ms (32,768 voices, same box).
#pragma once
#include "voice_roles.h"

namespace olfx {
namespace {

// polyBLEP residual with one division: t/dt near the wrap start, (t-1)/dt near its end -- the
// same quotients as the two-branch form; q + q - q q - 1 and q q + q + q + 1 as
// fma(-q, q, 2q) - 1 and fma(q, q, 2q) + 1
__device__ __forceinline__ float polyblep(float dt, float t) {
    const bool lo = t < dt, hi = t > 1.0f - dt;                          // (lo wins the select)
    const float q = (lo ? t : t - 1.0f) * __builtin_amdgcn_rcpf(dt);   // v_rcp: ~1 ulp
    const float q2 = q + q;
    float rlo = __builtin_fmaf(-q, q, q2) - 1.0f;
    float rhi = __builtin_fmaf(q, q, q2) + 1.0f;
    asm volatile("" : "+v"(rlo), "+v"(rhi));      // both computed: selects, not an exec-mask diamond
    return lo ? rlo : (hi ? rhi : 0.0f);
}

// Oscillator::Process's saw, WAVE_POLYBLEP_SAW with amp 0.5 (o = 2t - 1, o -= blep, o *= -1, o * amp):
// -((2t - 1) - blep) / 2 = fma(1/2, blep, 1/2 - t) -- 2t - 1 = 2 (t - 1/2) and the halving are
// exact scalings, so both forms round the same sum once (up to the sign of an exact zero)
__device__ __forceinline__ float saw_out(float t, float blep) { return __builtin_fmaf(0.5f, blep, 0.5f - t); }

struct Ladder {
    float z0[4], z1[4], old;
};

// SynthVoice.h:42-45 up to the filter's input: the amp envelope, Port::Process, Oscillator::SetFreq /
// Process, and LadderFilter::Process's input scaling
__device__ __forceinline__ float2 moog_amp_tick(Env &ea, float &port_z, float &phase, float freq, float amp_amt,
                                                float port_c, float inv_sr, float drive) {
    const float amp = ea.step() * amp_amt;
    // Port::Process (Portamento.h:218-221), Oscillator::SetFreq: inc = f * sr_recip
    port_z = freq + port_c * (port_z - freq);
    const float inc = port_z * inv_sr;
    // Oscillator::Process, WAVE_POLYBLEP_SAW
    const float src = saw_out(phase, polyblep(inc, phase));
    phase += inc;
    phase = phase > 1.0f ? phase - 1.0f : phase;
    return make_float2(src * drive, amp);   // ladder: Process's input scaling
}

// SynthVoice.h:46-47: the filter envelope and the cutoff sum, then LadderFilter::SetFreq -> SetAlpha
// (fc_max holds 1 / (4 sr), VCC_LADDER_WREC): alpha and Qadjust
__device__ __forceinline__ float2 moog_cut_tick(Env &ef, float fenv_amt, float cutoff, float fc_max) {
    float2 cd;
    const float fe = ef.step();
    const float fc_in = __builtin_fmaf(fe * 20000.0f, fenv_amt, cutoff);
    const float wc = fc_in * 2.0f * 3.1415927410125732f * fc_max;
    const float wc2 = wc * wc;
    // the same polynomials in Horner form
    cd.x = wc * __builtin_fmaf(__builtin_fmaf(__builtin_fmaf(-0.0202f, wc, 0.1381f), wc, -0.4324f), wc, 0.9892f);
    cd.y = __builtin_fmaf(__builtin_fmaf(-0.05f, wc2, -0.095f), wc2, __builtin_fmaf(0.0536f, wc, 1.006f));
    return cd;
}

// LadderFilter::Process on v = (input, amp, alpha, Qadjust), times amp (SynthVoice.h:48-52); K is
// VCC_LADDER_K.  Contracted (see Contraction above); the Pade tanh as r(med3(x, -3, 3)) (r(+-3) =
// +-1 exactly: the saturation, branch-free) with a hardware reciprocal
__device__ __forceinline__ float ladder_tick(Ladder &L, const float4 v, float K) {
    const float input = v.x, alpha = v.z, kq = K * v.w;
    const float fb0 = -0.5f * input, dold = L.old - input;
    float total = 0.0f;
#pragma unroll
    for (int os = 0; os < 4; ++os) {
        const float interp = 0.25f * (float)os;
        // the linear interpolation interp old + (1 - interp) input as
        // input + interp (old - input): one fma per oversample (os = 0: input)
        const float mixin = os == 0 ? input : __builtin_fmaf(interp, dold, input);
        float x = __builtin_fmaf(-(L.z1[3] + fb0), kq, mixin);
        x = __builtin_amdgcn_fmed3f(x, -3.0f, 3.0f);
        const float x2 = x * x;
        float u = (x * (27.0f + x2)) * __builtin_amdgcn_rcpf(__builtin_fmaf(9.0f, x2, 27.0f));
#pragma unroll
        for (int st = 0; st < 4; ++st) {
            float ft = __builtin_fmaf(u, 1.0f / 1.3f, __builtin_fmaf(0.3f / 1.3f, L.z0[st], -L.z1[st]));
            ft = __builtin_fmaf(ft, alpha, L.z1[st]);
            L.z1[st] = ft;
            L.z0[st] = u;
            u = ft;
        }
        total = __builtin_fmaf(u, 0.25f, total);
    }
    L.old = input;
    return total * v.y;
}

}  // namespace
}  // namespace olfx
