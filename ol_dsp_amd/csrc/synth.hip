// ol_dsp_amd/csrc/synth.hip -- a whole polyphonic instrument (voices, Polyvoice sum, effect rack) in
// one launch, gfx950, wave64.  One kernel template over the voice type, synth_block<SVF>, whose two
// instantiations go by the names olfx_kernel_name reports:
//
// synth_block_v1 = synth_block<false> (OLFX_KIND_SYNTH): the Daisy synth firmware's audio callback
// (ol_daisy/app/synth/main.cpp:78-86):
//
//   mono = 0; voice.Process(&mono);       Polyvoice over P x SynthVoice(OscillatorSoundSource, MoogFilter)
//   delay_fx.Process(&mono, &mono);       DelayFx<1>
//   stereo[0] = stereo[1] = mono;
//   reverb_fx.Process(stereo, stereo);    ReverbFx<2> over the ReverbSc stub
//   filter_fx.Process(stereo, stereo);    FilterFx<2> in place
//
// Per frame and instrument, every operation in fp32:
//   v[p]  = voice p: voice_block_v4's arithmetic, operation for operation (moog_voice.h)
//   mono  = 0.0f; mono += v[0]; ... mono += v[P-1]         Polyvoice.h:28-33, in that order from +0.0f
//   a     = DelayFx<1>::Process(mono)                       rack_delay_stage.h (fr::delay_stage_from)
//   b     = (a 0.8) balance + a (1 - balance)               ReverbFx over the stub, both channels equal
//   out 0 = FilterFx's Svf on b, out 1 = b                  (x 1.0f: the rack's topology 1 has no master)
// which is what voice_block_v4 + voice_mix + fxrack_block_v3 at OLFX_FR_TOPOLOGY 1 compute in three
// launches, bit for bit; the voice samples and the sum stay in LDS.
//
// synth_svf_block_v1 = synth_block<true> (OLFX_KIND_SYNTH_SVF): the library's own voice, SynthVoice(OscillatorSoundSource,
// SvfFilter), behind the same Polyvoice, into the rack at the instrument's topology:
//   v[p]  = voice p: voice_block_v5's arithmetic, operation for operation (svf_voice.h)
//   topology 1: as above
//   topology 0: FxRack<2>::Process (Fx.h:432-440) on the frame (mono, 0.0f): DelayFx<2> -> ReverbFx<2> ->
//               filter1 into the zeroed buf_c -> x master: out 0 = c0 master, out 1 = 0.0f master
// which is voice_block_v5 + voice_mix + fxrack_block_v3 with the sum in input channel 0 and zeros in
// channel 1.  The topology is per instrument: D and F select per lane (FRC_TOPO), so one wave may hold
// both.  (Channel 1's delay line reaches no output at either topology.)
//
// A workgroup owns 64 instruments (lane = instrument in every role but D) and runs seven single-role
// waves over LDS queues of 16-frame chunks, with the progress counters of lds_flags.h (no workgroup
// barrier after the first: the roles' trip counts differ):
//   waves 0..3 ("V0".."V3"): voice slots p = w and p = w + 4 of the 64 instruments, a sample's whole
//                            voice back to back in one lane (no hand-off inside a voice), both
//                            voices' state in registers for the whole block; a chunk of voice p goes
//                            to queue V [depth 2][P][16][64]; waves w >= P exit at once;
//   waves 4, 5 ("D0", "D1"): the delay stage, 32 instruments x 2 channel lanes each (the channel-1
//                            lane runs a delay line that no output reads: fr::delay_stage_from as it
//                            stands); its input callback forms the ordered sum from queue V (the Svf
//                            synth's channel-1 lane takes 0.0f at topology 0); `a` into queue A
//                            [depth 2][16][64]; D1 exits when the group's upper half holds no
//                            instrument, and nobody waits for it then;
//   wave 6 ("F"):            the stub reverb's balance mix, filter_fx / filter1, the output stores.
// The Svf voice keeps this mapping although it is about a quarter of the Moog voice's work: a wave64
// VALU instruction issues over four cycles, so a lane's dependent chain leaves no bubble to fill with a
// second wave, and a SIMD's time is its instruction total, which one voice per wave over eight waves
// would not change; eleven waves per workgroup would cap the kernel at 168 VGPRs where D needs more
// ("Svf synth").
// Counters (chunks, per workgroup): F_V0..3 published by V_w, F_R0/1 taken from queue V by D0/D1,
// F_D0/1 published by D0/D1, F_FIN taken by F.
//   V_w (chunk c) waits  F_R0, F_R1 + 2 > c                  (its queue-V buffer was taken)
//   D   (input c) waits  F_V_w > c for every w < min(P, 4)
//   D   (emit  c) waits  F_FIN + 2 > c                       (its queue-A buffer was taken)
//   F   (chunk c) waits  F_D0, F_D1 > c
// No deadlock: all waves of a workgroup are resident together (a workgroup is dispatched whole), and
// every wait is for a (stage, chunk) pair that precedes the waiter in the order "lower chunk first,
// then V < D input < D emit < F".  D's program order is input(0), input(1), emit(0), input(2),
// emit(1), ...: input(c + 1) before emit(c) needs V(c + 1), which needs D's input(c - 1) -- already
// done; emit(c) needs F(c - 2), which needs both D's emit(c - 2).  So the dependencies are
// well-founded and some role can always advance.  The voice type and the topology change what a role
// computes, not what it waits for: the argument holds for both kernels.  The spins are bounded all the
// same (kSySpinMax): a wave that gives up goes on with stale data instead of hanging the device.
// The grid is one workgroup per 64 instruments (not persistent): 63,040 B of LDS at P = 4, 95,808 B at 8.
// Bound: the voice waves' per-sample recurrence, one wave per SIMD ("Synth"); the
// Svf synth: the D role's chunk chain for P <= 4, the voice wave that runs two voices from P = 5 on
// (measured, "Svf synth").
#include "rack_delay_stage.h"
#include "svf_voice.h"
#include "lds_flags.h"

namespace olfx {

namespace {
constexpr int kSyVWaves = 4;                              // voice waves
constexpr int kSyThreads = (kSyVWaves + 3) * 64;          // + D0, D1, F
constexpr int kSyChunk = fr::kChunk;
constexpr int kSyQ = kSyChunk * 64;                       // floats of one (voice, chunk) or one queue-A buffer
constexpr int kSyDepthV = 2, kSyDepthA = 2;
constexpr int kSyFlags = 16;
constexpr uint32_t kSyMaxVoices = 8;
constexpr uint32_t kSySpinMax = 1u << 22;                 // x s_sleep(1): ~0.1 s, five orders above any real wait
enum { F_V0 = 0, F_R0 = kSyVWaves, F_R1, F_D0, F_D1, F_FIN };
constexpr size_t sy_lds_floats(uint32_t voices) {
    return 2 * (size_t)fr::kRegion + (size_t)kSyDepthV * voices * kSyQ + (size_t)kSyDepthA * kSyQ + kSyFlags +
           (size_t)kSyVWaves * 64 * 2;
}
static_assert(sy_lds_floats(kSyMaxVoices) * 4 < 160 * 1024, "LDS budget");
static_assert((2 * fr::kRegion) % 4 == 0, "16-byte aligned queues");

template <class Cond>
__device__ __forceinline__ void sy_wait(Cond &&cond) {
    for (uint32_t t = 0; !cond() && t < kSySpinMax; ++t) __builtin_amdgcn_s_sleep(1);
}

// One MoogFilter SynthVoice of this lane: voice_block_v4's feed and ladder roles in one lane.
struct SyVoice {
    float phase, port_z, freq;
    Env ea, ef;
    Ladder L;
    bool gate, gprev_a, gprev_f, set_freq;
};
// One SvfFilter SynthVoice of this lane: voice_block_v5's four roles in one lane.
struct SySvfVoice {
    float phase, port_z, freq;
    Env ea, ef;
    float low, band;
    bool gate, gprev_a, gprev_f, set_freq;
};
}  // namespace

// SVF: SvfFilter voices and the rack's topology per instrument, 0 or 1 (synth_svf_block_v1); else
// MoogFilter voices and topology 1 (synth_block_v1, the instruction stream it had as a plain kernel).
template <bool SVF>
__global__ __launch_bounds__(kSyThreads) void synth_block(SynthArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const uint32_t tid = threadIdx.x;
    const uint32_t wib = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const uint32_t lane = tid & 63u;
    const uint32_t n = a.n, nf = a.n_frames, P = a.voices;
    const uint32_t nchunks = (nf + kSyChunk - 1) / kSyChunk;
    const uint32_t g = blockIdx.x;                         // the group: instruments 64 g ..
    float *vq = lds + 2 * fr::kRegion;                     // voices -> delay   [kSyDepthV][P][16][64]
    float *aq = vq + (size_t)kSyDepthV * P * kSyQ;         // delay -> filter   [kSyDepthA][16][64]
    uint32_t *flags = (uint32_t *)(aq + kSyDepthA * kSyQ);
    uint2 *evslots = (uint2 *)(flags + kSyFlags);          // [kSyVWaves][64]
    if (tid < kSyFlags) flags[tid] = 0;
    __syncthreads();                                       // the only barrier
    const bool d1_on = g * 64u + 32u < n;                  // the group's upper half holds an instrument
    const uint32_t nvw = min(P, (uint32_t)kSyVWaves);

    if (wib < (uint32_t)kSyVWaves) {
        // ---------------- V: voice slots wib and wib + 4, lane = instrument ----------------
        if (wib >= nvw) return;
        const uint32_t i_raw = g * 64u + lane;
        // lanes past n mirror instrument n - 1 exactly (same state, coefficients and events), so their
        // stores write the values its own lane writes (as voice_block_v4's dead lanes)
        const uint32_t i = i_raw < n ? i_raw : n - 1;
        const uint32_t me = i - g * 64u;
        const uint32_t sn = P * a.npad;                    // voice slots: the state planes' stride
        const float *c = a.vc_coef;                        // the instrument's: shared by its voices
        float *s = a.vc_state;
        uint2 *evslot = evslots + wib * 64u;
        const bool two = wib + (uint32_t)kSyVWaves < P;

        const float amp_amt = c[VCC_AMP_AMT * n + i], port_c = c[VCC_PORT_COEF * n + i];
        const float inv_sr = c[VCC_INV_SR * n + i];
        const float cutoff = c[VCC_CUTOFF * n + i], fenv_amt = c[VCC_FENV_AMT * n + i];
        const float drive = c[VCC_DRIVE * n + i], fc_max = c[VCC_FC_MAX * n + i];
        const float K = c[VCC_LADDER_K * n + i];           // the Svf voice: VCC_DAMP_RES (the same word)
        SvfVoiceCoef kc{};
        if constexpr (SVF)                                 // as voice_role_env / voice_role_freq form them
            kc = SvfVoiceCoef{0.5f * amp_amt, port_c, inv_sr, cutoff, fenv_amt, fc_max, drive, K,
                              1.0f / (c[VCC_SR * n + i] * 2.0f)};

        auto load = [&](auto &v, uint32_t p) {
            const uint32_t si = p * a.npad + i;
            uint32_t flags0 = __float_as_uint(s[VCS_FLAGS * sn + si]);
            float xa0 = s[VCS_ENVA_X * sn + si], xf0 = s[VCS_ENVF_X * sn + si];
            const float freq_s = s[VCS_FREQ * sn + si];
            const VoiceEv ev = voice_event_of(a.ev, a.ev_more, evslot, lane, me, p * (a.npad >> 6) + g);
            apply_gate_events(ev, flags0, xa0, xf0);
            v.gate = (flags0 >> 8) & 1u;
            v.set_freq = (ev.op & VEV_FREQ) != 0u;
            v.freq = v.set_freq ? ev.freq : freq_s;
            v.phase = s[VCS_PHASE * sn + si];
            v.port_z = s[VCS_PORT_Z * sn + si];
            v.gprev_a = (flags0 >> 6) & 1u;
            v.gprev_f = (flags0 >> 7) & 1u;
            v.ea.begin(v.gate, v.gprev_a, flags0 & 7u, xa0, c[VCC_ATK_D0A * n + i], c[VCC_ATK_TGT_A * n + i],
                       c[VCC_DEC_D0A * n + i], c[VCC_REL_D0A * n + i], c[VCC_SUS_A * n + i]);
            v.ef.begin(v.gate, v.gprev_f, (flags0 >> 3) & 7u, xf0, c[VCC_ATK_D0F * n + i], c[VCC_ATK_TGT_F * n + i],
                       c[VCC_DEC_D0F * n + i], c[VCC_REL_D0F * n + i], c[VCC_SUS_F * n + i]);
            if constexpr (SVF) {
                v.low = s[VCS_LOW * sn + si];
                v.band = s[VCS_BAND * sn + si];
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    v.L.z0[k] = s[(VCS_LZ0 + k) * sn + si];
                    v.L.z1[k] = s[(VCS_LZ1 + k) * sn + si];
                }
                v.L.old = s[VCS_LOLD * sn + si];
            }
        };
        auto store = [&](const auto &v, uint32_t p) {
            const uint32_t si = p * a.npad + i;
            s[VCS_PHASE * sn + si] = v.phase;
            s[VCS_PORT_Z * sn + si] = v.port_z;
            s[VCS_ENVA_X * sn + si] = v.ea.x;
            s[VCS_ENVF_X * sn + si] = v.ef.x;
            s[VCS_FLAGS * sn + si] = __uint_as_float(v.ea.mode | v.ef.mode << 3 | (uint32_t)v.gprev_a << 6 |
                                                     (uint32_t)v.gprev_f << 7 | (uint32_t)v.gate << 8);
            if (v.set_freq) s[VCS_FREQ * sn + si] = v.freq;
            if constexpr (SVF) {
                s[VCS_LOW * sn + si] = v.low;
                s[VCS_BAND * sn + si] = v.band;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    s[(VCS_LZ0 + k) * sn + si] = v.L.z0[k];
                    s[(VCS_LZ1 + k) * sn + si] = v.L.z1[k];
                }
                s[VCS_LOLD * sn + si] = v.L.old;
            }
        };
        // the voice's samples of a chunk of m frames -> q[k * 64] (its column of queue V)
        auto run = [&](auto &v, float *q, uint32_t m) {
            auto tick = [&](uint32_t k) {
                if constexpr (SVF) {
                    q[k * 64u] = svf_voice_tick(v.ea, v.ef, v.port_z, v.phase, v.low, v.band, v.freq, kc);
                } else {
                    const float2 ab = moog_amp_tick(v.ea, v.port_z, v.phase, v.freq, amp_amt, port_c, inv_sr, drive);
                    const float2 cd = moog_cut_tick(v.ef, fenv_amt, cutoff, fc_max);
                    q[k * 64u] = ladder_tick(v.L, make_float4(ab.x, ab.y, cd.x, cd.y), K);
                }
            };
            if (m == (uint32_t)kSyChunk) {
#pragma unroll 4
                for (uint32_t k = 0; k < (uint32_t)kSyChunk; ++k) tick(k);
            } else {
                for (uint32_t k = 0; k < m; ++k) tick(k);
            }
        };

        std::conditional_t<SVF, SySvfVoice, SyVoice> va, vb;
        load(va, wib);
        if (two) load(vb, wib + kSyVWaves);
        else vb = va;                                      // (never run, never stored)
        for (uint32_t ck = 0; ck < nchunks; ++ck) {
            const uint32_t m = min((uint32_t)kSyChunk, nf - ck * kSyChunk);
            sy_wait([&] {
                return flag_get(flags + F_R0) + kSyDepthV > ck && (!d1_on || flag_get(flags + F_R1) + kSyDepthV > ck);
            });
            float *q = vq + (size_t)(ck % kSyDepthV) * P * kSyQ + lane;
            run(va, q + wib * kSyQ, m);
            if (two) run(vb, q + (wib + kSyVWaves) * kSyQ, m);
            flag_put(flags + F_V0 + wib, ck + 1);
        }
        store(va, wib);
        if (two) store(vb, wib + kSyVWaves);
    } else if (wib < (uint32_t)kSyVWaves + 2u) {
        // ---------------- D: the delay stage, per (instrument, channel) lane ----------------
        const uint32_t dw = wib - kSyVWaves;
        const uint32_t inst0 = g * 64u + 32u * dw;
        if (inst0 >= n) return;                            // D1 of a group whose upper half is empty
        const uint32_t col = 32u * dw + (lane >> 1);       // this lane's instrument within the group
        // FxRack<2>::Process runs on the frame (mono, 0.0f): the channel-1 lane of a topology-0 instrument
        bool ch1_zero = false;
        if constexpr (SVF)
            ch1_zero = (lane & 1u) != 0u && a.fr_coef[FRC_TOPO * n + min(inst0 + (lane >> 1), n - 1u)] == 0u;
        auto mono = [&](uint32_t f0, int Cx, float (&xv)[kSyChunk]) {
            if (Cx == 0) {                                 // past the block's end: nothing to wait for
#pragma unroll
                for (int k = 0; k < kSyChunk; ++k) xv[k] = 0.f;
                return;
            }
            const uint32_t ck = f0 / kSyChunk;
            sy_wait([&] {
                bool ok = true;
                for (uint32_t w = 0; w < nvw; ++w) ok = ok && flag_get(flags + F_V0 + w) > ck;
                return ok;
            });
            // Polyvoice::Process: mono = 0; mono += v[0]; ... mono += v[P-1]
            const float *q = vq + (size_t)(ck % kSyDepthV) * P * kSyQ + col;
            float m[kSyChunk];
#pragma unroll
            for (int k = 0; k < kSyChunk; ++k) m[k] = 0.0f;
            for (uint32_t p = 0; p < P; ++p) {
#pragma unroll
                for (int k = 0; k < kSyChunk; ++k) m[k] += q[p * kSyQ + k * 64];
            }
            flag_put(flags + F_R0 + dw, ck + 1);          // (the release waits for these reads)
#pragma unroll
            for (int k = 0; k < kSyChunk; ++k) {
                if constexpr (SVF) xv[k] = k < Cx && !ch1_zero ? m[k] : 0.f;
                else xv[k] = k < Cx ? m[k] : 0.f;
            }
        };
        auto put = [&](uint32_t ck, const float (&av)[kSyChunk]) {
            sy_wait([&] { return flag_get(flags + F_FIN) + kSyDepthA > ck; });
            float *q = aq + (ck % kSyDepthA) * kSyQ + col;
            if ((lane & 1u) == 0u) {                       // channel 0's at either topology (the even lane's own)
#pragma unroll
                for (int k = 0; k < kSyChunk; ++k) q[k * 64] = av[k];
            }
            flag_put(flags + F_D0 + dw, ck + 1);
        };
        fr::delay_stage_from(a.ring, a.fr_state, a.fr_coef, n, nf, a.t0, lds + dw * fr::kRegion, lane, inst0, mono, put);
    } else {
        // ---------------- F: the stub reverb's balance mix, filter_fx, the stores; lane = instrument ----------------
        const uint32_t i_raw = g * 64u + lane;
        const bool valid = i_raw < n;
        const uint32_t i = valid ? i_raw : n - 1;
        const float rbal = __uint_as_float(a.fr_coef[FRC_RBAL * n + i]);
        const float ffreq = __uint_as_float(a.fr_coef[FRC_FFREQ * n + i]);
        const float fdamp = __uint_as_float(a.fr_coef[FRC_FDAMP * n + i]);
        const float fdrive = __uint_as_float(a.fr_coef[FRC_FDRIVE * n + i]);
        const uint32_t ftype = a.fr_coef[FRC_FTYPE * n + i];
        const float master = __uint_as_float(a.fr_coef[FRC_MASTER * n + i]);   // 1.0f: topology 1 (derive_fxrack)
        // topology 0: FilterFx<2> writes channel 0 of the zeroed buf_c only, so out 1 = 0.0f x master
        bool fw = true;
        if constexpr (SVF) fw = a.fr_coef[FRC_TOPO * n + i] == 1u;
        float flow = __uint_as_float(a.fr_state[FRS_FLOW * n + i]);
        float fband = __uint_as_float(a.fr_state[FRS_FBAND * n + i]);
        float *const o0 = a.out + i, *const o1 = a.out + a.plane + i;
        for (uint32_t ck = 0; ck < nchunks; ++ck) {
            const uint32_t f0 = ck * kSyChunk;
            const uint32_t C = min((uint32_t)kSyChunk, nf - f0);
            sy_wait([&] { return flag_get(flags + F_D0) > ck && (!d1_on || flag_get(flags + F_D1) > ck); });
            const float *q = aq + (ck % kSyDepthA) * kSyQ + lane;
            float a0[kSyChunk];
#pragma unroll
            for (int k = 0; k < kSyChunk; ++k) a0[k] = q[k * 64];
            flag_put(flags + F_FIN, ck + 1);               // (the release waits for these reads)
#pragma unroll
            for (int k = 0; k < kSyChunk; ++k) {
                if ((uint32_t)k < C) {                     // C is wave-uniform
                    // ReverbFx over the ReverbSc stub (fxrack.hip): stereo[0] = stereo[1], so b1 = b0
                    const float vb = a0[k] * 0.8f;
                    const float b0 = (vb * rbal) + (a0[k] * (1 - rbal));
                    // FilterFx<2> in place: the Svf on channel 0, channel 1 keeps the reverb's output
                    const float c0 = fr::svf_tick(b0, ffreq, fdamp, fdrive, ftype, flow, fband);
                    if (valid) {
                        o0[(size_t)(f0 + k) * n] = c0 * master;
                        if constexpr (SVF) o1[(size_t)(f0 + k) * n] = (fw ? b0 : 0.0f) * master;
                        else o1[(size_t)(f0 + k) * n] = b0 * master;
                    }
                }
            }
        }
        if (valid) {
            a.fr_state[FRS_FLOW * n + i] = __float_as_uint(flow);
            a.fr_state[FRS_FBAND * n + i] = __float_as_uint(fband);
        }
    }
}

hipError_t launch_synth(const SynthArgs &a, hipStream_t s) {
    if (a.n == 0 || a.n_frames == 0) return hipSuccess;
    if ((a.n_frames & 3u) || (a.t0 & 1u) || a.t0 >= kFrMaxDelay || a.voices < 1u || a.voices > kSyMaxVoices ||
        a.npad != ((a.n + 63u) & ~63u) || a.plane < (uint64_t)a.n_frames * a.n)
        return hipErrorInvalidValue;
    // one workgroup per 64 instruments; its seven waves are dispatched together
    const dim3 grid(a.npad / 64u), block(kSyThreads);
    const size_t lds = sy_lds_floats(a.voices) * sizeof(float);
    if (a.svf) hipLaunchKernelGGL(synth_block<true>, grid, block, lds, s, a);
    else hipLaunchKernelGGL(synth_block<false>, grid, block, lds, s, a);
    return hipGetLastError();
}

}  // namespace olfx
