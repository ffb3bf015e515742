// ol_dsp_amd/csrc/platerack.hip -- the effect rack with the Dattorro plate as its reverb stage
// (OLFX_KIND_PLATERACK): delay -> plate -> filter in one launch, gfx950, wave64.
//
// Per frame and instance, every operation in fp32 and none contracted:
//   a    = DelayFx<2>::Process(in)                      Fx.h:193-206, the rack's delay stage
//   v    = Dattorro((a[0] + a[1]) / 2) -> (vL, vR)      ReverbFx.cpp:13-19, verb.cpp:258-325
//   b[i] = (v[i] * balance) + (a[i] * (1 - balance))    Fx.h:298
//   c    = FilterFx<2>::Process(b): the Svf on channel 0   Fx.h:88-108
//   out  = c * master_volume                            Fx.h:431-433
// Topology 0 is FxRack<2>::Process: buf_c[1] is never written, so output channel 1 is 0 * master.
// Topology 1 is the Daisy firmware callback (ol_daisy/app/synth/main.cpp:78-86): DelayFx<1> on
// channel 0, stereo[0] = stereo[1], the reverb, FilterFx<2> in place (channel 1 keeps b[1]), no
// master volume (the host derives master = 1.0f for it).
//
// A workgroup owns 64 instances and runs the stages as a pipeline of four single-role waves, one per
// SIMD (the fused chain's plan, chain.hip), over a persistent grid of groups:
//   waves 0, 1 ("D0", "D1"): the delay stage (rack_delay_stage.h), 32 instances x 2 channels each,
//                            input from HBM, `a` into queue 1;
//   wave 2 ("DT"):           the 64 plates (dt::rows_network), lane = instance; its input callback
//                            forms (a0 + a1) / 2 from queue 1, its output callback puts vL, vR into
//                            queue 2;
//   wave 3 ("F"):            lane = instance: the balance mix of queue 2's vL, vR with queue 1's dry
//                            a0, a1, filter1, master, output to HBM.
// Choice for the mix: the F role, not DT's output callback.  DT is the critical wave (the plate's 27
// taps, 256 VGPR + AGPRs): the mix there would add filter1's serial recurrence, its coefficients and
// the output stores to it, while the fourth SIMD idles.  F reads the dry signal from queue 1 itself:
// a queue-1 buffer is released by F (not by DT), so DT forwards nothing but its own two outputs.
//
// Queues are [ch][16 frames][64 instances] buffers in LDS with the progress counters of
// lds_flags.h (chunk numbers gc run on across the groups of a workgroup):
//   F_D0, F_D1  chunks published by D0 / D1     F_DT  chunks published by DT
//   F_FIN       chunks taken by F (both queues' buffers gc are free again)
//   D  (chunk gc) waits  F_FIN + kDepth1 > gc            (its buffer was taken)
//   DT (chunk gc) waits  F_D0, F_D1 > gc  and  F_FIN + kDepth2 > gc
//   F  (chunk gc) waits  F_DT > gc        (which implies F_D0, F_D1 > gc)
// Two things hold by construction:
//   * All four waves of a workgroup are resident together: __launch_bounds__(256, 1) and 104 KB of
//     LDS (< 160 KB) make the workgroup one CU's only one, and a workgroup's waves are dispatched
//     together.
//   * No role waits for a chunk whose producer needs the waiter to advance by more than the queue
//     depth: every wait above is for (stage, chunk) pairs that precede the waiter in the order
//     "lower chunk first, then D < DT < F" -- D(gc) needs F(gc - kDepth1), DT(gc) needs D(gc) and
//     F(gc - kDepth2), F(gc) needs DT(gc) -- so the dependencies are well-founded and some role can
//     always advance; a wave whose instances lie past n still publishes its chunks.
// Addressing follows fxrack.hip: a wave's 32 rack rings get their own buffer descriptor (16,384
// instances are a 6.3 GB ring), the plate's rings use 64-bit row bases (dattorro_stage.h).
// Bound: HBM ("Plate rack": 180.6 B per frame).
#include "rack_delay_stage.h"
#include "dattorro_stage.h"
#include "lds_flags.h"

namespace olfx {

namespace {
constexpr int kPrThreads = 256;               // 4 waves
constexpr int kPrQCh = 16 * 64 + 16;          // floats per channel of one queue buffer (chain.hip's padding)
constexpr int kPrQBuf = 2 * kPrQCh;           // one buffer: [ch][16 frames][64 instances]
constexpr int kDepth1 = 4;                    // queue 1 (a): D may run 4 chunks ahead of F
constexpr int kDepth2 = 3;                    // queue 2 (v): DT may run 3 chunks ahead of F
constexpr int kPrFlags = 8;
constexpr int kPrPreLds = (17 + 8) * 64 * 4;  // DT's pre-delay staging (dt::PreRow)
constexpr int kPrLds = 2 * fr::kRegion + (kDepth1 + kDepth2) * kPrQBuf + kPrFlags + kPrPreLds;
static_assert(kPrLds * 4 < 160 * 1024, "LDS budget");
enum { F_D0 = 0, F_D1, F_DT, F_FIN };
}  // namespace

__global__ __launch_bounds__(kPrThreads, 1) void platerack_block_v1(PlateRackArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int kChunk = 16;
    const uint32_t tid = threadIdx.x;
    const uint32_t wib = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const uint32_t lane = tid & 63u;
    const uint32_t n = a.n, nf = a.n_frames;
    const uint32_t nchunks = (nf + kChunk - 1) / kChunk;
    const uint32_t ngroups = (n + 63u) / 64u;              // 64 instances per group
    float *q1 = lds + 2 * fr::kRegion;                     // delay -> plate, filter   [kDepth1][2 ch][16][64]
    float *q2 = q1 + kDepth1 * kPrQBuf;                    // plate -> filter          [kDepth2][2 ch][16][64]
    uint32_t *flags = (uint32_t *)(q2 + kDepth2 * kPrQBuf);
    if (tid < kPrFlags) flags[tid] = 0;
    __syncthreads();                                       // the only barrier

    if (wib < 2) {
        // ---------------- D: the delay stage, per (instance, channel) lane ----------------
        for (uint32_t g = blockIdx.x, gi = 0; g < ngroups; g += gridDim.x, ++gi) {
            const uint32_t gc0 = gi * nchunks;
            const uint32_t inst0 = g * 64u + 32u * wib;
            const uint32_t qcol = (lane & 1u) * kPrQCh + 32u * wib + (lane >> 1);
            auto put = [&](uint32_t c, const float (&av)[kChunk]) {
                const uint32_t gc = gc0 + c;
                wait_for([&] { return flag_get(flags + F_FIN) + kDepth1 > gc; });   // buffer gc % kDepth1 free
                float *q = q1 + (gc % kDepth1) * kPrQBuf + qcol;
#pragma unroll
                for (int k = 0; k < kChunk; ++k) q[k * 64] = av[k];
                flag_put(flags + F_D0 + wib, gc + 1);
            };
            if (inst0 < n) {
                fr::delay_stage(a.ring, a.state, a.coef, a.in, a.plane, n, nf, a.t0, lds + wib * fr::kRegion, lane,
                                inst0, put);
            } else {
                // no instance in this half of the group: zeros for the plate's padding lanes
                float z[kChunk];
#pragma unroll
                for (int k = 0; k < kChunk; ++k) z[k] = 0.f;
                for (uint32_t c = 0; c < nchunks; ++c) put(c, z);
            }
        }
    } else if (wib == 2) {
        // ---------------- DT: the plate, lane = instance, queue 1 -> queue 2 ----------------
        float4 *const stage = (float4 *)(flags + kPrFlags);
        for (uint32_t g = blockIdx.x, gi = 0; g < ngroups; g += gridDim.x, ++gi) {
            const uint32_t gc0 = gi * nchunks;
            dt::rows_network<false>(
                a.d, g, lane, nf, stage,
                [&](uint32_t c, uint32_t, uint32_t, float (&xm)[kChunk]) {   // the chunk's mono input, (a0 + a1) / 2
                    const uint32_t gc = gc0 + c;
                    wait_for([&] {
                        return flag_get(flags + F_D0) > gc && flag_get(flags + F_D1) > gc &&
                               flag_get(flags + F_FIN) + kDepth2 > gc;       // and queue 2's buffer is free
                    });
                    const float *q = q1 + (gc % kDepth1) * kPrQBuf + lane;
#pragma unroll
                    for (int k = 0; k < kChunk; ++k) xm[k] = (q[k * 64] + q[kPrQCh + k * 64]) / 2;
                },
                [&](uint32_t f, const float (&o_l)[4], const float (&o_r)[4]) {
                    const uint32_t c = f / kChunk, k0 = f % kChunk, gc = gc0 + c;
                    float *q = q2 + (gc % kDepth2) * kPrQBuf + k0 * 64u + lane;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        q[k * 64] = o_l[k];
                        q[kPrQCh + k * 64] = o_r[k];
                    }
                    if (k0 + 4u == kChunk || f + 4u >= nf) flag_put(flags + F_DT, gc + 1);   // the chunk's last step
                });
        }
    } else {
        // ---------------- F: balance mix, filter1, master; lane = instance ----------------
        for (uint32_t g = blockIdx.x, gi = 0; g < ngroups; g += gridDim.x, ++gi) {
            const uint32_t gc0 = gi * nchunks;
            const uint32_t i_raw = g * 64u + lane;
            const bool valid = i_raw < n;
            const uint32_t i = valid ? i_raw : n - 1;
            const float rbal = __uint_as_float(a.coef[FRC_RBAL * n + i]);
            const float ffreq = __uint_as_float(a.coef[FRC_FFREQ * n + i]);
            const float fdamp = __uint_as_float(a.coef[FRC_FDAMP * n + i]);
            const float fdrive = __uint_as_float(a.coef[FRC_FDRIVE * n + i]);
            const uint32_t ftype = a.coef[FRC_FTYPE * n + i];
            const float master = __uint_as_float(a.coef[FRC_MASTER * n + i]);
            const bool fw = a.coef[FRC_TOPO * n + i] == 1u;
            float flow = __uint_as_float(a.state[FRS_FLOW * n + i]);
            float fband = __uint_as_float(a.state[FRS_FBAND * n + i]);
            float *const o0 = a.out + i, *const o1 = a.out + a.plane + i;
            for (uint32_t c = 0; c < nchunks; ++c) {
                const uint32_t gc = gc0 + c, f0 = c * kChunk;
                const uint32_t C = min((uint32_t)kChunk, nf - f0);
                wait_for([&] { return flag_get(flags + F_DT) > gc; });
                const float *qa = q1 + (gc % kDepth1) * kPrQBuf + lane;
                const float *qv = q2 + (gc % kDepth2) * kPrQBuf + lane;
                float a0[kChunk], a1[kChunk], vl[kChunk], vr[kChunk];
#pragma unroll
                for (int k = 0; k < kChunk; ++k) {
                    a0[k] = qa[k * 64];
                    a1[k] = qa[kPrQCh + k * 64];
                    vl[k] = qv[k * 64];
                    vr[k] = qv[kPrQCh + k * 64];
                }
                flag_put(flags + F_FIN, gc + 1);              // (the release waits for these reads)
#pragma unroll
                for (int k = 0; k < kChunk; ++k) {
                    if ((uint32_t)k < C) {                    // C is wave-uniform
                        // ReverbFx::Process: out = verb balance + in (1 - balance)
                        const float b0 = (vl[k] * rbal) + (a0[k] * (1 - rbal));
                        const float b1 = (vr[k] * rbal) + (a1[k] * (1 - rbal));
                        // FilterFx: the Svf on channel 0; channel 1 is buf_c's 0, or in place b1
                        const float c0 = fr::svf_tick(b0, ffreq, fdamp, fdrive, ftype, flow, fband);
                        if (valid) {
                            o0[(size_t)(f0 + k) * n] = c0 * master;
                            o1[(size_t)(f0 + k) * n] = (fw ? b1 : 0.0f) * master;
                        }
                    }
                }
            }
            if (valid) {
                a.state[FRS_FLOW * n + i] = __float_as_uint(flow);
                a.state[FRS_FBAND * n + i] = __float_as_uint(fband);
            }
        }
    }
}

hipError_t launch_platerack(const PlateRackArgs &a, hipStream_t s) {
    if (a.n == 0 || a.n_frames == 0) return hipSuccess;
    if ((a.n_frames & 3u) || (a.t0 & 1u) || a.t0 >= kFrMaxDelay || (a.d.t0 & 3u) || a.d.n < ((a.n + 63u) & ~63u))
        return hipErrorInvalidValue;
    if ((a.plane + (uint64_t)a.n_frames * a.n) * 4 >= (1ull << 32)) return hipErrorInvalidValue;
    // one workgroup per CU (LDS and registers allow no more), each running its groups back to back
    if (a.cus == 0) return hipErrorInvalidValue;
    const uint32_t groups = (a.n + 63u) / 64u;
    const uint32_t blocks = groups < a.cus ? groups : a.cus;
    hipLaunchKernelGGL(platerack_block_v1, dim3(blocks), dim3(kPrThreads), (size_t)kPrLds * sizeof(float), s, a);
    return hipGetLastError();
}

}  // namespace olfx
