// ol_dsp_amd/csrc/meter.hip -- level meters: per-signal running RMS and peak hold (OLFX_KIND_METER,
// OLFX_KIND_METER_MONO).
//
// Reference: ol::core::Rms (modules/corelib/ol_corelib.h:61-85), a windowed running RMS with a hard reset,
// and the peak-hold follower its one caller pairs it with (modules/ol_daisy/workouts/sandbox/main.cpp:
// 98-137).  Per signal and frame, in fp32 with no contraction (include/olfx.h has the steps):
//   reset test, sum = sum + x * x, count = count + 1, rms = sqrtf(sum / count), peak compare, hold count.
// Rms is header-only and free of DaisySP, so the kernel is held to the real class bit for bit.
//
// A pure stream with a short serial chain per lane: 4 B in (and, in envelope mode, 4 B out) per
// signal-frame, the state in registers for the whole launch.  One lane = one signal (or four adjacent
// instances' signals on the quad path), the channel planes along grid.y.  Frames go in chunks of 16; the
// next chunk's 16 loads are issued ahead of this chunk's arithmetic, branch-free (a load under a branch
// drains every outstanding load): past the last frame the row index is clamped, so the last chunk's
// look-ahead re-reads the call's last row and nothing else.  No LDS, no cross-lane traffic, no atomics.
// (Chunks of 32 in summary mode measured slower at 65,536 stereo instances: DESIGN.md section 4 "Meter".)
// The quad path measured slower than the scalar one on MI355X (DESIGN.md section 4 "Meter"): it is built,
// bit-identical, and runs only under OLFX_MT_QUAD=1.
#include "olfx_internal.h"

#include <cstdlib>

namespace olfx {

namespace {

constexpr uint32_t kMtChunk = 16;
constexpr uint32_t kMtBlock = 64;       // one wave per block: few waves at the sizes of interest, spread over every CU

struct MtState {
    float sum, count, rms, peak, peak_count;
};

// One frame of one signal.  ENV: the value Rms::Process returns; otherwise the divide and the root are left
// to the end of the launch (only the last frame's rms is observable).
template <bool ENV>
__device__ __forceinline__ float mt_step(MtState &s, float x, float window, float hold) {
    if (s.count == window) {
        s.sum = 0.f;
        s.count = 0.f;
    }
    s.sum = s.sum + x * x;
    s.count = s.count + 1.0f;
    float r = 0.f;
    if (ENV) s.rms = r = sqrtf(s.sum / s.count);
    const float ax = fabsf(x);
    s.peak = (s.peak < ax) ? ax : s.peak;
    s.peak_count = s.peak_count + 1.0f;
    if (s.peak_count == hold) {
        s.peak_count = 0.f;
        s.peak = 0.f;
    }
    return r;
}

// V = float (one signal per lane) or float4 (four adjacent instances per lane; n % 4 == 0, 16-B aligned planes)
template <class V>
struct MtLanes;
template <>
struct MtLanes<float> {
    static constexpr uint32_t W = 1;
    __device__ static float get(const float &v, uint32_t) { return v; }
    __device__ static void put(float &v, uint32_t, float x) { v = x; }
};
template <>
struct MtLanes<float4> {
    static constexpr uint32_t W = 4;
    __device__ static float get(const float4 &v, uint32_t k) { return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w; }
    __device__ static void put(float4 &v, uint32_t k, float x) {
        if (k == 0) v.x = x;
        else if (k == 1) v.y = x;
        else if (k == 2) v.z = x;
        else v.w = x;
    }
};

}  // namespace

template <bool ENV, class V>
__global__ __launch_bounds__(kMtBlock) void meter_block_v1(MeterArgs a) {
    using L = MtLanes<V>;
    constexpr uint32_t W = L::W;
    const uint32_t i = (blockIdx.x * kMtBlock + threadIdx.x) * W;     // the lane's first instance
    if (i >= a.n) return;                                             // lanes past n: nothing loaded, nothing done
    const uint32_t p = blockIdx.y, nf = a.n_frames;
    const size_t n = a.n, signals = (size_t)a.planes * n, sig = (size_t)p * n + i;

    // state and coefficients: loaded once, stored once
    MtState st[W];
    float window[W], hold[W];
    {
        const V sum = *(const V *)(a.state + MTS_SUM * signals + sig);
        const V count = *(const V *)(a.state + MTS_COUNT * signals + sig);
        const V rms = *(const V *)(a.state + MTS_RMS * signals + sig);
        const V peak = *(const V *)(a.state + MTS_PEAK * signals + sig);
        const V peak_count = *(const V *)(a.state + MTS_PEAK_COUNT * signals + sig);
        const V w = *(const V *)(a.coef + MTC_WINDOW * n + i);
        const V h = *(const V *)(a.coef + MTC_HOLD * n + i);
#pragma unroll
        for (uint32_t k = 0; k < W; ++k) {
            st[k] = MtState{L::get(sum, k), L::get(count, k), L::get(rms, k), L::get(peak, k), L::get(peak_count, k)};
            window[k] = L::get(w, k);
            hold[k] = L::get(h, k);
        }
    }

    const float *src = a.in + (size_t)p * a.plane + i;
    float *dst = ENV ? a.out + (size_t)p * a.plane + i : nullptr;
    const uint32_t last = nf - 1;

    V next[kMtChunk];
#pragma unroll
    for (uint32_t j = 0; j < kMtChunk; ++j) {
        const uint32_t f = j < last ? j : last;                       // uniform
        next[j] = *(const V *)(src + (size_t)f * n);
    }
    for (uint32_t f0 = 0; f0 < nf; f0 += kMtChunk) {
        V x[kMtChunk];
#pragma unroll
        for (uint32_t j = 0; j < kMtChunk; ++j) x[j] = next[j];
        // the next chunk's loads, ahead of this chunk's arithmetic
#pragma unroll
        for (uint32_t j = 0; j < kMtChunk; ++j) {
            const uint32_t g = f0 + kMtChunk + j;
            const uint32_t f = g < last ? g : last;
            next[j] = *(const V *)(src + (size_t)f * n);
        }
        // n_frames is a multiple of 4: a short last chunk ends after a whole group of four
#pragma unroll
        for (uint32_t q = 0; q < kMtChunk; q += 4) {
            if (f0 + q < nf) {                                        // uniform
#pragma unroll
                for (uint32_t j = q; j < q + 4; ++j) {
                    V r;
#pragma unroll
                    for (uint32_t k = 0; k < W; ++k) L::put(r, k, mt_step<ENV>(st[k], L::get(x[j], k), window[k], hold[k]));
                    if (ENV) *(V *)(dst + (size_t)(f0 + j) * n) = r;
                }
            }
        }
    }

    V sum, count, rms, peak, peak_count;
#pragma unroll
    for (uint32_t k = 0; k < W; ++k) {
        // summary mode: the last frame's rms, from the sum and count that frame left
        const float r = ENV ? st[k].rms : sqrtf(st[k].sum / st[k].count);
        L::put(sum, k, st[k].sum);
        L::put(count, k, st[k].count);
        L::put(rms, k, r);
        L::put(peak, k, st[k].peak);
        L::put(peak_count, k, st[k].peak_count);
    }
    *(V *)(a.state + MTS_SUM * signals + sig) = sum;
    *(V *)(a.state + MTS_COUNT * signals + sig) = count;
    *(V *)(a.state + MTS_RMS * signals + sig) = rms;
    *(V *)(a.state + MTS_PEAK * signals + sig) = peak;
    *(V *)(a.state + MTS_PEAK_COUNT * signals + sig) = peak_count;
}

// OLFX_MT_QUAD=1 takes the quad path wherever the shapes allow (read once per process; tools/meter_ab.py)
static bool meter_quad_enabled() {
    static const bool on = [] {
        const char *v = std::getenv("OLFX_MT_QUAD");
        return v && v[0] == '1';
    }();
    return on;
}

hipError_t launch_meter(const MeterArgs &a, hipStream_t s) {
    if (a.n == 0 || a.n_frames == 0 || a.planes == 0) return hipSuccess;
    // four instances per lane: whole quads in every row, every row and plane on a 16-B boundary
    const bool quad = meter_quad_enabled() && (a.n & 3u) == 0 && (a.plane & 3u) == 0 && ((uintptr_t)a.in & 15u) == 0 &&
                      ((uintptr_t)a.out & 15u) == 0 && ((uintptr_t)a.state & 15u) == 0 && ((uintptr_t)a.coef & 15u) == 0;
    const uint32_t lanes = quad ? a.n / 4u : a.n;
    const dim3 grid((lanes + kMtBlock - 1) / kMtBlock, a.planes), block(kMtBlock);
    if (quad) {
        if (a.out) hipLaunchKernelGGL((meter_block_v1<true, float4>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((meter_block_v1<false, float4>), grid, block, 0, s, a);
    } else {
        if (a.out) hipLaunchKernelGGL((meter_block_v1<true, float>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((meter_block_v1<false, float>), grid, block, 0, s, a);
    }
    return hipGetLastError();
}

}  // namespace olfx
