// ol_dsp_amd/csrc/chorus.hip -- RNBO stereo chorus and gen~ pitch-shifter kernel on gfx950.
// The stage (spec, memory shape, line carry, software pipeline) is in chorus_stage_l.h, its
// helpers in chorus_stage.h; the chorus kind's ring-free stage in chorus_stage_rf.h.
#include "chorus_stage_l.h"
#include "chorus_stage_rf.h"

namespace olfx {

// Round 4's block-at-once kernels (chorus_block_v13: frame-parallel pitch-shifter and chorus tap
// over a whole 256-frame block per 16 instances, lores~ serial; v14: lores~ on its own wave,
// overlapped with the next group) were bit-exact and slower (chorus 0.324-0.328 ms against v11's
// 0.234-0.241, pitch-shift 0.151-0.168 against 0.148-0.152) and are not kept.

// chorus_block_v11: one wave = 32 instances x 2 channels over the line-carry stage
// (chorus_stage_l.h); chunks alternate the line set (PAR), so the chunk loop is unrolled by two.
// COOP: cooperative input/output rows (4 + 4 dwordx4 per lane and chunk, transposed through LDS:
// ChStageL COOP), for n and the plane distance multiples of 4 (16-B aligned rows, no row split by
// the last instance); otherwise one float per lane, frame and direction.
template <bool FULL, bool COOP>
__global__ __launch_bounds__(ch::kThreads, 2) void chorus_block_v11(ChorusArgs a) {
    using Stage = ch::ChStageL<FULL, COOP>;
    constexpr int kChunk = Stage::kChunk;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const uint32_t tid = threadIdx.x;
    const uint32_t wib = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const uint32_t wave = blockIdx.x * (ch::kThreads / 64) + wib, lane = tid & 63u;
    const uint32_t inst0 = wave * 32u;
    if (inst0 >= a.n) return;
    Stage st;
    st.init(a, lds + wib * Stage::kRegion, lane, inst0);

    const uint32_t nf = a.n_frames, n = a.n;
    const ch::Rsrc rIn = ch::rsrc(a.in, (a.plane + (uint64_t)nf * n) * 4);
    const ch::Rsrc rOut = ch::rsrc(a.out, (a.plane + (uint64_t)nf * n) * 4);
    const uint32_t io_v = st.ch * (uint32_t)a.plane * 4u + st.i * 4u, frame_b = n * 4u;
    const uint32_t out_v = st.valid ? io_v : 0xFFFFFFF0u;
    // COOP rows: lane's piece of row r = (frame r / 2, channel r % 2): instances inst0 + 4 (lane % 8) ..
    const uint32_t pinst = inst0 + (lane & 7u) * 4u;
    auto row_v = [&](int q, uint32_t f0) {              // byte offset of the lane's piece, frame clamped
        const uint32_t r = Stage::coop_row(q, lane);
        return (r & 1u) * (uint32_t)a.plane * 4u + min(f0 + (r >> 1), nf - 1u) * frame_b + pinst * 4u;
    };

    float x[kChunk], xn[kChunk];
    float4 xq[4];
    int C = (int)min((uint32_t)kChunk, nf);
    if constexpr (COOP) {
#pragma unroll
        for (int q = 0; q < 4; ++q) xq[q] = ch::ld4(rIn, row_v(q, 0));
        st.begin(x, C, xq);
    } else {
#pragma unroll
        for (int k = 0; k < kChunk; ++k) x[k] = k < C ? ch::ld1<ch::kStreamAux>(rIn, io_v, (uint32_t)k * frame_b) : 0.f;
        st.begin(x, C);
    }
    auto step = [&](auto par, uint32_t f0) {
        C = (int)min((uint32_t)kChunk, nf - f0);
        const int Cn = f0 + kChunk < nf ? (int)min((uint32_t)kChunk, nf - f0 - kChunk) : 0;
        // the next chunk's input (unconditional loads, the frame clamped into the block; lanes
        // past Cn get 0), issued by the stage once this chunk's stores and staging are out
        auto prefetch = [&]() {
            if constexpr (COOP) {
#pragma unroll
                for (int q = 0; q < 4; ++q) xq[q] = ch::ld4(rIn, row_v(q, f0 + kChunk));
            } else {
#pragma unroll
                for (int k = 0; k < kChunk; ++k) {
                    const float v = ch::ld1<ch::kStreamAux>(rIn, io_v, min(f0 + kChunk + (uint32_t)k, nf - 1u) * frame_b);
                    xn[k] = k < Cn ? v : 0.f;
                }
            }
        };
        if constexpr (COOP) {
            st.template chunk<decltype(par)::value>(
                x, xn, C, Cn, [&](int k, float v) { st.out_stage(k, v); }, prefetch, xq);
            // the chunk's outputs: rows of 32 instances, 16 B per lane (frames past C dropped)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t r = Stage::coop_row(q, lane), f = r >> 1;
                const bool ok = pinst < n && (int)f < C;
                ch::st4(rOut, ok ? (r & 1u) * (uint32_t)a.plane * 4u + (f0 + f) * frame_b + pinst * 4u : 0xFFFFFFF0u,
                        st.coop_out(q));
            }
        } else {
            st.template chunk<decltype(par)::value>(
                x, xn, C, Cn,
                [&](int k, float v) { ch::st1<ch::kStreamAux>(rOut, out_v, (f0 + (uint32_t)k) * frame_b, v); },
                prefetch, xq);
        }
#pragma unroll
        for (int k = 0; k < kChunk; ++k) x[k] = xn[k];
    };
    for (uint32_t f0 = 0; f0 < nf; f0 += 2 * kChunk) {
        step(std::integral_constant<int, 0>{}, f0);
        if (f0 + kChunk < nf) step(std::integral_constant<int, 1>{}, f0 + kChunk);
    }
    st.finish(a);
}

// chorus_block_rf1: the chorus without its chorus ring (chorus_stage_rf.h) -- v11's wave mapping, I/O
// variants and chunk loop, run per segment of at most 256 frames: each segment takes its lead, computes
// its psv window fresh and restarts the line carry.  A 256-frame block is one segment.
template <bool COOP>
__global__ __launch_bounds__(ch::kThreads, 2) void chorus_block_rf1(ChorusArgs a) {
    using Stage = ch::ChStageRF<COOP>;
    constexpr int kChunk = Stage::kChunk;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const uint32_t tid = threadIdx.x;
    const uint32_t wib = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const uint32_t wave = blockIdx.x * (ch::kThreads / 64) + wib, lane = tid & 63u;
    const uint32_t inst0 = wave * 32u;
    if (inst0 >= a.n) return;
    Stage st;
    st.init(a, lds + wib * Stage::kRegion, lane, inst0);

    const uint32_t nf = a.n_frames, n = a.n;
    const ch::Rsrc rIn = ch::rsrc(a.in, (a.plane + (uint64_t)nf * n) * 4);
    const ch::Rsrc rOut = ch::rsrc(a.out, (a.plane + (uint64_t)nf * n) * 4);
    const uint32_t io_v = st.ch * (uint32_t)a.plane * 4u + st.i * 4u, frame_b = n * 4u;
    const uint32_t out_v = st.valid ? io_v : 0xFFFFFFF0u;
    const uint32_t pinst = inst0 + (lane & 7u) * 4u;
    auto row_v = [&](int q, uint32_t f0) {
        const uint32_t r = Stage::coop_row(q, lane);
        return (r & 1u) * (uint32_t)a.plane * 4u + min(f0 + (r >> 1), nf - 1u) * frame_b + pinst * 4u;
    };

    float x[kChunk], xn[kChunk];
    float4 xq[4] = {};
    for (uint32_t seg0 = 0; seg0 < nf;) {
        // the longest segment whose delay excursion every lane's psv window holds (16 frames always do:
        // the delay moves by at most one in a chunk)
        uint32_t len = min((uint32_t)Stage::kSegment, nf - seg0);
        while (!__all(st.choose_lead((int)len)) && len > (uint32_t)kChunk) len = max((uint32_t)kChunk, (len >> 1) & ~15u);
        const uint32_t seg1 = seg0 + len;
        int C = (int)min((uint32_t)kChunk, len);
        if constexpr (COOP) {
#pragma unroll
            for (int q = 0; q < 4; ++q) xq[q] = ch::ld4(rIn, row_v(q, seg0));
        } else {
#pragma unroll
            for (int k = 0; k < kChunk; ++k)
                x[k] = k < C ? ch::ld1<ch::kStreamAux>(rIn, io_v, min(seg0 + (uint32_t)k, nf - 1u) * frame_b) : 0.f;
        }
        st.begin_segment(x, C, xq);
        auto step = [&](auto par, uint32_t f0) {
            C = (int)min((uint32_t)kChunk, seg1 - f0);
            const int Cn = f0 + kChunk < seg1 ? (int)min((uint32_t)kChunk, seg1 - f0 - kChunk) : 0;
            auto prefetch = [&]() {
                if constexpr (COOP) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) xq[q] = ch::ld4(rIn, row_v(q, f0 + kChunk));
                } else {
#pragma unroll
                    for (int k = 0; k < kChunk; ++k) {
                        const float v = ch::ld1<ch::kStreamAux>(rIn, io_v, min(f0 + kChunk + (uint32_t)k, nf - 1u) * frame_b);
                        xn[k] = k < Cn ? v : 0.f;
                    }
                }
            };
            if constexpr (COOP) {
                st.template chunk<decltype(par)::value>(
                    x, xn, C, Cn, [&](int k, float v) { st.out_stage(k, v); }, prefetch, xq);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const uint32_t r = Stage::coop_row(q, lane), f = r >> 1;
                    const bool ok = pinst < n && (int)f < C;
                    ch::st4(rOut, ok ? (r & 1u) * (uint32_t)a.plane * 4u + (f0 + f) * frame_b + pinst * 4u : 0xFFFFFFF0u,
                            st.coop_out(q));
                }
            } else {
                st.template chunk<decltype(par)::value>(
                    x, xn, C, Cn,
                    [&](int k, float v) { ch::st1<ch::kStreamAux>(rOut, out_v, (f0 + (uint32_t)k) * frame_b, v); },
                    prefetch, xq);
            }
#pragma unroll
            for (int k = 0; k < kChunk; ++k) x[k] = xn[k];
        };
        for (uint32_t f0 = seg0; f0 < seg1; f0 += 2 * kChunk) {
            step(std::integral_constant<int, 0>{}, f0);
            if (f0 + kChunk < seg1) step(std::integral_constant<int, 1>{}, f0 + kChunk);
        }
        st.end_segment();
        seg0 = seg1;
    }
    st.finish(a);
}

// chorus_materialise: psv at the last `history` positions below a.t0 into the chorus ring, from the x
// ring under the coefficients and phasors in force (ch::psv_direct, the ring-free stage's own
// function).  One thread per (instance, channel) and run of 64 positions.
__global__ __launch_bounds__(256) void chorus_materialise(ChorusArgs a, uint32_t history) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x, i = t >> 1, c = t & 1u, n = a.n;
    if (i >= n) return;
    const uint64_t ps_inc = ((uint64_t)a.coef[CHC_PS_INC * n + i] << 32) | a.coef[CHC_PS_INC_LO * n + i];
    const uint64_t ps_acc = ((uint64_t)a.state[CHS_PS_ACC * n + i] << 32) | a.state[CHS_PS_LO * n + i];
    const uint32_t wi = a.coef[CHC_WINDOW * n + i], wf = a.coef[CHC_WINDOW_LO * n + i];
    const ch::Rsrc rP = ch::rsrc(a.pitch_ring, (uint64_t)n * 2 * a.psize * 4);
    const ch::Rsrc rC = ch::rsrc(a.chorus_ring, (uint64_t)n * 2 * a.csize * 4);
    const uint32_t pb = i * a.psize * 8u + c * 4u, cb = i * a.csize * 8u + c * 4u;
    const uint32_t m0 = blockIdx.y * 64u;
    for (uint32_t m = m0; m < min(m0 + 64u, history); ++m) {
        const uint32_t back = history - m;                   // the position is `back` frames before a.t0
        const float v = ch::psv_direct(rP, pb, a.psize - 1u, ps_acc - (uint64_t)back * ps_inc, a.t0 - back, wi, wf, a.pmax);
        ch::st1(rC, cb + ((a.t0 - back) & (a.csize - 1u)) * 8u, 0, v);
    }
}

static bool chorus_args_ok(const ChorusArgs &a) {
    if ((a.n_frames & 3u) || (a.t0 & 3u)) return false;
    // 32-bit buffer offsets: the rings and the two audio planes must stay below 4 GiB
    return !((uint64_t)a.n * 2 * a.csize * 4 >= (1ull << 32) || (uint64_t)a.n * 2 * a.psize * 4 >= (1ull << 32) ||
             (a.plane + (uint64_t)a.n_frames * a.n) * 4 >= (1ull << 32) || a.plane < (uint64_t)a.n_frames * a.n);
}

hipError_t launch_chorus_ringfree(const ChorusArgs &a, hipStream_t s) {
    if (a.n == 0 || a.n_frames == 0) return hipSuccess;
    // the x ring holds the chorus history, the pitch window and the chunks in flight (olfx_host.cpp chorus_x_size)
    if (!chorus_args_ok(a) || a.mode != 0 || a.psize < a.pmax + 64u) return hipErrorInvalidValue;
    const uint32_t waves = (a.n + 31) / 32;
    const uint32_t blocks = (waves + ch::kThreads / 64 - 1) / (ch::kThreads / 64);
    const bool coop = (a.n & 3u) == 0 && (a.plane & 3u) == 0 && (((uintptr_t)a.in | (uintptr_t)a.out) & 15u) == 0;
    const size_t lds_t = (size_t)(ch::kThreads / 64) * ch::ChStageRF<true>::kRegion * sizeof(float);
    const size_t lds_f = (size_t)(ch::kThreads / 64) * ch::ChStageRF<false>::kRegion * sizeof(float);
    if (coop) hipLaunchKernelGGL((chorus_block_rf1<true>), dim3(blocks), dim3(ch::kThreads), lds_t, s, a);
    else hipLaunchKernelGGL((chorus_block_rf1<false>), dim3(blocks), dim3(ch::kThreads), lds_f, s, a);
    return hipGetLastError();
}

hipError_t launch_chorus_materialise(const ChorusArgs &a, uint32_t history, hipStream_t s) {
    if (a.n == 0 || history == 0) return hipSuccess;
    if ((uint64_t)a.n * 2 * a.csize * 4 >= (1ull << 32) || (uint64_t)a.n * 2 * a.psize * 4 >= (1ull << 32) ||
        history > a.csize)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(chorus_materialise, dim3((2 * a.n + 255) / 256, (history + 63) / 64), dim3(256), 0, s, a, history);
    return hipGetLastError();
}

hipError_t launch_chorus(const ChorusArgs &a, hipStream_t s) {
    if (a.n == 0 || a.n_frames == 0) return hipSuccess;
    if ((a.n_frames & 3u) || (a.t0 & 3u)) return hipErrorInvalidValue;
    // 32-bit buffer offsets: the rings and the two audio planes must stay below 4 GiB
    if ((uint64_t)a.n * 2 * a.csize * 4 >= (1ull << 32) || (a.plane + (uint64_t)a.n_frames * a.n) * 4 >= (1ull << 32) ||
        a.plane < (uint64_t)a.n_frames * a.n)
        return hipErrorInvalidValue;
    const uint32_t waves = (a.n + 31) / 32;              // 32 instances x 2 channels per wave
    const uint32_t blocks = (waves + ch::kThreads / 64 - 1) / (ch::kThreads / 64);
    auto lds = [](auto full, auto coop) {
        return (size_t)(ch::kThreads / 64) * ch::ChStageL<decltype(full)::value, decltype(coop)::value>::kRegion *
               sizeof(float);
    };
    using T = std::true_type;
    using F = std::false_type;
    const size_t lds_c = lds(T{}, T{}), lds_cl = lds(T{}, F{}), lds_p = lds(F{}, T{}), lds_pl = lds(F{}, F{});
    // cooperative rows need 16-B aligned rows that never straddle the last instance
    const bool coop = (a.n & 3u) == 0 && (a.plane & 3u) == 0 && (((uintptr_t)a.in | (uintptr_t)a.out) & 15u) == 0;
    if (a.mode == 0) {
        if (coop) hipLaunchKernelGGL((chorus_block_v11<true, true>), dim3(blocks), dim3(ch::kThreads), lds_c, s, a);
        else hipLaunchKernelGGL((chorus_block_v11<true, false>), dim3(blocks), dim3(ch::kThreads), lds_cl, s, a);
    } else {
        if (coop) hipLaunchKernelGGL((chorus_block_v11<false, true>), dim3(blocks), dim3(ch::kThreads), lds_p, s, a);
        else hipLaunchKernelGGL((chorus_block_v11<false, false>), dim3(blocks), dim3(ch::kThreads), lds_pl, s, a);
    }
    return hipGetLastError();
}

}  // namespace olfx
