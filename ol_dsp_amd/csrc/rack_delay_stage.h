// ol_dsp_amd/csrc/rack_delay_stage.h -- the fx rack's delay stage, DelayFx<2>::Process
// (modules/fxlib/Fx.h:193-206), shared by the rack kernel (fxrack.hip) and the plate rack
// (platerack.hip):
//
//   per channel: r = DelayLine.Read(); DelayLine.Write(in + feedback r);
//   filter_ (Svf LowPass) on channel 0 in place; a = r balance + in (1 - balance)
//
// Mapping, window and LINE CARRY are derived in fxrack.hip's head comment: lane = (instance j of the
// wave, channel), a wave = 32 instances x 2 channels, the block in 16-frame chunks; a chunk's reads
// fall in a window of 18 ring positions that lies in two 128-B stereo lines, of which each chunk
// loads only its successor's new one; the chunk's writes leave as one 128-B run per instance from LDS
// staging at the start of the next chunk; the last two chunks' writes are patched into the window
// from registers, so every delay 0..47999 takes one branch-free path.
//
// Three layers:
//   * fr:: helpers: the Svf tick, static_for, the ring wrap;
//   * FR_DELAY_LINES (with FR_PATCH_WINDOW, FR_CARRY_LINES, FR_FLUSH_RING): the window's machinery
//     (line loads and carry, staging, patches, the ring run) as locals and lambdas declared in the
//     caller's scope -- as DT_STAGE in dattorro_stage.h: one
//     aggregate holding the carried lines would stay in scratch memory, separate locals are promoted
//     to registers.  fxrack_block_v3 builds its tick loop on it (both filters share the lane pair
//     there, filter1 one tick behind: 17 ticks per chunk);
//   * fr::delay_stage: the whole stage up to DelayFx's output `a`, handed to a sink (an LDS queue):
//     the plate rack's D role.  The channel-1 lane runs no filter here and a chunk is 16 ticks.
#pragma once
#include <type_traits>
#include <utility>

#include "chorus_stage.h"

namespace olfx {
namespace fr {

constexpr int kChunk = 16;
constexpr int kWin = 20;                            // window slots (18 read) staged from two lines
constexpr int kSlots = kWin + 1;                    // + junk slot
constexpr int kStride = 36;                         // staging floats per instance (32 + pad)
constexpr int kRegion = kSlots * 64 + 32 * kStride; // floats of LDS per wave: the window, the ring-run staging

__device__ __forceinline__ void wave_lds_order() {   // one wave's LDS writes before its other lanes' reads
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Svf::Process (DaisySP, double-sampled Chamberlin) returning the selected output (0 low, 1 band,
// 2 high, 3 notch, 4 peak), as oracle/fxrack_ref.c: the mean of the two passes' values, 0.5 x1 +
// 0.5 x2, formed for the selected output only
__device__ __forceinline__ float svf_pick(uint32_t type, float low, float band, float high, float notch) {
    float peak = low - high;
    asm volatile("" : "+v"(peak));                  // computed for every lane: selects, not branches
    float r = type == 4 ? peak : low;
    r = type == 3 ? notch : r;
    r = type == 2 ? high : r;
    return type == 1 ? band : r;
}
__device__ __forceinline__ float svf_tick(float in, float freq, float damp, float drive, uint32_t type,
                                          float &low, float &band) {
    float notch = in - damp * band;
    low = low + freq * band;
    float high = notch - low;
    band = freq * high + band - drive * band * band * band;
    const float x1 = svf_pick(type, low, band, high, notch);
    notch = in - damp * band;
    low = low + freq * band;
    high = notch - low;
    band = freq * high + band - drive * band * band * band;
    const float x2 = svf_pick(type, low, band, high, notch);
    return 0.5f * x1 + 0.5f * x2;
}

// f(integral_constant<int, 0>) ... f(integral_constant<int, N-1>), unrolled at compile time
template <class F, int... K>
__device__ __forceinline__ void static_for_impl(F &&f, std::integer_sequence<int, K...>) {
    (f(std::integral_constant<int, K>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void static_for(F &&f) {
    static_for_impl(f, std::make_integer_sequence<int, N>{});
}

__device__ __forceinline__ uint32_t wrap48k(int64_t p) {
    const int64_t m = p % (int64_t)kFrMaxDelay;
    return (uint32_t)(m < 0 ? m + kFrMaxDelay : m);
}

}  // namespace fr
}  // namespace olfx

// The window's machinery for the wave's 32 instances from INST0 (of N; LANE = this lane), declared in
// the caller's scope.  RR: the buffer descriptor of the wave's 32 rings; D: this lane's line delay;
// T00: the ring position of frame 0 (even); WIN: the window [fr::kSlots][64].
//   rel_of(t)             the window's first position as an offset from the chunk's first position t
//   lo, nx, lcur          the two lines in registers, the current line number
//   load_line, next_line  a line's cooperative load; the line after (the ring wraps at a line edge)
//   stage_lines()         the chunk's two lines -> the window
// FR_PATCH_WINDOW, FR_CARRY_LINES and FR_FLUSH_RING below are the chunk's other steps over these
// names, as statements (text, not lambdas: fxrack_block_v3's instruction stream is unchanged by them).
#define FR_DELAY_LINES(RR, N, INST0, LANE, D, T00, WIN)                                                            \
    constexpr uint32_t kRing = olfx::kFrMaxDelay * 8u;  /* bytes per instance ring */                            \
    /* window of the chunk starting at t: first position (t - D - 1) rounded down to even, as an offset from    \
       t -- the same for every chunk (t is even) */                                                              \
    auto rel_of = [&](uint32_t t) { return (int)(((int64_t)t - (int64_t)(D) - 1) & ~(int64_t)1) - (int)t; };     \
    /* Cooperative line loads: piece P = r * 64 + lane of 256 -> piece m = 2 r + lane / 32 (16 B: positions     \
       2m, 2m + 1 of the line) of instance jj = lane % 32 (instances innermost: a ds_write_b64 lane group of    \
       16 contiguous lanes stages one piece of 16 instances, 16 distinct bank pairs, conflict-free).  Every     \
       part of a lane serves the same instance jj, whose window start (ring position, wrapped) comes from       \
       lane 2 jj once per launch. */                                                                             \
    const uint32_t jj = (LANE) & 31u;                                                                            \
    const uint32_t oj = min((INST0) + jj, (N) - 1) - (INST0);   /* ring within the wave's descriptor */          \
    const uint32_t spos = (uint32_t)__builtin_amdgcn_ds_bpermute(                                                \
        (int)(jj << 3), (int)olfx::fr::wrap48k(((int64_t)(T00) - (int64_t)(D) - 1) & ~(int64_t)1));              \
    const uint32_t so15 = spos & 15u;                   /* window start within its line (even) */                \
    uint32_t lcur = spos >> 4;                          /* line L of the current chunk (instance jj) */          \
    constexpr uint32_t kLines = olfx::kFrMaxDelay / 16u;   /* 3000 lines per ring: wraps at a line edge */       \
    float4 lo[4], nx[4];                                /* lines L (carried) and L + 1 (loaded a chunk back) */  \
    auto load_line = [&](float4 (&dst)[4], uint32_t line) {                                                      \
        _Pragma("unroll") for (int r = 0; r < 4; ++r)                                                            \
            dst[r] = olfx::ch::ld4(RR, oj * kRing + line * 128u + ((uint32_t)r * 2u + ((LANE) >> 5)) * 16u);     \
    };                                                                                                           \
    auto next_line = [&](uint32_t l) { return l + 1u == kLines ? 0u : l + 1u; };                                 \
    auto stage_lines = [&]() {                                                                                   \
        _Pragma("unroll") for (int r = 0; r < 4; ++r) {                                                          \
            const int m = r * 2 + (int)((LANE) >> 5);                                                            \
            const int slo = 2 * m - (int)so15, shi = slo + 16;   /* slots of the piece in L, L + 1 */            \
            if (slo >= 0) {                                                                                      \
                float *p = (WIN) + (uint32_t)slo * 64u + 2u * jj;                                                \
                *(float2 *)p = make_float2(lo[r].x, lo[r].y);                                                    \
                *(float2 *)(p + 64) = make_float2(lo[r].z, lo[r].w);                                             \
            }                                                                                                    \
            if (shi < olfx::fr::kWin) {                 /* shi + 1 <= kWin: the junk slot at most */             \
                float *p = (WIN) + (uint32_t)shi * 64u + 2u * jj;                                                \
                *(float2 *)p = make_float2(nx[r].x, nx[r].y);                                                    \
                *(float2 *)(p + 64) = make_float2(nx[r].z, nx[r].w);                                             \
            }                                                                                                    \
        }                                                                                                        \
    };

// The last two chunks' writes (Y: chunk c-1's, Y2: chunk c-2's, in registers) into the window of the
// chunk at frame F0: line L was loaded before chunk c-2's stores, L + 1 before chunk c-1's.  Only
// delays below 2 chunks + a window reach those positions: skipped wave-uniformly otherwise
// (REL = -D - 1 or -D - 2).
#define FR_PATCH_WINDOW(F0, REL, WCOL, Y, Y2)                                                                    \
    if ((F0) >= 2u * olfx::fr::kChunk && __builtin_amdgcn_ballot_w64(-2 * olfx::fr::kChunk - (REL) < olfx::fr::kWin)) { \
        _Pragma("unroll") for (int k = 0; k < olfx::fr::kChunk; ++k) {                                           \
            const int s = k - 2 * olfx::fr::kChunk - (REL);   /* slot of position t - 32 + k */                  \
            if (s >= 0 && s < olfx::fr::kWin) (WCOL)[s * 64] = (Y2)[k];                                          \
        }                                                                                                        \
    }                                                                                                            \
    if ((F0) > 0 && __builtin_amdgcn_ballot_w64(-olfx::fr::kChunk - (REL) < olfx::fr::kWin)) {                   \
        _Pragma("unroll") for (int k = 0; k < olfx::fr::kChunk; ++k) {                                           \
            const int s = k - olfx::fr::kChunk - (REL);       /* slot of position t - 16 + k */                  \
            if (s >= 0 && s < olfx::fr::kWin) (WCOL)[s * 64] = (Y)[k];                                           \
        }                                                                                                        \
    }
// L + 1 becomes L; the next chunk's new line in flight (unconditional)
#define FR_CARRY_LINES()                                                                                         \
    _Pragma("unroll") for (int r = 0; r < 4; ++r) lo[r] = nx[r];                                                 \
    lcur = next_line(lcur);                                                                                      \
    load_line(nx, next_line(lcur))
// The ring run of the chunk at frame FP (CP frames) from the staging: one 128-B stereo run per
// instance (8 lanes x 16 B); STAGE: the ring-run staging [32][fr::kStride], WCOL above: this lane's
// column of the window
#define FR_FLUSH_RING(RR, N, INST0, LANE, T00, STAGE, FP, CP)                                                    \
    {                                                                                                            \
        const uint32_t tp = (T00) + (FP);                                                                        \
        _Pragma("unroll") for (int r = 0; r < 4; ++r) {                                                          \
            const uint32_t q = (uint32_t)r * 64u + (LANE), oo = q >> 3, f2 = 2u * (q & 7u);                      \
            const float4 vv = *(const float4 *)((STAGE) + oo * olfx::fr::kStride + 2u * f2);                     \
            const uint32_t oi = (INST0) + oo;                                                                    \
            const bool ok = oi < (N) && (int)f2 < (CP);   /* else an offset past the buffer: dropped */          \
            olfx::ch::st4(RR, ok ? oo * kRing + olfx::fr::wrap48k((int64_t)tp + f2) * 8u : 0xFFFFFFF0u, vv);     \
        }                                                                                                        \
    }

namespace olfx {
namespace fr {

// The delay stage over the block's nf frames for the 32 instances from inst0 (< n; instances past n
// mirror instance n - 1 and store nothing).  ring / state / coef: FxRackArgs'; t00: the ring position
// of frame 0 (even); region: kRegion floats of LDS of this wave.  load(f0, Cx, xv) fills xv[k] with
// this lane's (instance, channel) input of frame f0 + k for k < Cx and 0.f from Cx on (Cx = 0: a chunk
// past the block's end); it is called for chunk c + 1 before chunk c is computed, chunk 0 first.
// emit(c, av) takes chunk c's DelayFx outputs of this lane's (instance, channel), av[k] for frame
// 16 c + k (frames past a short last chunk are unspecified); in topology 1 (DelayFx<1>, then
// stereo[0] = stereo[1]) both lanes of the instance give channel 0's.
template <class Load, class Emit>
__device__ __forceinline__ void delay_stage_from(float *ring, uint32_t *state, const uint32_t *coef, uint32_t n,
                                                 uint32_t nf, uint32_t t00, float *region, uint32_t lane,
                                                 uint32_t inst0, Load &&load, Emit &&emit) {
    const uint32_t j = lane >> 1, chn = lane & 1u;
    const uint32_t i_raw = inst0 + j;
    const bool valid = i_raw < n;
    const uint32_t i = valid ? i_raw : n - 1;

    const uint32_t D = coef[FRC_DELAY * n + i];
    const float frac = __uint_as_float(coef[FRC_FRAC * n + i]);
    const float feedback = __uint_as_float(coef[FRC_FEEDBACK * n + i]);
    const float dbal = __uint_as_float(coef[FRC_DBAL * n + i]);
    const float dfreq = __uint_as_float(coef[FRC_DFREQ * n + i]);
    const float ddamp = __uint_as_float(coef[FRC_DDAMP * n + i]);
    const float ddrive = __uint_as_float(coef[FRC_DDRIVE * n + i]);
    const bool fw = coef[FRC_TOPO * n + i] == 1u;
    // DelayFx's filter_ acts on channel 0 only: the lane of channel 1 computes it too and drops it
    float slow = __uint_as_float(state[FRS_DLOW * n + i]);
    float sband = __uint_as_float(state[FRS_DBAND * n + i]);

    // the wave's 32 rings (12.3 MB) get their own descriptor, so 32-bit offsets cover any n
    const ch::Rsrc rR = ch::rsrc(ring + (size_t)inst0 * kFrMaxDelay * 2, (uint64_t)min(32u, n - inst0) * kFrMaxDelay * 8);

    float *win = region;                                // [kSlots][64]
    float *wcol = win + lane;
    float *stage = win + kSlots * 64;                   // [32][kStride]
    FR_DELAY_LINES(rR, n, inst0, lane, D, t00, win);

    float x[kChunk], xn[kChunk], y[kChunk], y2[kChunk];
    int C = (int)min((uint32_t)kChunk, nf);
    load(0u, C, x);
    load_line(lo, lcur);
    load_line(nx, next_line(lcur));
    for (uint32_t f0 = 0, c = 0; f0 < nf; f0 += kChunk, ++c) {
        C = (int)min((uint32_t)kChunk, nf - f0);
        const int Cn = f0 + kChunk < nf ? (int)min((uint32_t)kChunk, nf - f0 - kChunk) : 0;
        const uint32_t t = t00 + f0;                    // chunk's first position, unreduced
        const int rel = rel_of(t);
        // ---- 1. this chunk's window -> LDS from its two lines, patched with the last two chunks'
        //         writes: line L was loaded before chunk c-2's stores, L + 1 before chunk c-1's ----
        stage_lines();
        FR_PATCH_WINDOW(f0, rel, wcol, y, y2)
        // a chunk's ring run is stored at the start of the NEXT chunk, ahead of that chunk's loads
        if (f0 > 0) FR_FLUSH_RING(rR, n, inst0, lane, t00, stage, f0 - kChunk, kChunk)   // the previous chunk was full
        // ---- 2. the next chunk's inputs and new line in flight (unconditional); L + 1 is carried ----
        load(f0 + kChunk, Cn, xn);
        FR_CARRY_LINES();
#pragma unroll
        for (int k = 0; k < kChunk; ++k) y2[k] = y[k];
        // ---- 3. the frames: the delay line (both lanes, own channel), filter_, the balance ----
        float av[kChunk];
#pragma unroll
        for (int k = 0; k < kChunk; ++k) av[k] = __builtin_nondeterministic_value(0.f);
        auto tick = [&](auto generic_tag, auto k_tag) {
            constexpr bool GENERIC = decltype(generic_tag)::value;
            constexpr int k = decltype(k_tag)::value;
            if (GENERIC && k >= C) return;
            // DelayLine::Read: a at delay D, b at D + 1 (slots k - D - rel, one below)
            const int sa = k - (int)D - rel;
            const float pa = wcol[sa * 64], pb = wcol[(sa - 1) * 64];
            const float r = pa + (pb - pa) * frac;
            const float w = x[k] + (feedback * r);      // DelayLine::Write
            y[k] = w;
            wcol[min(k - rel, kWin) * 64] = w;          // visible to later frames of this chunk
            float lw = slow, bd = sband;
            const float so = svf_tick(r, dfreq, ddamp, ddrive, 0u, lw, bd);
            slow = lw;
            sband = bd;
            // DelayFx: out = buf balance + in (1 - balance); buf is filtered on channel 0 only
            const float own = ((chn ? r : so) * dbal) + (x[k] * (1 - dbal));
            const float a0 = ch::pair_even(own);
            av[k] = fw ? a0 : own;
        };
        if (C == kChunk) static_for<kChunk>([&](auto kt) { tick(std::false_type{}, kt); });
        else static_for<kChunk>([&](auto kt) { tick(std::true_type{}, kt); });
        emit(c, av);
        // ---- 4. the chunk's writes -> LDS staging ([instance][frame][ch]); they leave as 128-B
        //         runs (8 lanes each) with the next chunk's flush ----
        {
            float *st = stage + j * kStride + chn;
#pragma unroll
            for (int k = 0; k < kChunk; ++k) st[2 * k] = y[k];
        }
#pragma unroll
        for (int k = 0; k < kChunk; ++k) x[k] = xn[k];
    }
    {
        const uint32_t fl = (nf - 1u) / kChunk * kChunk;   // the last chunk
        FR_FLUSH_RING(rR, n, inst0, lane, t00, stage, fl, (int)(nf - fl))
    }
    if (valid && chn == 0u) {
        state[FRS_DLOW * n + i] = __float_as_uint(slow);
        state[FRS_DBAND * n + i] = __float_as_uint(sband);
    }
}

// The stage with its input in HBM (the plate rack's D role): in is [2][..][n] with the channel planes
// `plane` floats apart; every chunk's loads are issued unconditionally (clamped to the block's last
// frame) a chunk ahead.
template <class Emit>
__device__ __forceinline__ void delay_stage(float *ring, uint32_t *state, const uint32_t *coef, const float *in,
                                            uint64_t plane, uint32_t n, uint32_t nf, uint32_t t00, float *region,
                                            uint32_t lane, uint32_t inst0, Emit &&emit) {
    const uint32_t i = min(inst0 + (lane >> 1), n - 1);
    const ch::Rsrc rIn = ch::rsrc(in, (plane + (uint64_t)nf * n) * 4);
    const uint32_t io_v = (lane & 1u) * (uint32_t)plane * 4u + i * 4u, frame_b = n * 4u;
    delay_stage_from(
        ring, state, coef, n, nf, t00, region, lane, inst0,
        [&](uint32_t f0, int Cx, float (&xv)[kChunk]) {
#pragma unroll
            for (int k = 0; k < kChunk; ++k) {
                const float vv = ch::ld1(rIn, io_v, min(f0 + (uint32_t)k, nf - 1u) * frame_b);
                xv[k] = k < Cx ? vv : 0.f;
            }
        },
        emit);
}

}  // namespace fr
}  // namespace olfx
