// ol_dsp_amd/csrc/chorus_stage_rf.h -- the RING-FREE chorus stage (chorus_block_rf1).
//
// Same spec and per-frame arithmetic as chorus_stage_l.h (v11); what changes is where the chorus
// tap gets the pitch-shifter's output psv from.  v11 writes psv to a second ring and sweeps it with
// the chorus tap: 16 of its 56 B/frame.  But psv(tau) is a pure function of
//   - the x history around tau - dA(tau) and tau - dB(tau),
//   - the pitch phasor at tau, which is ps_acc(now) - (now - tau) ps_inc, exact in the 64-bit fixed
//     point of the stage (all arithmetic mod 2^64), and
//   - ps_inc, the window W and the pitch delay clamp,
// and the output at frame t needs psv only at t - dc and t - dc - 1 (dc = the chorus tap's integer
// delay).  So this stage keeps only the x ring, made deep enough for the chorus delay plus the pitch
// window, and runs the pitch-shifter LATE: at the positions the chorus tap is about to read.  The
// values are bit-identical to the stored ones as long as ps_inc, W and the clamp are the ones that
// were in force at tau: the same x samples, phasor bits and fused-multiply-add sequence.  The host
// guarantees that (olfx_host.h RingFree): after a pitch or window change it runs v11 on both rings
// until the whole chorus history has been written under the new coefficients.
//
// Lead.  A launch is cut into segments of at most 256 frames.  For a segment each instance takes a
// constant lead L = a lower bound of floor(dc) over the segment, from the LFO's bounds (choose_lead);
// chunk c (first frame w0) then produces psv at the 16 positions w0 - L .. w0 - L + 15 -- the
// pitch-shifter of v11 with its time base shifted by L: the phasor is ps_acc - L ps_inc and the
// window starts lie L positions earlier.  Every lane produces exactly 16 new positions per chunk, so
// the small per-lane window of psv in LDS ([kTail old | 16 new] slots, the old ones copied down at
// each chunk) is addressed with wave-uniform slot numbers.  Frame k with delay d reads slots
// kTail + k - (d - L) and the one below: 0 <= d - L <= kTail - 1 is what choose_lead checks (the
// delay moves by < 10 samples in 256 frames at the fastest legal depth x rate; where the bound does
// not hold for some lane, the wave halves the segment).
//
// Segment start.  The kTail old positions of a segment's first chunk come from a LEAD-IN chunk: the
// fast path's phase A run once over the 16 positions w0 - L - 16 .. w0 - L - 1 (phasor 16 ps_inc
// further back, plan and lines relative to write position w0 - 16), of which the last kTail are
// kept.  It has no tap, no output, no ring store and no x patch: it reads x at positions <= w0 - 2,
// all in the ring from earlier chunks or launches, and its lines are loaded fresh.  Its line
// addresses do not depend on the segment's input, so they are issued along with the first input
// loads; chunk 0 then finds its window one line on from the lead-in's, carries that line and loads
// one new line per tap, issued ahead of the lead-in's arithmetic.  Where the two lines cannot cover
// the lead-in's windows for every lane of the wave (a phasor wrap inside the 16 positions), the
// wave computes the kTail positions straight from the ring instead (psv_direct, four at a time) and
// loads chunk 0's windows fresh.
//
// Staleness, restated for the shifted time base.  As in v11 each chunk stores the NEXT chunk's
// input x_{c+1} to the ring before it issues the next chunk's line loads, so a freshly loaded line
// holds everything up to the next chunk's own frames, and a line carried from the chunk before
// lacks only x_c, which is patched into the windows from registers.  With L > 0 the windows lie L
// positions further back, so the patch matters only for L < 15 (depth near 0: the tap reads psv of
// the chunk's own frames, which need x of the chunk); for larger L every patched slot falls past
// the window into the junk slot.  There is no psv ring, so v11's second patch (psv_{c-1}) is gone.
// The generic path and the tail pass read x straight from the ring: x_c is there since the chunk
// before (or since begin()), stored by this wave ahead of the loads.
//
// Partial chunks (C < 16, only at the end of a launch) and chunks whose pitch windows the lines
// cannot cover take the generic path: psv_direct per position, then the tap per frame.
#pragma once
#include "chorus_stage_l.h"

namespace olfx {
namespace ch {

// psv at ring position tau for the pitch phasor `acc` of that position, its x history read straight
// from the ring (own channel of instance offset pb): the arithmetic of the stage's frames.  Shared
// by the ring-free stage (tail pass, generic chunks) and the materialise kernel (chorus.hip).
__device__ __forceinline__ float psv_direct(Rsrc rP, uint32_t pb, uint32_t pmask, uint64_t acc, uint32_t tau,
                                            uint32_t wi, uint32_t wf, uint32_t pmaxu) {
    const uint32_t ph = hi32(acc);
    float gA, gB;
    win_gains(unit24(ph), gA, gB);
    uint32_t di; float fr;
    pitch_split(ph, wi, wf, pmaxu, di, fr);
    uint32_t q = tau - di;
    const float tA = lerp_pair(ld1(rP, pb + (q & pmask) * 8u, 0), ld1(rP, pb + ((q - 1u) & pmask) * 8u, 0), fr);
    pitch_split(ph + 0x80000000u, wi, wf, pmaxu, di, fr);
    q = tau - di;
    const float tB = lerp_pair(ld1(rP, pb + (q & pmask) * 8u, 0), ld1(rP, pb + ((q - 1u) & pmask) * 8u, 0), fr);
    return xfade(tB, gB, tA, gA);
}

template <bool COOP>
struct ChStageRF : ChStageL<false, COOP, false> {
    using B = ChStageL<false, COOP, false>;
    static constexpr int kChunk = B::kChunk, kWin = B::kWin, kSlots = B::kSlots;
    // the psv window: kTail old positions below the chunk's 16 new ones
    static constexpr int kTail = 12, kPsvSlots = kTail + kChunk;
    static constexpr int kSegment = 256;
    static_assert(kTail % 4 == 0, "the tail pass runs in fours");
    // floats of LDS per wave: two pitch windows and the psv window (80 slots x 64 lanes = 20 KB: two
    // waves per SIMD); the COOP output staging overlays the pitch windows, dead by then, as in v11
    static constexpr int kRegion = (2 * kSlots + kPsvSlots) * kRow;
    static constexpr uint32_t kPsvWin = (uint32_t)(2 * kSlots * kRow);
    static constexpr uint32_t kOutCh = B::kOutCh;
    static_assert(B::kOutFloats <= kPsvWin && 32 * B::kStride <= (int)kPsvWin, "staging must stay below the psv window");
    static_assert(kRegion * 4 <= 20 * 1024, "two waves per SIMD");

    using B::lane; using B::j; using B::ch; using B::inst0; using B::n; using B::lfo_inc; using B::lfo_off;
    using B::ps_inc; using B::D; using B::wi; using B::wf; using B::b0; using B::b1; using B::b2; using B::a1;
    using B::a2; using B::mix; using B::dry; using B::lfo_acc; using B::ps_acc; using B::z1; using B::z2;
    using B::pmask; using B::pmaxu; using B::cmaxd; using B::rP; using B::region; using B::pl; using B::wpos;
    using B::started;

    uint32_t lead;            // L of the segment; ps_acc is the SHIFTED phasor (position wpos - L) meanwhile
    Rsrc rNone;               // the x ring with no records: loads against it fetch nothing

    __device__ __forceinline__ void init(const ChorusArgs &a, float *lds_region, uint32_t lane_, uint32_t inst0_) {
        B::init(a, lds_region, lane_, inst0_);
        rNone = rsrc(a.pitch_ring, 0);
    }

    // Bounds of the chorus delay over the next len frames -> the segment's lead; false if the psv
    // window cannot hold the delay's excursion (the caller shortens the segment).  The delay is
    // monotone in cos, whose extremes over the phase interval are its endpoints, +1 where the
    // interval passes phase 0 and -1 where it passes 1/2; endpoints in fp32 as in plan_chunk_l
    // (within 5e-4 sample of the frames' own double delays), widened by 0.01.
    __device__ __forceinline__ bool choose_lead(int len) {
        const uint64_t span = (uint64_t)(len - 1) * lfo_inc;
        const uint64_t p0 = lfo_acc + lfo_off, p1 = p0 + span;
        const bool many = lfo_inc > 0xFFFFFFFFFFFFFFFFull / (uint64_t)len;          // more than a cycle
        const bool has_max = many || p1 < p0;
        const bool has_min = many || (p1 + kHalfCycle) < (p0 + kHalfCycle);
        const float Df = (float)D, cm = (float)cmaxd;
        const float e0 = cos2pi(unit24h(p0)) * Df + Df, e1 = cos2pi(unit24h(p1)) * Df + Df;
        const float hi = fminf(fmaxf(has_max ? 2.0f * Df : fmaxf(e0, e1), 0.0f), cm);
        const float lo = fminf(fmaxf(has_min ? 0.0f : fminf(e0, e1), 0.0f), cm);
        const int dhi = min((int)(hi + 0.01f), (int)cmaxd);
        const int dlo = (int)fmaxf(lo - 0.01f, 0.0f);
        lead = (uint32_t)dlo;
        return dhi - dlo <= kTail - 1;
    }

    // the pitch windows of a chunk of C positions whose first has the (shifted) phasor acc: starts
    // relative to the chunk's first WRITE position, i.e. L further back than the positions' own
    __device__ __forceinline__ PlanL plan_rf(uint64_t acc, int C) const {
        PlanL p;
        const uint32_t last = (uint32_t)(C - 1);
        const int L = (int)lead;
        uint32_t d0, d1;
        float fr;
        {
            const uint64_t a0 = acc, a1_ = acc + last * ps_inc;
            pitch_split(hi32(a0), wi, wf, pmaxu, d0, fr);
            pitch_split(hi32(a1_), wi, wf, pmaxu, d1, fr);
            const int lo = -(int)d1 - 1 - L, hi = (int)last - (int)d0 - L;
            p.sA = lo & ~3;
            p.okA = a1_ >= a0 && hi - p.sA < kWin;
        }
        {
            const uint64_t a0 = acc + kHalfCycle, a1_ = a0 + last * ps_inc;
            pitch_split(hi32(a0), wi, wf, pmaxu, d0, fr);
            pitch_split(hi32(a1_), wi, wf, pmaxu, d1, fr);
            const int lo = -(int)d1 - 1 - L, hi = (int)last - (int)d0 - L;
            p.sB = lo & ~3;
            p.okB = a1_ >= a0 && hi - p.sB < kWin;
        }
        p.sC = 0; p.hiC = 0;
        return p;
    }

    __device__ __forceinline__ void out_stage(int k, float v) { region[ch * kOutCh + (uint32_t)k * 32u + j] = v; }
    __device__ __forceinline__ float4 coop_out(int q) const {
        const uint32_t r = B::coop_row(q, lane);
        return *(const float4 *)(region + (r & 1u) * kOutCh + (r >> 1) * 32u + (lane & 7u) * 4u);
    }

    // v11's phase A on the shifted time base, for the positions K0 .. 15 of the 16 whose windows p
    // plans (acc: the phasor of position K0, advanced past the last on return): position index k
    // reads slot k - L - d - s (s relative to the first write position)
    template <int K0>
    __device__ __forceinline__ void phase_a(uint64_t &acc, const PlanL &p, const float *wP0, const float *wP1,
                                            float (&psv)[kChunk]) const {
        static_assert(K0 % 2 == 0, "frame pairs");
        const int L = (int)lead;
        const int chA = (int)ch - L - p.sA, chB = (int)ch - L - p.sB;
        float gA0 = 0.f, gA1 = 0.f, gB0 = 0.f, gB1 = 0.f, fA0 = 0.f, fA1 = 0.f, fB0 = 0.f, fB1 = 0.f;
        int rA0 = 0, rA1 = 0, rB0 = 0, rB1 = 0;
#pragma unroll
        for (int k = K0; k < kChunk; ++k) {
            if ((k & 1) == 0) {
                const uint64_t pa = acc + (ch ? ps_inc : 0ull);
                const uint32_t ph = hi32(pa);
                float m_gA, m_gB;
                win_gains(unit24(ph), m_gA, m_gB);
                gA0 = pair_even(m_gA); gA1 = pair_odd(m_gA);
                gB0 = pair_even(m_gB); gB1 = pair_odd(m_gB);
                uint32_t di; float fr;
                pitch_split(ph, wi, wf, pmaxu, di, fr);
                const int ra = chA - (int)di;
                rA0 = pair_even_i(ra); rA1 = pair_odd_i(ra);
                fA0 = pair_even(fr); fA1 = pair_odd(fr);
                pitch_split(ph + 0x80000000u, wi, wf, pmaxu, di, fr);
                const int rb = chB - (int)di;
                rB0 = pair_even_i(rb); rB1 = pair_odd_i(rb);
                fB0 = pair_even(fr); fB1 = pair_odd(fr);
            }
            acc += ps_inc;
            const bool odd = k & 1;
            const float *qA = wP0 + (k & ~1) * kRow + (odd ? rA1 : rA0) * kRow;
            const float *qB = wP1 + (k & ~1) * kRow + (odd ? rB1 : rB0) * kRow;
            const float tA = lerp_pair(qA[0], qA[-kRow], odd ? fA1 : fA0);
            const float tB = lerp_pair(qB[0], qB[-kRow], odd ? fB1 : fB0);
            psv[k] = xfade(tB, odd ? gB1 : gB0, tA, odd ? gA1 : gA0);
        }
    }

    // First chunk of a segment (choose_lead has run; the caller has issued the loads of its inputs):
    // shift the phasor, issue the lead-in's line loads, store the inputs, then the kTail positions
    // below the chunk's own -- the lead-in's phase A under chunk 0's line loads, or the direct pass.
    __device__ __forceinline__ void begin_segment(float (&x)[kChunk], int C, const float4 (&xq)[4]) {
        ps_acc -= (uint64_t)lead * ps_inc;
        // the lead-in: positions wpos - L - 16 .. wpos - L - 1 as a chunk written at wpos - 16
        const PlanL li = plan_rf(ps_acc - (uint64_t)kChunk * ps_inc, kChunk);
        const bool leadin = __all(li.okA && li.okB);
        if (leadin) B::template load_lines<1>(li, wpos - (uint32_t)kChunk, true);
        if (COOP) {
            B::stage_rows(xq);
            B::coop_store(true, 0, wpos, C);
            B::read_own(x, C);
        } else {
            B::stage_run(x, 0);
            B::coop_store(true, 0, wpos, C);
        }
        float *wV = region + kPsvWin + lane;
        if (leadin) {
            // (the input staging above lies under the pitch windows: staged after it is read)
            B::template stage_tap<1, 0>();
            B::template stage_tap<1, 1>();
        } else {
            const uint32_t pb = B::own_pb();
            // (rolled by four: the whole pass in flight at once costs registers the chunk loop then spills)
#pragma unroll 1
            for (int m0 = 0; m0 < kTail; m0 += 4) {
                float tv[4];
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    tv[u] = psv_direct(rP, pb, pmask, ps_acc - (uint64_t)(kTail - m0 - u) * ps_inc,
                                       wpos - lead - (uint32_t)(kTail - m0 - u), wi, wf, pmaxu);
#pragma unroll
                for (int u = 0; u < 4; ++u) wV[(m0 + u) * kRow] = tv[u];
            }
        }
        // chunk 0's lines: after the lead-in it carries the lead-in's upper line (set 1) where its
        // window lies one line on, and the loads see the inputs stored above (same wave, issue order)
        pl = plan_rf(ps_acc, C);
        started = false;
        B::template load_lines<0>(pl, wpos, !leadin);
        if (leadin) {
            float psv[kChunk];
            uint64_t acc = ps_acc - (uint64_t)kTail * ps_inc;
            phase_a<kChunk - kTail>(acc, li, region + 0 * kSlots * kRow + lane, region + 1 * kSlots * kRow + lane, psv);
#pragma unroll
            for (int m = 0; m < kTail; ++m) wV[m * kRow] = psv[kChunk - kTail + m];
        }
    }
    // the phasor back on the stream's own time base (the next segment's lead, or finish())
    __device__ __forceinline__ void end_segment() { ps_acc += (uint64_t)lead * ps_inc; }

    // x_{c+1} into the ring, then chunk c+1's plan and line loads (v11's stores_and_next without the
    // psv store)
    template <int PAR>
    __device__ __forceinline__ void stores_and_next(float (&xn)[kChunk], const float4 (&xq)[4], uint32_t w0, int C,
                                                    int Cn, uint64_t ps0) {
        if (COOP) {
            if (Cn > 0) {
                B::stage_rows(xq);
                B::coop_store(true, 0, w0 + (uint32_t)C, Cn);
            }
            B::read_own(xn, Cn);
        } else if (Cn > 0) {
            B::stage_run(xn, 0);
            B::coop_store(true, 0, w0 + (uint32_t)C, Cn);
        }
        pl = plan_rf(ps0 + (uint64_t)C * ps_inc, Cn > 0 ? Cn : 4);
        // after a segment's last chunk nobody reads the lines: the same instructions run against an
        // empty buffer (every load out of range: zeros, no memory access), so the chunk body keeps
        // one shape -- a load under a branch would cost the steady chunks their waits
        const Rsrc ring = rP;
        rP = Cn > 0 ? ring : rNone;
        B::template load_lines<PAR ^ 1>(pl, w0 + (uint32_t)C, false);
        rP = ring;
    }

    // One chunk of C frames with input x; xn / Cn / prefetch / xq as in ChStageL::chunk.  Order:
    //   carry the psv window down; stage the pitch windows, patch in x_c
    //   A  the pitch-shifter over positions w0 - L .. + 15 -> the psv window
    //      x_{c+1} -> ring; plan chunk c+1, issue its line loads
    //   C  chorus tap (from the psv window) + lores~ + outputs, the cover for those loads
    template <int PAR, class Sink, class Prefetch>
    __device__ __forceinline__ void chunk(const float (&x)[kChunk], float (&xn)[kChunk], int C, int Cn, Sink &&sink,
                                          Prefetch &&prefetch, const float4 (&xq)[4]) {
        asm volatile("" : "+v"(lane));
        j = lane >> 1;
        ch = lane & 1u;
        const uint32_t w0 = wpos;
        const uint64_t ps0 = ps_acc;
        const PlanL cur = pl;
        const int L = (int)lead;
        float psv[kChunk];
        float *wP0 = region + 0 * kSlots * kRow + lane;
        float *wP1 = region + 1 * kSlots * kRow + lane;
        float *wV = region + kPsvWin + lane;

        // the newest kTail positions of the chunk before become the old ones of this chunk: all
        // read first, stored after the staging below
        float tv[kTail];
        if (started) {
#pragma unroll
            for (int m = 0; m < kTail; ++m) tv[m] = wV[(kChunk + m) * kRow];
        }
        B::template stage_tap<PAR, 0>();
        B::template stage_tap<PAR, 1>();
        if (started) {
#pragma unroll
            for (int m = 0; m < kTail; ++m) wV[m * kRow] = tv[m];
        }
        // x_c is not in a carried line: frame k -> slot k - s, or the junk slot past the window
        {
            const int limA = kWin + cur.sA, limB = kWin + cur.sB;
            float *pA = wP0 - cur.sA * kRow, *pB = wP1 - cur.sB * kRow;
            const int mA = min(limA, C), mB = min(limB, C);
#pragma unroll
            for (int k = 0; k < kChunk; ++k) {
                pA[min(k, mA) * kRow] = x[k];
                pB[min(k, mB) * kRow] = x[k];
            }
        }
        started = true;
        __builtin_amdgcn_s_setprio(kLoadPrio);
        prefetch();
        __builtin_amdgcn_s_setprio(0);

        const bool fast = C == kChunk && __all(cur.okA && cur.okB);
        if (fast) {
            // A. v11's phase A on the shifted time base
            phase_a<0>(ps_acc, cur, wP0, wP1, psv);
        } else {
            // generic chunk: the positions its frames can read (index < C), straight from the ring
            const uint32_t pb = B::own_pb();
#pragma unroll 1
            for (int k0 = 0; k0 < C; k0 += 4) {          // C is a multiple of 4
                float tv[4];
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    tv[u] = psv_direct(rP, pb, pmask, ps_acc + (uint64_t)(k0 + u) * ps_inc,
                                       w0 - lead + (uint32_t)(k0 + u), wi, wf, pmaxu);
#pragma unroll
                for (int u = 0; u < 4; ++u) wV[(kTail + k0 + u) * kRow] = tv[u];
            }
            ps_acc += (uint64_t)C * ps_inc;
        }
        if (fast) {
#pragma unroll
            for (int k = 0; k < kChunk; ++k) wV[(kTail + k) * kRow] = psv[k];
        }

        stores_and_next<PAR>(xn, xq, w0, C, Cn, ps0);

        if (fast) {
            // C. v11's phase C: frame k reads slot kTail + k - (d - L) and the one below
            const int chC = (int)ch + kTail + L;
            int r0 = 0, r1 = 0;
            float f0 = 0.f, f1 = 0.f;
            uint32_t dn = 0;
            float fn = 0.f;
#pragma unroll
            for (int k = 0; k < kChunk; ++k) {
                if ((k & 1) == 0) {
                    uint32_t di; float fr;
                    if ((k & 3) == 0) {
                        const uint64_t p = lfo_acc + (ch ? lfo_inc : 0ull) + lfo_off;
                        chorus_split2(p, p + 2ull * lfo_inc, D, cmaxd, di, fr, dn, fn);
                    } else {
                        di = dn;
                        fr = fn;
                    }
                    const int rc = chC - (int)di;
                    r0 = pair_even_i(rc); r1 = pair_odd_i(rc);
                    f0 = pair_even(fr); f1 = pair_odd(fr);
                }
                lfo_acc += lfo_inc;
                const bool odd = k & 1;
                const float *qC = wV + (k & ~1) * kRow + (odd ? r1 : r0) * kRow;
                const float wet = lerp_pair(qC[0], qC[-kRow], odd ? f1 : f0);
                const float lp = lores_step(wet, b0, b1, b2, a1, a2, z1, z2);
                sink(k, dry_wet(x[k], dry, lp, mix));
            }
        } else {
#pragma unroll
            for (int k = 0; k < kChunk; ++k) {
                if (k >= C) continue;
                uint32_t di; float fr;
                chorus_split(lfo_acc + lfo_off, D, cmaxd, di, fr);
                lfo_acc += lfo_inc;
                const int jw = kTail + k + L - (int)di;
                const float wet = lerp_pair(wV[jw * kRow], wV[(jw - 1) * kRow], fr);
                const float lp = lores_step(wet, b0, b1, b2, a1, a2, z1, z2);
                sink(k, dry_wet(x[k], dry, lp, mix));
            }
        }
        wpos = w0 + (uint32_t)C;
    }
};

}  // namespace ch
}  // namespace olfx
