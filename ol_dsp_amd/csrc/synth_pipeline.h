// ol_dsp_amd/csrc/synth_pipeline.h -- the seven-wave pipeline of the fused instrument kernels (synth.hip:
// synth_block_v1, synth_svf_block_v1; drumkit.hip: drumkit_block_v1), stated once: voices -> ordered sum ->
// effect rack in one launch, gfx950, wave64.  A kernel supplies its voice (role_v's operations) and its sum
// (role_d's callable); geometry, LDS layout, counters, waits and the D and F roles are here.
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
//                            stands); its input callback forms the ordered sum from queue V (with TOPO the
//                            channel-1 lane takes 0.0f at topology 0); `a` into queue A
//                            [depth 2][16][64]; D1 exits when the group's upper half holds no
//                            instrument, and nobody waits for it then;
//   wave 6 ("F"):            the stub reverb's balance mix, filter_fx / filter1, the output stores.
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
// well-founded and some role can always advance.  The voice type, the sum and the topology change what
// a role computes, not what it waits for: the argument holds for every kernel built from this header.
// The spins are bounded all the same (kSpinMax): a wave that gives up goes on with stale data instead
// of hanging the device.  The grid is one workgroup per 64 instruments (not persistent).
#pragma once
#include "rack_delay_stage.h"
#include "lds_flags.h"
#include "voice_roles.h"

namespace olfx {
namespace sy {

constexpr int kVWaves = 4;                                // voice waves
constexpr int kThreads = (kVWaves + 3) * 64;              // + D0, D1, F
constexpr int kChunk = fr::kChunk;
constexpr int kQ = kChunk * 64;                           // floats of one (voice, chunk) or one queue-A buffer
constexpr int kDepthV = 2, kDepthA = 2;
constexpr int kFlags = 16;
constexpr uint32_t kSpinMax = 1u << 22;                   // x s_sleep(1): ~0.1 s, five orders above any real wait
enum { F_V0 = 0, F_R0 = kVWaves, F_R1, F_D0, F_D1, F_FIN };

// LDS of a workgroup, in floats: the D waves' two regions, queue V, queue A, the counters, the V waves'
// event slots, then `extra` floats for each V wave (the kernel's own)
constexpr size_t lds_floats(uint32_t voices, uint32_t extra) {
    return 2 * (size_t)fr::kRegion + (size_t)kDepthV * voices * kQ + (size_t)kDepthA * kQ + kFlags +
           (size_t)kVWaves * 64 * 2 + (size_t)kVWaves * extra;
}
static_assert((2 * fr::kRegion) % 4 == 0, "16-byte aligned queues");

template <class Cond>
__device__ __forceinline__ void wait(Cond &&cond) {
    for (uint32_t t = 0; !cond() && t < kSpinMax; ++t) __builtin_amdgcn_s_sleep(1);
}

// A wave's view of its workgroup: the LDS carve and the block's shape.
struct Wg {
    float *lds;                 // the D waves' regions [2][fr::kRegion]
    float *vq;                  // voices -> delay   [kDepthV][P][16][64]
    float *aq;                  // delay -> filter   [kDepthA][16][64]
    uint32_t *flags;
    uint2 *evslots;             // [kVWaves][64]
    float *extra;               // [kVWaves][extra]
    uint32_t wib, lane, g;      // wave in the workgroup, lane, the group: instruments 64 g ..
    uint32_t n, nf, P, nchunks, nvw;
    bool d1_on;                 // the group's upper half holds an instrument
};
// Every thread of the kernel calls this first: it zeroes the counters behind the pipeline's only barrier.
__device__ __forceinline__ Wg enter(const InstrumentArgs &a, float *lds) {
    const uint32_t tid = threadIdx.x;
    Wg b;
    b.lds = lds;
    b.vq = lds + 2 * fr::kRegion;
    b.aq = b.vq + (size_t)kDepthV * a.voices * kQ;
    b.flags = (uint32_t *)(b.aq + kDepthA * kQ);
    b.evslots = (uint2 *)(b.flags + kFlags);
    b.extra = (float *)(b.evslots + kVWaves * 64);
    b.wib = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    b.lane = tid & 63u;
    b.g = blockIdx.x;
    b.n = a.n, b.nf = a.n_frames, b.P = a.voices;
    b.nchunks = (b.nf + kChunk - 1) / kChunk;
    b.nvw = min(b.P, (uint32_t)kVWaves);
    b.d1_on = b.g * 64u + 32u < b.n;
    if (tid < kFlags) b.flags[tid] = 0;
    __syncthreads();
    return b;
}
__device__ __forceinline__ bool is_v(const Wg &b) { return b.wib < (uint32_t)kVWaves; }
__device__ __forceinline__ bool is_d(const Wg &b) { return !is_v(b) && b.wib < (uint32_t)kVWaves + 2u; }
// a V lane's instrument: lanes past n mirror instrument n - 1 exactly (same state, coefficients and events),
// so their stores write the values its own lane writes (as voice_block_v4's dead lanes)
__device__ __forceinline__ uint32_t v_instrument(const Wg &b) { return min(b.g * 64u + b.lane, b.n - 1u); }
// a D lane's instrument (two channel lanes each), clamped likewise
__device__ __forceinline__ uint32_t d_instrument(const Wg &b) {
    return min(b.g * 64u + 32u * (b.wib - kVWaves) + (b.lane >> 1), b.n - 1u);
}

// ---------------- V: voice slots wib and wib + 4, lane = instrument ----------------
// load(v, p) / store(v, p): voice slot p's state into and out of v; fetch(v, m, x): what the voice can do for a
// chunk of m frames ahead of the queue-V wait, its latency hidden under the previous chunk's consumers, handed on
// in an X; run(v, x, q, m): the voice's samples of that chunk -> q[k * 64] (its column of queue V).
//
// SEG (timed notes, the *_seg kernels; a = the launch's arguments): only this role sees note events -- D is continuous
// in time, and F but for its six coefficients (role_f, TP) -- so the chunk grid, the queues, every counter and every
// wait stay as they are, and a V wave splits a chunk's frames at the segment starts that fall inside it (multiples of 4: they can fall in mid-chunk).
// The pieces' samples go to the same queue-V columns, q[(k0 + k) * 64]; the wave waits once and publishes F_V
// once per chunk, as without segments.  At a segment start, for va and vb in turn, start(v, p, ev) does from
// registers what load does at a launch's start (voice_envs_restart and the voice's own events).  fetch runs per
// piece -- the first piece's ahead of the wait, as ever -- so nothing fetched spans a segment start.  The next
// segment's records and start frame are read one segment ahead (seg_event_fetch); the starts are clamped to the
// block and forced to ascend, whatever the table holds, so a piece is 1 .. m frames inside its chunk.
// Timed parameters (tp; olfx_timed_instrument_params): a voice slot's table entry of the next segment is read one
// segment ahead with its events (wave-uniform: scalar registers), and at the segment start start(v, p, ev, r) gets
// the lane's voice record r (seg_inst_record; kNoCoef: none), which it takes ahead of the events -- parameters
// precede notes.  TP is an instantiation of its own (the *_seg_tp kernels): a launch without such records runs the
// SEG code as it was, start(v, p, ev) and all.
template <class V, class X, bool SEG = false, bool TP = false, class Load, class Run, class Store, class Fetch,
          class Start = std::nullptr_t>
__device__ __forceinline__ void role_v(const Wg &b, Load &&load, Run &&run, Store &&store, Fetch &&fetch,
                                       const InstrumentArgs *a = nullptr, Start &&start = nullptr,
                                       const InstrumentTimed *tp = nullptr) {
    const uint32_t wib = b.wib;
    if (wib >= b.nvw) return;
    const bool two = wib + (uint32_t)kVWaves < b.P;
    V va, vb;
    load(va, wib);
    if (two) load(vb, wib + kVWaves);
    else vb = va;                                          // (never run, never stored)
    // SEG: the next segment, its start frame and its records of this wave's one or two voice-slot groups
    [[maybe_unused]] uint32_t sgi = 1u, S = 1u, nb = b.nf, gpa = 0u, gpb = 0u, groups = 0u, me = 0u;
    [[maybe_unused]] uint2 pa = make_uint2(0u, 0u), pb = make_uint2(0u, 0u);
    [[maybe_unused]] uint2 *slots = b.evslots + wib * 64u;
    [[maybe_unused]] uint4 ta = make_uint4(0u, 0u, 0u, 0u), tb = ta;
    [[maybe_unused]] uint32_t tga = 0u, tgb = 0u;
    [[maybe_unused]] auto ahead = [&] {
        if (sgi < S) {
            const uint32_t f = a->seg[sgi], lo = nb;       // (nb: the previous start)
            pa = seg_event_fetch(a->ev, sgi, groups, gpa, b.lane);
            if (two) pb = seg_event_fetch(a->ev, sgi, groups, gpb, b.lane);
            if constexpr (TP) {
                ta = tp->vtab[(size_t)sgi * tp->gv + tga];
                tb = tp->vtab[(size_t)sgi * tp->gv + tgb];
            }
            nb = min(max(f, lo), b.nf);
        } else {
            nb = b.nf;
        }
    };
    if constexpr (SEG) {
        S = min(a->n_seg, kSegCap);
        groups = b.P * (a->npad >> 6);
        gpa = wib * (a->npad >> 6) + b.g;
        gpb = (wib + kVWaves) * (a->npad >> 6) + b.g;
        me = v_instrument(b) - b.g * 64u;
        if constexpr (TP) {
            // the table's group of each voice slot: the slot's own (a kit), or the instrument group (tp->gv = npad / 64)
            const bool per_slot = tp->gv != (a->npad >> 6);
            tga = per_slot ? gpa : b.g;
            tgb = per_slot && two ? gpb : tga;
        }
        nb = 0u;
        ahead();
    }
    for (uint32_t ck = 0; ck < b.nchunks; ++ck) {
        const uint32_t m = min((uint32_t)kChunk, b.nf - ck * kChunk);
        float *q = b.vq + (size_t)(ck % kDepthV) * b.P * kQ + b.lane;
        auto taken = [&] {                                 // the chunk's queue-V buffer was taken by D0 and D1
            return flag_get(b.flags + F_R0) + kDepthV > ck && (!b.d1_on || flag_get(b.flags + F_R1) + kDepthV > ck);
        };
        if constexpr (!SEG) {
            X xa, xb;
            fetch(va, m, xa);
            if (two) fetch(vb, m, xb);
            wait(taken);
            run(va, xa, q + wib * kQ, m);
            if (two) run(vb, xb, q + (wib + kVWaves) * kQ, m);
        } else {
            const uint32_t f0 = ck * kChunk;
            bool waited = false;
            for (uint32_t k0 = 0; k0 < m;) {
                while (sgi < S && nb == f0 + k0) {         // a segment starts at this frame
                    if constexpr (TP) {
                        start(va, wib, seg_event_take(pa, a->ev_more, slots, b.lane, me), seg_inst_record(ta, me, tp->n_v));
                        if (two)
                            start(vb, wib + kVWaves, seg_event_take(pb, a->ev_more, slots, b.lane, me),
                                  seg_inst_record(tb, me, tp->n_v));
                    } else {
                        start(va, wib, seg_event_take(pa, a->ev_more, slots, b.lane, me));
                        if (two) start(vb, wib + kVWaves, seg_event_take(pb, a->ev_more, slots, b.lane, me));
                    }
                    ++sgi;
                    ahead();
                }
                // (nb > f0 + k0 now, or no segment is left and nb = nf: the piece has a frame at least)
                const uint32_t k1 = sgi < S ? min(m, nb - f0) : m, len = k1 - k0;
                X xa, xb;
                fetch(va, len, xa);
                if (two) fetch(vb, len, xb);
                if (!waited) wait(taken);
                waited = true;
                run(va, xa, q + wib * kQ + k0 * 64u, len);
                if (two) run(vb, xb, q + (wib + kVWaves) * kQ + k0 * 64u, len);
                k0 = k1;
            }
        }
        flag_put(b.flags + F_V0 + wib, ck + 1);
    }
    store(va, wib);
    if (two) store(vb, wib + kVWaves);
}
// a voice with nothing to fetch: run(v, q, m)
template <class V, bool SEG = false, bool TP = false, class Load, class Run, class Store, class Start = std::nullptr_t>
__device__ __forceinline__ void role_v(const Wg &b, Load &&load, Run &&run, Store &&store, const InstrumentArgs *a = nullptr,
                                       Start &&start = nullptr, const InstrumentTimed *tp = nullptr) {
    struct None {};
    role_v<V, None, SEG, TP>(
        b, load, [&](V &v, None &, float *q, uint32_t m) { run(v, q, m); }, store, [](V &, uint32_t, None &) {}, a, start, tp);
}

// ---------------- D: the delay stage, per (instrument, channel) lane ----------------
// sum(q, m): the ordered sum of the voices' chunk at q[p * kQ + k * 64] into m[k] (zeroed).  TOPO: the rack's
// topology per instrument (FRC_TOPO), else topology 1.
template <bool TOPO, class Sum>
__device__ __forceinline__ void role_d(const Wg &b, const InstrumentArgs &a, Sum &&sum) {
    const uint32_t lane = b.lane, dw = b.wib - kVWaves;
    const uint32_t inst0 = b.g * 64u + 32u * dw;
    if (inst0 >= b.n) return;                              // D1 of a group whose upper half is empty
    const uint32_t col = 32u * dw + (lane >> 1);           // this lane's instrument within the group
    // FxRack<2>::Process runs on the frame (sum, 0.0f): the channel-1 lane of a topology-0 instrument
    bool ch1_zero = false;
    if constexpr (TOPO) ch1_zero = (lane & 1u) != 0u && a.fr_coef[FRC_TOPO * b.n + d_instrument(b)] == 0u;
    auto mono = [&](uint32_t f0, int Cx, float (&xv)[kChunk]) {
        if (Cx == 0) {                                     // past the block's end: nothing to wait for
#pragma unroll
            for (int k = 0; k < kChunk; ++k) xv[k] = 0.f;
            return;
        }
        const uint32_t ck = f0 / kChunk;
        wait([&] {
            bool ok = true;
            for (uint32_t w = 0; w < b.nvw; ++w) ok = ok && flag_get(b.flags + F_V0 + w) > ck;
            return ok;
        });
        float m[kChunk];
#pragma unroll
        for (int k = 0; k < kChunk; ++k) m[k] = 0.0f;
        sum(b.vq + (size_t)(ck % kDepthV) * b.P * kQ + col, m);
        flag_put(b.flags + F_R0 + dw, ck + 1);            // (the release waits for these reads)
#pragma unroll
        for (int k = 0; k < kChunk; ++k) xv[k] = k < Cx && !ch1_zero ? m[k] : 0.f;
    };
    auto put = [&](uint32_t ck, const float (&av)[kChunk]) {
        wait([&] { return flag_get(b.flags + F_FIN) + kDepthA > ck; });
        float *q = b.aq + (ck % kDepthA) * kQ + col;
        if ((lane & 1u) == 0u) {                           // channel 0's at either topology (the even lane's own)
#pragma unroll
            for (int k = 0; k < kChunk; ++k) q[k * 64] = av[k];
        }
        flag_put(b.flags + F_D0 + dw, ck + 1);
    };
    fr::delay_stage_from(a.ring, a.fr_state, a.fr_coef, b.n, b.nf, a.t0, b.lds + dw * fr::kRegion, lane, inst0, mono, put);
}

// ---------------- F: the stub reverb's balance mix, filter_fx / filter1, the stores; lane = instrument ----------------
// TP (the *_seg_tp kernels; tp->ftab; olfx_timed_instrument_params): the six coefficients are loop-carried.  F reads
// the segment table itself, one start and its table entry ahead; a chunk that holds a start (k = 0, 4, 8 or 12) runs
// a second copy of the sample loop that, at each quad, lets the lanes with a rack record of a segment starting there
// take it (seg_inst_record).  Every other chunk runs the loop it always ran; the waits and counters are unchanged.
template <bool TOPO, bool TP = false>
__device__ __forceinline__ void role_f(const Wg &b, const InstrumentArgs &a, const InstrumentTimed *tp = nullptr) {
    const uint32_t n = b.n, i_raw = b.g * 64u + b.lane;
    const bool valid = i_raw < n;
    const uint32_t i = valid ? i_raw : n - 1;
    float rbal = __uint_as_float(a.fr_coef[FRC_RBAL * n + i]);
    float ffreq = __uint_as_float(a.fr_coef[FRC_FFREQ * n + i]);
    float fdamp = __uint_as_float(a.fr_coef[FRC_FDAMP * n + i]);
    float fdrive = __uint_as_float(a.fr_coef[FRC_FDRIVE * n + i]);
    uint32_t ftype = a.fr_coef[FRC_FTYPE * n + i];
    float master = __uint_as_float(a.fr_coef[FRC_MASTER * n + i]);   // 1.0f: topology 1 (derive_fxrack)
    // TP: the segments F has yet to reach, the next one's start (clamped and ascending, as V's) and table entry
    [[maybe_unused]] uint32_t fS = 1u, fsg = 1u, fnb = b.nf;
    [[maybe_unused]] uint4 fe = make_uint4(0u, 0u, 0u, 0u);
    [[maybe_unused]] const uint32_t fgroups = a.npad >> 6;
    [[maybe_unused]] auto fahead = [&](uint32_t lo) {
        if (fsg < fS) {
            fnb = min(max(a.seg[fsg], lo), b.nf);
            fe = tp->ftab[(size_t)fsg * fgroups + b.g];
        } else {
            fnb = b.nf;
        }
    };
    if constexpr (TP) {
        if (tp->n_f) fS = min(a.n_seg, kSegCap);
        fahead(0u);
    }
    // topology 0: FilterFx<2> writes channel 0 of the zeroed buf_c only, so out 1 = 0.0f x master
    bool fw = true;
    if constexpr (TOPO) fw = a.fr_coef[FRC_TOPO * n + i] == 1u;
    float flow = __uint_as_float(a.fr_state[FRS_FLOW * n + i]);
    float fband = __uint_as_float(a.fr_state[FRS_FBAND * n + i]);
    float *const o0 = a.out + i, *const o1 = a.out + a.plane + i;
    for (uint32_t ck = 0; ck < b.nchunks; ++ck) {
        const uint32_t f0 = ck * kChunk;
        const uint32_t C = min((uint32_t)kChunk, b.nf - f0);
        wait([&] { return flag_get(b.flags + F_D0) > ck && (!b.d1_on || flag_get(b.flags + F_D1) > ck); });
        const float *q = b.aq + (ck % kDepthA) * kQ + b.lane;
        float a0[kChunk];
#pragma unroll
        for (int k = 0; k < kChunk; ++k) a0[k] = q[k * 64];
        flag_put(b.flags + F_FIN, ck + 1);                 // (the release waits for these reads)
        if constexpr (TP) {
            if (fsg < fS && fnb < f0 + C) {                // wave-uniform: a segment starts inside this chunk
#pragma unroll
                for (int k = 0; k < kChunk; ++k) {
                    if ((uint32_t)k < C) {
                        if ((k & 3) == 0) {
                            while (fsg < fS && fnb <= f0 + (uint32_t)k) {
                                const uint32_t r = seg_inst_record(fe, i - b.g * 64u, tp->n_f);
                                if (r != kNoCoef) {
                                    const uint32_t *w = tp->frec + r;
                                    const size_t T = tp->n_f;
                                    rbal = __uint_as_float(w[TIF_RBAL * T]);
                                    ffreq = __uint_as_float(w[TIF_FFREQ * T]);
                                    fdamp = __uint_as_float(w[TIF_FDAMP * T]);
                                    fdrive = __uint_as_float(w[TIF_FDRIVE * T]);
                                    ftype = w[TIF_FTYPE * T];
                                    master = __uint_as_float(w[TIF_MASTER * T]);
                                }
                                ++fsg;
                                fahead(fnb);
                            }
                        }
                        const float vb = a0[k] * 0.8f;
                        const float b0 = (vb * rbal) + (a0[k] * (1 - rbal));
                        const float c0 = fr::svf_tick(b0, ffreq, fdamp, fdrive, ftype, flow, fband);
                        if (valid) {
                            o0[(size_t)(f0 + k) * n] = c0 * master;
                            o1[(size_t)(f0 + k) * n] = (fw ? b0 : 0.0f) * master;
                        }
                    }
                }
                continue;
            }
        }
#pragma unroll
        for (int k = 0; k < kChunk; ++k) {
            if ((uint32_t)k < C) {                         // C is wave-uniform
                // ReverbFx over the ReverbSc stub (fxrack.hip): stereo[0] = stereo[1], so b1 = b0
                const float vb = a0[k] * 0.8f;
                const float b0 = (vb * rbal) + (a0[k] * (1 - rbal));
                // FilterFx<2> in place: the Svf on channel 0, channel 1 keeps the reverb's output
                const float c0 = fr::svf_tick(b0, ffreq, fdamp, fdrive, ftype, flow, fband);
                if (valid) {
                    o0[(size_t)(f0 + k) * n] = c0 * master;
                    o1[(size_t)(f0 + k) * n] = (fw ? b0 : 0.0f) * master;
                }
            }
        }
    }
    if (valid) {
        a.fr_state[FRS_FLOW * n + i] = __float_as_uint(flow);
        a.fr_state[FRS_FBAND * n + i] = __float_as_uint(fband);
    }
}

// The launch both kinds share: one workgroup per 64 instruments, its seven waves dispatched together.
template <class Args>
hipError_t launch(void (*kernel)(Args), const Args &a, uint32_t extra, hipStream_t s) {
    hipLaunchKernelGGL(kernel, dim3(a.npad / 64u), dim3(kThreads), lds_floats(a.voices, extra) * sizeof(float), s, a);
    return hipGetLastError();
}

}  // namespace sy
}  // namespace olfx
