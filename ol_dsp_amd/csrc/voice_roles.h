// ol_dsp_amd/csrc/voice_roles.h -- the SynthVoice pieces that the voice kernels share: the note-event
// staging, the Adsr segment machine, Svf::SetFreq's helpers and the three Svf-voice roles that do
// not depend on the sound source (ENV, FREQ, FILT of voice_block_v5).  voice.hip (the polyBLEP saw)
// and sampler.hip (sample playback) build their kernels from them, so both run the same envelope and
// filter arithmetic, operation for operation.  Everything is forced inline: a role's body is compiled
// into its kernel exactly as when it was written there.
#pragma once
#include "olfx_internal.h"

namespace olfx {
namespace {

enum { SEG_IDLE = 0, SEG_ATTACK = 1, SEG_DECAY = 2, SEG_RELEASE = 3 };

// sin(x) for x in [0, pi/4] (Svf::SetFreq's argument pi * min(0.25, fc / 2sr)): odd Taylor
// polynomial to x^9 in Horner form, truncation < 2e-9; branch-free.
__device__ __forceinline__ float sin_quarter(float x) {
    const float x2 = x * x;
    float p = __builtin_fmaf(2.7557319e-6f, x2, -1.9841270e-4f);     // 1/9!, -1/7!
    p = __builtin_fmaf(p, x2, 8.3333333e-3f);                        // 1/5!
    p = __builtin_fmaf(p, x2, -1.6666667e-1f);                       // -1/3!
    return __builtin_fmaf(x * x2, p, x);
}

// the cutoff sum (SynthVoice.h:46-47) clamped as Svf::SetFreq clamps it, fclamp(f, 1e-6, sr / 3):
// fminf(fmaxf(f, 1e-6), fc_max) for 1e-6 <= fc_max and a non-NaN sum (ENV hands it to FREQ clamped:
// the ENV + FILT SIMDs had the spare issue slots)
__device__ __forceinline__ float svf_fc(float f, float fc_max) { return __builtin_amdgcn_fmed3f(f, 1.0e-6f, fc_max); }

// Svf::SetFreq's damping, negated for FILT: -min(damp_res, min(2, lim)) = max(-damp_res, -2, -lim),
// one v_max3 (the negations are operand modifiers); equal for every non-NaN lim
__device__ __forceinline__ float neg_damp(float damp_res, float lim) {
    return __builtin_fmaxf(__builtin_fmaxf(-damp_res, -2.0f), -lim);
}

// packed FP32 (v_pk_mul_f32 / v_pk_add_f32: two IEEE operations per lane and instruction, the same
// bits as two scalar ones)
typedef float f2 __attribute__((ext_vector_type(2)));

// The block's folded note events (VoiceArgs::ev, VEV_*) of this lane's voice: the wave reads its
// workgroup's fixed slots (lanes 0 .. kVevCap-1, one host-link round trip; a crowded workgroup's
// overflow list is a second one), stages the records into its own 64 LDS slots, slot = voice within
// the group, and each lane reads its own.  `me` is the lane's voice within the group (dead lanes of
// the last group mirror voice n-1, so they read its slot too).  No events: one uniform test.
struct VoiceEv {
    uint32_t op;
    float freq;
};
// `group`: the 64-voice group whose slots these are (a voice kernel's workgroup; the synth's voice
// slot p of a 64-instrument group, synth.hip).
__device__ __forceinline__ VoiceEv voice_event_of(const uint2 *evs, const uint2 *evs_more, uint2 *slot, uint32_t lane,
                                                  uint32_t me, uint32_t group) {
    VoiceEv r{0u, 0.0f};
    if (!evs) return r;
    uint2 e = make_uint2(0u, 0u);
    if (lane < kVevCap) e = evs[group * kVevCap + lane];
    slot[lane] = make_uint2(0u, 0u);
    const uint32_t head = __builtin_amdgcn_readfirstlane(e.x);
    if ((head >> 8) & VEV_MORE) {
        const uint32_t cnt = head >> 16, first = __builtin_amdgcn_readfirstlane(e.y);
        e = make_uint2(0u, 0u);
        if (lane < cnt) e = evs_more[first + lane];
    }
    if (e.x >> 8) slot[e.x & 63u] = make_uint2(e.x >> 8, e.y);
    // one wave writes and reads its slots: LDS operations of a wave complete in order; the fences
    // keep the compiler from moving the read above the other lanes' writes
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const uint2 v = slot[me];
    r.op = v.x;
    r.freq = __uint_as_float(v.y);
    return r;
}
// the voice kernels: the group is the workgroup
__device__ __forceinline__ VoiceEv voice_event(const VoiceArgs &a, uint2 *slot, uint32_t lane, uint32_t me) {
    return voice_event_of(a.ev, a.ev_more, slot, lane, me, blockIdx.x);
}

// Another wave's view of slots voice_event staged, after a workgroup barrier.
__device__ __forceinline__ VoiceEv staged_event(const VoiceArgs &a, const uint2 *slot, uint32_t me) {
    VoiceEv r{0u, 0.0f};
    if (!a.ev) return r;
    const uint2 v = slot[me];
    r.op = v.x;
    r.freq = __uint_as_float(v.y);
    return r;
}

// ---- timed events: a launch of several segments (olfx_layout.h kSegCap, VoiceArgs::seg) ----
// A segmented kernel's block is the concatenation of its segments' chunks: chunking restarts at each
// segment start, so every frame takes the arithmetic path it takes when each segment is a launch of its
// own, and at a segment's first chunk a role does from registers what it does at a launch's start.
// The LDS of such a kernel: the segments' bounds (start[n_seg] = n_frames) and every segment's staged
// records, slot = voice within the group.  A slot set per segment, all staged before the first barrier:
// a role that runs a step or two behind ENV reads a segment's records however short the segments are,
// and the host-link reads of all segments are in flight together, ahead of the chunk loop.
// ... and, with timed parameters, the number of the group's first coefficient record of each segment (tc_base).
struct VoiceSegs {
    uint32_t start[kSegCap + 1];
    uint32_t cbase[kSegCap];
    uint2 slot[kSegCap][64];
};
// The bounds, by the workgroup's first threads (the caller's next barrier publishes them); clamped to the
// block, whatever the table holds.
__device__ __forceinline__ void voice_segs_bounds(const VoiceArgs &a, VoiceSegs &sg) {
    const uint32_t t = threadIdx.x, S = a.n_seg;
    if (t <= S && t <= kSegCap) {
        const uint32_t f = (t == 0u || t == S) ? 0u : a.seg[t];
        sg.start[t] = t == S ? a.n_frames : (f < a.n_frames ? f : a.n_frames);
    }
    if (t < S && t < kSegCap) sg.cbase[t] = a.tc_base ? a.tc_base[(size_t)t * ((a.n + 63u) / 64u) + blockIdx.x] : 0u;
}
// Every segment's records of `group` into sg.slot, by one wave: all the fixed-slot reads first (one
// host-link round trip for the lot), then the crowded segments' overflow runs (a second), then the slots.
__device__ __forceinline__ void voice_events_stage(const VoiceArgs &a, VoiceSegs &sg, uint32_t lane, uint32_t group) {
    const uint32_t S = a.n_seg < kSegCap ? a.n_seg : kSegCap;
    const size_t per_seg = (size_t)((a.n + 63u) / 64u) * kVevCap;
    uint2 e[kSegCap];
#pragma unroll
    for (uint32_t s = 0; s < kSegCap; ++s) {
        e[s] = make_uint2(0u, 0u);
        if (s < S && lane < kVevCap) e[s] = a.ev[s * per_seg + group * kVevCap + lane];
    }
#pragma unroll
    for (uint32_t s = 0; s < kSegCap; ++s) {
        if (s < S) {
            const uint32_t head = __builtin_amdgcn_readfirstlane(e[s].x);
            if ((head >> 8) & VEV_MORE) {
                const uint32_t cnt = head >> 16, first = __builtin_amdgcn_readfirstlane(e[s].y);
                e[s] = make_uint2(0u, 0u);
                if (lane < cnt) e[s] = a.ev_more[first + lane];
            }
        }
    }
#pragma unroll
    for (uint32_t s = 0; s < kSegCap; ++s) {
        if (s < S) {
            sg.slot[s][lane] = make_uint2(0u, 0u);
            if (e[s].x >> 8) sg.slot[s][e[s].x & 63u] = make_uint2(e[s].x >> 8, e[s].y);
        }
    }
    // as voice_event_of: one wave writes and reads its slots in order; other waves read after a barrier
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ VoiceEv seg_event(const VoiceSegs &sg, uint32_t seg, uint32_t me) {
    const uint2 v = sg.slot[seg][me];
    return VoiceEv{v.x, __uint_as_float(v.y)};
}
// Timed parameters (olfx_timed_params): a voice whose segment record has VEV_COEF takes new coefficients at that
// segment's start.  Each role reloads its own words at ITS segment start (the roles run a step or two apart),
// before it does what it does at a launch's start, and keeps them until the voice's next such record.  The
// records are read straight from the packet; no per-record index: a group's records of a segment are
// consecutive from cbase[seg], by voice, so a lane's is cbase + the lower live lanes that have one too.  Dead
// lanes of the last group mirror voice n - 1: they are left out of the vote and take that lane's rank (`me`).
// Returns the record's number, or kNoCoef (also for a number outside the section, whatever the packet holds).
constexpr uint32_t kNoCoef = 0xFFFFFFFFu;
__device__ __forceinline__ uint32_t seg_coef_record(const VoiceArgs &a, const VoiceSegs &sg, uint32_t seg, const VoiceEv &ev,
                                                    uint32_t n, uint32_t me) {
    if (!a.tc) return kNoCoef;                             // a launch without timed parameters: one scalar test
    const bool has = (ev.op & VEV_COEF) != 0u;
    const bool live = blockIdx.x * 64u + (threadIdx.x & 63u) < n;
    const uint64_t votes = __builtin_amdgcn_ballot_w64(has && live);
    if (!votes) return kNoCoef;                            // wave-uniform: the common segment start
    const uint32_t r = sg.cbase[seg] + (uint32_t)__builtin_popcountll(votes & ((1ull << me) - 1ull));
    return has && r < a.tc_n ? r : kNoCoef;
}
__device__ __forceinline__ float seg_coef(const VoiceArgs &a, uint32_t r, uint32_t word) {
    return __uint_as_float(a.tc[(size_t)word * a.tc_n + r]);
}

// A role's place in the launch's chunk sequence (wave-uniform): the chunk's first frame, its segment and
// whether it starts it.  SEG = false: nothing (the roles index chunks by step, as they always have).
template <bool SEG>
struct SegCursor {
    __device__ __forceinline__ SegCursor(const VoiceSegs *, uint32_t) {}
    __device__ __forceinline__ uint32_t len() const { return 0u; }
    __device__ __forceinline__ void next() {}
    static constexpr uint32_t f0 = 0u, seg = 0u, end = 0u;
    static constexpr bool first = false;
};
template <>
struct SegCursor<true> {
    const VoiceSegs *sg;
    uint32_t n_seg, seg, f0, end;
    bool first;
    __device__ __forceinline__ SegCursor(const VoiceSegs *s, uint32_t n)
        : sg(s), n_seg(n), seg(0u), f0(0u), end(__builtin_amdgcn_readfirstlane(s->start[1])), first(true) {}
    __device__ __forceinline__ uint32_t len() const {
        const uint32_t d = end - f0;
        return d < (uint32_t)8 ? d : (uint32_t)8;          // kVcChunk (below)
    }
    __device__ __forceinline__ void next() {
        f0 += len();
        first = false;
        if (f0 == end && seg + 1u < n_seg) {
            ++seg;
            const uint32_t e1 = __builtin_amdgcn_readfirstlane(sg->start[seg + 1u]);
            end = e1 > f0 ? e1 : f0;                       // (ascending by the host's construction)
            first = true;
        }
    }
};

// NoteOn / GateOn / NoteOff / GateOff on the envelope flags word and levels (SynthVoice.h:231-251):
// Retrigger(true) = mode ATTACK and x = 0 for the amp (bits 0-2) and filter (bits 3-5) envelopes;
// the gate is bit 8
__device__ __forceinline__ void apply_gate_events(const VoiceEv &ev, uint32_t &flags, float &xa, float &xf) {
    if (ev.op & VEV_RETRIGGER) {
        flags = (flags & ~0x3Fu) | 1u | (1u << 3);
        xa = 0.0f;
        xf = 0.0f;
    }
    if (ev.op & VEV_GATE_SET) flags = (flags & ~0x100u) | ((ev.op & VEV_GATE_ON) ? 0x100u : 0u);
}

}  // namespace

// daisysp::Adsr as a segment machine.  The gate is constant inside a block (note events apply
// between blocks; with timed events, inside each of the block's event segments, and begin() runs at
// every segment start), so the gate-edge test of Adsr::Process only fires on the first sample:
// it is applied once in begin(), and each sample is the segment update x += d0 (target - x)
// followed by the segment's clamp -- ATTACK ends above 1 (-> DECAY at x = 1), DECAY / RELEASE end
// below 0 (-> IDLE at x = 0) -- which is v_med3(xn, lo, hi) with the segment's (lo, hi).  The
// segment ends in a lane only a few times per note, so the parameter switch runs behind a
// wave-uniform test.  IDLE is d0 = 0, target 0 and no bounds: x stays 0, Adsr's IDLE output (x is 0
// whenever the envelope is idle: it enters IDLE at 0 and leaves only through Retrigger).
struct Env {
    float x, d0, tgt, hi, lo;
    uint32_t mode;
    float dec_d0, sus;

    __device__ __forceinline__ void set_segment(uint32_t m, float atk_d0, float atk_tgt, float rel_d0) {
        const float inf = __builtin_inff();
        const bool atk = m == SEG_ATTACK, dcy = m == SEG_DECAY, rel = m == SEG_RELEASE;
        mode = m;
        d0 = atk ? atk_d0 : (dcy ? dec_d0 : (rel ? rel_d0 : 0.0f));
        tgt = atk ? atk_tgt : (dcy ? sus : (rel ? -0.01f : 0.0f));
        hi = atk ? 1.0f : inf;
        lo = (dcy || rel) ? 0.0f : -inf;
    }
    __device__ __forceinline__ void begin(bool gate, bool &gprev, uint32_t m, float x0, float atk_d0, float atk_tgt,
                                          float dec, float rel_d0, float s) {
        m = (gate && !gprev) ? (uint32_t)SEG_ATTACK : ((!gate && gprev) ? (uint32_t)SEG_RELEASE : m);
        gprev = gate;
        x = x0;
        dec_d0 = dec;
        sus = s;
        set_segment(m, atk_d0, atk_tgt, rel_d0);
    }
    // the same update with no segment switch, for a chunk computed speculatively: returns the
    // sample and records in `ended` whether the segment ended (then the chunk is redone by step())
    __device__ __forceinline__ float step_spec(bool &ended) {
        const float xn = x + d0 * (tgt - x);
        ended = ended || xn > hi || xn < lo;
        x = xn;                                          // == v_med3(xn, lo, hi) while inside
        return x;
    }
    __device__ __forceinline__ float step() {
        const float xn = x + d0 * (tgt - x);
        const bool ends = xn > hi || xn < lo;
        x = __builtin_amdgcn_fmed3f(xn, lo, hi);
        if (__builtin_amdgcn_ballot_w64(ends)) {       // rare, wave-uniform: a segment ended
            // every lane evaluates the switch and keeps it only where its segment ended (selects,
            // no exec-masked block)
            const float inf = __builtin_inff();
            const bool to_dcy = mode == SEG_ATTACK;
            d0 = ends ? (to_dcy ? dec_d0 : 0.0f) : d0;
            tgt = ends ? (to_dcy ? sus : 0.0f) : tgt;
            hi = ends ? inf : hi;
            lo = ends ? (to_dcy ? 0.0f : -inf) : lo;
            mode = ends ? (to_dcy ? (uint32_t)SEG_DECAY : (uint32_t)SEG_IDLE) : mode;
        }
        return x;
    }
};

// The envelopes and the gate of a voice that one lane holds for a whole block (synth.hip, drumkit.hip).
struct VoiceEnvs {
    Env ea, ef;
    bool gate, gprev_a, gprev_f;
};
// Voice slot si of state planes of stride sn, with the coefficients at ci of planes of stride cn: the flag word
// and levels, the block's gate events of `group` on them (returned for the caller's own events), both
// Env::begin.  The state loads are issued before the event read, as voice_role_env's.
__device__ __forceinline__ VoiceEv voice_envs_load(VoiceEnvs &v, const float *s, uint32_t sn, uint32_t si, const float *c,
                                                   uint32_t cn, uint32_t ci, const uint2 *evs, const uint2 *evs_more,
                                                   uint2 *slot, uint32_t lane, uint32_t me, uint32_t group) {
    uint32_t flags0 = __float_as_uint(s[VCS_FLAGS * sn + si]);
    float xa0 = s[VCS_ENVA_X * sn + si], xf0 = s[VCS_ENVF_X * sn + si];
    const VoiceEv ev = voice_event_of(evs, evs_more, slot, lane, me, group);
    apply_gate_events(ev, flags0, xa0, xf0);
    v.gate = (flags0 >> 8) & 1u;
    v.gprev_a = (flags0 >> 6) & 1u;
    v.gprev_f = (flags0 >> 7) & 1u;
    v.ea.begin(v.gate, v.gprev_a, flags0 & 7u, xa0, c[VCC_ATK_D0A * cn + ci], c[VCC_ATK_TGT_A * cn + ci],
               c[VCC_DEC_D0A * cn + ci], c[VCC_REL_D0A * cn + ci], c[VCC_SUS_A * cn + ci]);
    v.ef.begin(v.gate, v.gprev_f, (flags0 >> 3) & 7u, xf0, c[VCC_ATK_D0F * cn + ci], c[VCC_ATK_TGT_F * cn + ci],
               c[VCC_DEC_D0F * cn + ci], c[VCC_REL_D0F * cn + ci], c[VCC_SUS_F * cn + ci]);
    return ev;
}
__device__ __forceinline__ void voice_envs_store(const VoiceEnvs &v, float *s, uint32_t sn, uint32_t si) {
    s[VCS_ENVA_X * sn + si] = v.ea.x;
    s[VCS_ENVF_X * sn + si] = v.ef.x;
    s[VCS_FLAGS * sn + si] = __uint_as_float(v.ea.mode | v.ef.mode << 3 | (uint32_t)v.gprev_a << 6 |
                                             (uint32_t)v.gprev_f << 7 | (uint32_t)v.gate << 8);
}

// ---- timed notes in the instrument kernels (synth_pipeline.h role_v<SEG>; olfx_timed_notes) ----
// The voice kernels stage every segment's records in LDS up front (VoiceSegs, 8 KB per 64-voice group); eight
// voice slots of that do not fit beside the instrument pipeline's queues.  A V wave reads instead the fixed
// slots of the NEXT segment one segment ahead and keeps them in registers (the packet may be pinned host memory:
// the round trip hides under a segment's samples) ...
__device__ __forceinline__ uint2 seg_event_fetch(const uint2 *evs, uint32_t seg, uint32_t groups, uint32_t group, uint32_t lane) {
    uint2 e = make_uint2(0u, 0u);
    if (lane < kVevCap) e = evs[((size_t)seg * groups + group) * kVevCap + lane];
    return e;
}
// ... and at the segment start scatters them through its 64 slots, exactly as voice_event_of does (a crowded
// segment's overflow run is a dependent second read here: slower, correct).
__device__ __forceinline__ VoiceEv seg_event_take(uint2 e, const uint2 *evs_more, uint2 *slot, uint32_t lane, uint32_t me) {
    slot[lane] = make_uint2(0u, 0u);
    const uint32_t head = __builtin_amdgcn_readfirstlane(e.x);
    if ((head >> 8) & VEV_MORE) {
        const uint32_t cnt = head >> 16, first = __builtin_amdgcn_readfirstlane(e.y);
        e = make_uint2(0u, 0u);
        if (lane < cnt) e = evs_more[first + lane];
    }
    if (e.x >> 8) slot[e.x & 63u] = make_uint2(e.x >> 8, e.y);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const uint2 v = slot[me];
    return VoiceEv{v.x, __uint_as_float(v.y)};
}
// Timed instrument parameters (InstrumentTimed): the record of lane `me` at a segment start from its group's table
// entry, or kNoCoef.  No per-record index: the record is base + the lane's rank among the mask's lower bits.  Dead
// lanes of the last group mirror instrument n - 1: `me` is that lane, so they take its bit and its rank.  A reload
// is under the lane's own bit, and a number outside the section is no record, whatever the packet holds.
__device__ __forceinline__ uint32_t seg_inst_record(uint4 e, uint32_t me, uint32_t count) {
    const uint64_t mask = (uint64_t)e.x | (uint64_t)e.y << 32;
    if (!mask) return kNoCoef;                             // wave-uniform: the common segment start
    const bool has = (mask >> me) & 1ull;
    const uint32_t r = e.z + (uint32_t)__builtin_popcountll(mask & ((1ull << me) - 1ull));
    return has && r < count ? r : kNoCoef;
}
// A segment start from registers, what voice_envs_load does at a launch's start from the stored state: the flags
// word from the live envelope modes, gprev and gate; the segment's gate events on it; both Env::begin.
__device__ __forceinline__ void voice_envs_restart(VoiceEnvs &v, const VoiceEv &ev, const float *c, uint32_t cn, uint32_t ci) {
    uint32_t flags0 = v.ea.mode | v.ef.mode << 3 | (uint32_t)v.gprev_a << 6 | (uint32_t)v.gprev_f << 7 | (uint32_t)v.gate << 8;
    float xa0 = v.ea.x, xf0 = v.ef.x;
    apply_gate_events(ev, flags0, xa0, xf0);
    v.gate = (flags0 >> 8) & 1u;
    v.gprev_a = (flags0 >> 6) & 1u;
    v.gprev_f = (flags0 >> 7) & 1u;
    v.ea.begin(v.gate, v.gprev_a, flags0 & 7u, xa0, c[VCC_ATK_D0A * cn + ci], c[VCC_ATK_TGT_A * cn + ci],
               c[VCC_DEC_D0A * cn + ci], c[VCC_REL_D0A * cn + ci], c[VCC_SUS_A * cn + ci]);
    v.ef.begin(v.gate, v.gprev_f, (flags0 >> 3) & 7u, xf0, c[VCC_ATK_D0F * cn + ci], c[VCC_ATK_TGT_F * cn + ci],
               c[VCC_DEC_D0F * cn + ci], c[VCC_REL_D0F * cn + ci], c[VCC_SUS_F * cn + ci]);
}

// samples per hand-off between the roles: 8 (34 barrier steps per 256-frame block, pipeline fill
// 2 of them) measured 2 % faster than 16 (18 steps) for the Svf voice and equal for the Moog
// voice; 32 halves the workgroups per CU (96 KB of LDS each) and is 1.7x slower
constexpr int kVcChunk = 8;
static_assert(kVcChunk == 8 && kVoiceChunk == 8, "SegCursor<true>::len; the host's chunk count");

// Runs f(j) for the m samples of a chunk: unrolled when the chunk is full, so the off-recurrence
// work of neighbouring samples interleaves (ILP for a wave that is alone on its SIMD).
template <class F>
__device__ __forceinline__ void for_chunk(uint32_t m, F &&f) {
    if (m == (uint32_t)kVcChunk) {
#pragma unroll
        for (uint32_t j = 0; j < (uint32_t)kVcChunk; ++j) f(j);
    } else {
        for (uint32_t j = 0; j < m; ++j) f(j);
    }
}

// ---------------------------------------------------------------------------------------------
// The roles of the Svf voice's four-wave pipeline that do not depend on the sound source (the
// pipeline itself: voice.hip voice_block_v5).  A workgroup is 64 voices; at step k ENV makes chunk k,
// the source role and FREQ chunk k-1, FILT chunk k-2; one __syncthreads() per step in every role.
// ---------------------------------------------------------------------------------------------
typedef float2 VoiceEnvQ[3][kVcChunk][64];      // ENV -> FREQ (fc_in), FILT (amp): three chunks live
typedef float2 VoiceFreqQ[2][kVcChunk][64];     // FREQ -> FILT: (-damp, fq)

// A lane's place in the block: its voice i (dead lanes of the last workgroup mirror voice n-1
// exactly -- same state, same coefficients, same events -- so their stores write the values voice
// n-1's lane writes), me = the voice within the group.
struct VoiceLane {
    uint32_t n, lane, i, me, nf, nsteps;
    __device__ __forceinline__ uint32_t len(uint32_t k) const {          // frames of chunk k (the last may be short)
        const uint32_t f0 = k * kVcChunk;
        return nf - f0 < (uint32_t)kVcChunk ? nf - f0 : (uint32_t)kVcChunk;
    }
};
__device__ __forceinline__ VoiceLane voice_lane(const VoiceArgs &a) {
    VoiceLane v;
    v.n = a.n;
    v.lane = threadIdx.x & 63;
    const uint32_t i0 = blockIdx.x * 64 + v.lane;
    v.i = i0 < v.n ? i0 : v.n - 1;
    v.me = v.i - blockIdx.x * 64;
    v.nf = a.n_frames;
    v.nsteps = (v.nf + kVcChunk - 1) / kVcChunk + 2;
    return v;
}
// ... of a segmented launch: its chunks are the segments' (VoiceArgs::n_chunks)
__device__ __forceinline__ VoiceLane voice_lane_seg(const VoiceArgs &a) {
    VoiceLane v = voice_lane(a);
    v.nsteps = a.n_chunks + 2;
    return v;
}

// ---- ENV (SynthVoice.h:42,46-47): the amp and filter Adsr, the cutoff sum ----
// SEG (timed events): `evslot` is unused; the wave stages every segment's records into *sg, and at each
// segment's first chunk applies that segment's gate events to the live flag bits and levels and runs
// Env::begin again with the carried gprev -- what the next launch does from the stored state.
template <bool SEG = false>
__device__ __forceinline__ void voice_role_env(const VoiceArgs &a, const VoiceLane &v, VoiceEnvQ &eq, uint2 *evslot,
                                               VoiceSegs *sg = nullptr) {
    const uint32_t n = v.n, lane = v.lane, i = v.i, me = v.me, nsteps = v.nsteps;
    const float *c = a.coef;
    float *s = a.state;
    // the block's gate events first (NoteOn / GateOn / NoteOff / GateOff); the state loads are
    // issued before the event read, so their latency hides under its host-link round trip
    uint32_t flags0 = __float_as_uint(s[VCS_FLAGS * n + i]);
    float xa0 = s[VCS_ENVA_X * n + i], xf0 = s[VCS_ENVF_X * n + i];
    if constexpr (SEG) {
        voice_events_stage(a, *sg, lane, blockIdx.x);
    } else {
        const VoiceEv ev = voice_event(a, evslot, lane, me);
        apply_gate_events(ev, flags0, xa0, xf0);
    }
    bool gate = (flags0 >> 8) & 1u;
    bool gprev_a = (flags0 >> 6) & 1u, gprev_f = (flags0 >> 7) & 1u;
    // (SEG: loop-carried -- a segment with VEV_COEF replaces them)
    float amp_amt = c[VCC_AMP_AMT * n + i], fc_max = c[VCC_FC_MAX * n + i];
    float amp_half = 0.5f * amp_amt;             // FILT's Low() halving folded in (exact scaling)
    float cutoff = c[VCC_CUTOFF * n + i], fenv_amt = c[VCC_FENV_AMT * n + i];
    Env ea, ef;
    // (SEG: the envelope coefficients stay in registers for the segment starts)
    [[maybe_unused]] float ca[5], cf[5];
    if constexpr (SEG) {
        ca[0] = c[VCC_ATK_D0A * n + i]; ca[1] = c[VCC_ATK_TGT_A * n + i]; ca[2] = c[VCC_DEC_D0A * n + i];
        ca[3] = c[VCC_REL_D0A * n + i]; ca[4] = c[VCC_SUS_A * n + i];
        cf[0] = c[VCC_ATK_D0F * n + i]; cf[1] = c[VCC_ATK_TGT_F * n + i]; cf[2] = c[VCC_DEC_D0F * n + i];
        cf[3] = c[VCC_REL_D0F * n + i]; cf[4] = c[VCC_SUS_F * n + i];
    } else {
        ea.begin(gate, gprev_a, flags0 & 7u, xa0, c[VCC_ATK_D0A * n + i],
                 c[VCC_ATK_TGT_A * n + i], c[VCC_DEC_D0A * n + i], c[VCC_REL_D0A * n + i], c[VCC_SUS_A * n + i]);
        ef.begin(gate, gprev_f, (flags0 >> 3) & 7u, xf0, c[VCC_ATK_D0F * n + i],
                 c[VCC_ATK_TGT_F * n + i], c[VCC_DEC_D0F * n + i], c[VCC_REL_D0F * n + i], c[VCC_SUS_F * n + i]);
    }
    SegCursor<SEG> cu(sg, a.n_seg);
    for (uint32_t k = 0; k < nsteps; ++k) {
        if (k + 2 < nsteps) {
            if constexpr (SEG) {
                if (cu.first) {
                    if (k) {                     // the live state as the flags word and levels a launch would load
                        flags0 = ea.mode | ef.mode << 3 | (uint32_t)gprev_a << 6 | (uint32_t)gprev_f << 7 | (uint32_t)gate << 8;
                        xa0 = ea.x;
                        xf0 = ef.x;
                    }
                    const VoiceEv sev = seg_event(*sg, cu.seg, me);
                    if (const uint32_t r = seg_coef_record(a, *sg, cu.seg, sev, n, me); r != kNoCoef) {
                        // timed parameters: the segment's coefficients first, then what a launch's start does
                        ca[0] = seg_coef(a, r, VCC_ATK_D0A); ca[1] = seg_coef(a, r, VCC_ATK_TGT_A); ca[2] = seg_coef(a, r, VCC_DEC_D0A);
                        ca[3] = seg_coef(a, r, VCC_REL_D0A); ca[4] = seg_coef(a, r, VCC_SUS_A);
                        cf[0] = seg_coef(a, r, VCC_ATK_D0F); cf[1] = seg_coef(a, r, VCC_ATK_TGT_F); cf[2] = seg_coef(a, r, VCC_DEC_D0F);
                        cf[3] = seg_coef(a, r, VCC_REL_D0F); cf[4] = seg_coef(a, r, VCC_SUS_F);
                        amp_amt = seg_coef(a, r, VCC_AMP_AMT);
                        cutoff = seg_coef(a, r, VCC_CUTOFF);
                        fenv_amt = seg_coef(a, r, VCC_FENV_AMT);
                        fc_max = seg_coef(a, r, VCC_FC_MAX);
                        amp_half = 0.5f * amp_amt;
                    }
                    apply_gate_events(sev, flags0, xa0, xf0);
                    gate = (flags0 >> 8) & 1u;
                    gprev_a = (flags0 >> 6) & 1u;
                    gprev_f = (flags0 >> 7) & 1u;
                    ea.begin(gate, gprev_a, flags0 & 7u, xa0, ca[0], ca[1], ca[2], ca[3], ca[4]);
                    ef.begin(gate, gprev_f, (flags0 >> 3) & 7u, xf0, cf[0], cf[1], cf[2], cf[3], cf[4]);
                }
            }
            const uint32_t m = [&] { if constexpr (SEG) return cu.len(); else return v.len(k); }();
            float2 *qo = &eq[k % 3][0][lane];
            if (m == (uint32_t)kVcChunk) {
                // Full chunk: the envelopes run speculatively with no per-sample segment test
                // (a branch on a lane vote per sample serialised the chunk); if any lane's
                // segment ended inside the chunk -- a few chunks per note -- the chunk is
                // redone sample by sample from its start with the exact segment machine.
                const float xa0 = ea.x, xf0 = ef.x;
                bool ended = false;
                // both envelopes' Env::step_spec in packed operations (the pair lives in a
                // register pair for the chunk), then (x_a amp_amt, x_f 20000)
                f2 X = {ea.x, ef.x};
                const f2 D0 = {ea.d0, ef.d0}, T = {ea.tgt, ef.tgt}, AMT = {amp_half, 20000.0f};
#pragma unroll
                for (uint32_t j = 0; j < (uint32_t)kVcChunk; ++j) {
                    X = X + D0 * (T - X);
                    const f2 m = X * AMT;
                    qo[j * 64] = make_float2(m.x, svf_fc(__builtin_fmaf(m.y, fenv_amt, cutoff), fc_max));
                }
                // inside a segment the envelope is monotone toward a target beyond its bound
                // (x += d0 (tgt - x) with tgt - x of one sign: each IEEE step keeps the
                // direction), so it crossed the bound inside the chunk iff it ends past it
                ended = X.x > ea.hi || X.x < ea.lo || X.y > ef.hi || X.y < ef.lo;
                ea.x = X.x;
                ef.x = X.y;
                if (__builtin_amdgcn_ballot_w64(ended)) {
                    ea.x = xa0;
                    ef.x = xf0;
                    for (uint32_t j = 0; j < (uint32_t)kVcChunk; ++j) {
                        const float amp = ea.step() * amp_half;
                        const float fe = ef.step();
                        qo[j * 64] = make_float2(amp, svf_fc(__builtin_fmaf(fe * 20000.0f, fenv_amt, cutoff), fc_max));
                    }
                }
            } else {
                for_chunk(m, [&](uint32_t j) {
                    const float amp = ea.step() * amp_half;
                    const float fe = ef.step();
                    qo[j * 64] = make_float2(amp, svf_fc(__builtin_fmaf(fe * 20000.0f, fenv_amt, cutoff), fc_max));
                });
            }
            cu.next();
        }
        __syncthreads();
    }
    s[VCS_ENVA_X * n + i] = ea.x;
    s[VCS_ENVF_X * n + i] = ef.x;
    s[VCS_FLAGS * n + i] = __uint_as_float(ea.mode | ef.mode << 3 | (uint32_t)gprev_a << 6 |
                                           (uint32_t)gprev_f << 7 | (uint32_t)gate << 8);
}

// ---- FREQ: Svf::SetFreq (its divisions use the hardware reciprocal, as in v4) ----
template <bool SEG = false>
__device__ __forceinline__ void voice_role_freq(const VoiceArgs &a, const VoiceLane &v, const VoiceEnvQ &eq, VoiceFreqQ &fdq,
                                                const VoiceSegs *sg = nullptr) {
    const uint32_t n = v.n, lane = v.lane, i = v.i, nsteps = v.nsteps;
    const float *c = a.coef;
    float damp_res = c[VCC_DAMP_RES * n + i];    // (SEG: a segment with VEV_COEF replaces it)
    const float inv_2sr = 1.0f / (c[VCC_SR * n + i] * 2.0f);
    SegCursor<SEG> cu(sg, a.n_seg);
    for (uint32_t k = 0; k < nsteps; ++k) {
        if (k >= 1 && k + 1 < nsteps) {
            if constexpr (SEG) {
                if (cu.first && a.tc)            // timed parameters: this segment's damping
                    if (const uint32_t r = seg_coef_record(a, *sg, cu.seg, seg_event(*sg, cu.seg, v.me), n, v.me); r != kNoCoef)
                        damp_res = seg_coef(a, r, VCC_DAMP_RES);
            }
            const uint32_t m = [&] { if constexpr (SEG) return cu.len(); else return v.len(k - 1); }();
            const float2 *qi = &eq[(k - 1) % 3][0][lane];
            float2 *qo = &fdq[(k - 1) & 1][0][lane];
            // hands FILT (-damp, fq): its notch src - damp band is src + (-damp) band, exactly
            if (m == (uint32_t)kVcChunk) {
                // no recurrence here: two samples per packed operation, the chunk's four pairs
                // stage by stage (a packed result read by the next instruction costs a wait
                // state; four independent pairs fill them)
                constexpr int P = kVcChunk / 2;
                f2 x[P], x2[P], pp[P], fq[P], sq[P];
#pragma unroll
                for (int q = 0; q < P; ++q) {
                    const float c0 = qi[(2 * q) * 64].y;          // clamped by ENV (svf_fc)
                    const float c1 = qi[(2 * q + 1) * 64].y;
                    const f2 fcn = (f2){c0, c1} * inv_2sr;
                    const f2 arg = {__builtin_fminf(fcn.x, 0.25f), __builtin_fminf(fcn.y, 0.25f)};
                    x[q] = 3.1415927410125732f * arg;
                }
#pragma unroll
                for (int q = 0; q < P; ++q) x2[q] = x[q] * x[q];
#pragma unroll
                for (int q = 0; q < P; ++q) pp[q] = __builtin_elementwise_fma((f2)2.7557319e-6f, x2[q], (f2)-1.9841270e-4f);
#pragma unroll
                for (int q = 0; q < P; ++q) pp[q] = __builtin_elementwise_fma(pp[q], x2[q], (f2)8.3333333e-3f);
#pragma unroll
                for (int q = 0; q < P; ++q) pp[q] = __builtin_elementwise_fma(pp[q], x2[q], (f2)-1.6666667e-1f);
#pragma unroll
                for (int q = 0; q < P; ++q) x2[q] = x[q] * x2[q];
#pragma unroll
                for (int q = 0; q < P; ++q) sq[q] = __builtin_elementwise_fma(x2[q], pp[q], x[q]);   // sin(x); fq = 2 sin
#pragma unroll
                for (int q = 0; q < P; ++q) {
                    const f2 rq = {__builtin_amdgcn_rcpf(sq[q].x), __builtin_amdgcn_rcpf(sq[q].y)};
                    // 2 / fq - fq / 2 = 1 / s - s: one subtraction (and the reciprocal of s, not of 2 s)
                    const f2 lim = rq - sq[q];
                    fq[q] = sq[q] + sq[q];
                    qo[(2 * q) * 64] = make_float2(neg_damp(damp_res, lim.x), fq[q].x);
                    qo[(2 * q + 1) * 64] = make_float2(neg_damp(damp_res, lim.y), fq[q].y);
                }
            } else {
                for (uint32_t j = 0; j < m; ++j) {
                    const float fc = qi[j * 64].y;
                    const float fcn = fc * inv_2sr;
                    const float arg = __builtin_fminf(fcn, 0.25f);
                    const float s1 = sin_quarter(3.1415927410125732f * arg), fq = s1 + s1;
                    const float lim = __builtin_amdgcn_rcpf(s1) - s1;
                    qo[j * 64] = make_float2(neg_damp(damp_res, lim), fq);
                }
            }
            cu.next();
        }
        __syncthreads();
    }
}

// ---- FILT: Svf::Process; Low() = the average of the two passes' low outputs; * amp ----
// src_of(c) = this lane's first source sample of chunk c; the chunk's samples are STRIDE floats apart.
template <uint32_t STRIDE, bool SEG = false, class SrcOf>
__device__ __forceinline__ void voice_role_filt(const VoiceArgs &a, const VoiceLane &v, const VoiceEnvQ &eq,
                                                const VoiceFreqQ &fdq, SrcOf &&src_of, const VoiceSegs *sg = nullptr) {
    const uint32_t n = v.n, lane = v.lane, i = v.i, nsteps = v.nsteps;
    const float *c = a.coef;
    float *s = a.state;
    float drive = c[VCC_DRIVE * n + i];          // (SEG: a segment with VEV_COEF replaces it)
    float low = s[VCS_LOW * n + i], band = s[VCS_BAND * n + i];
    SegCursor<SEG> cu(sg, a.n_seg);
    for (uint32_t k = 0; k < nsteps; ++k) {
        if (k >= 2) {
            if constexpr (SEG) {
                if (cu.first && a.tc)            // timed parameters: this segment's drive
                    if (const uint32_t r = seg_coef_record(a, *sg, cu.seg, seg_event(*sg, cu.seg, v.me), n, v.me); r != kNoCoef)
                        drive = seg_coef(a, r, VCC_DRIVE);
            }
            const uint32_t f0 = SEG ? (uint32_t)cu.f0 : (k - 2) * kVcChunk;
            const uint32_t m = [&] { if constexpr (SEG) return cu.len(); else return v.len(k - 2); }();
            // the chunk's output rows through a buffer resource based at row f0: the row offset
            // j n 4 is a scalar (soffset), so a store costs no vector address arithmetic
            const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(
                a.out + (size_t)f0 * n, (short)0, (int)((uint32_t)kVcChunk * n * 4u), 0x00020000);
            const float *qs = src_of(k - 2);
            const float2 *qa = &eq[(k - 2) % 3][0][lane];
            const float2 *qf = &fdq[k & 1][0][lane];           // chunk k-2: (k-2) & 1 == k & 1
            for_chunk(m, [&](uint32_t j) {
                const float2 fd = qf[j * 64];
                const float2 sa = make_float2(qs[j * STRIDE], qa[j * 64].x);
                // (packing this serial recurrence's paired products cost as many register
                // moves as it saved operations: scalar)
                const float src = sa.x, ndamp = fd.x, fq = fd.y;     // FREQ hands over -damp
                // contracted except the notch (see Contraction in voice.hip)
                float notch = src + ndamp * band;
                low = __builtin_fmaf(fq, band, low);
                float high = notch - low;
                band = __builtin_fmaf(-((drive * band) * band), band, __builtin_fmaf(fq, high, band));
                const float low1 = low;
                notch = src + ndamp * band;
                low = __builtin_fmaf(fq, band, low);
                high = notch - low;
                band = __builtin_fmaf(-((drive * band) * band), band, __builtin_fmaf(fq, high, band));
                // Low() = 0.5 low1 + 0.5 low2, times amp: (low1 + low2) (amp / 2), the same rounding (halvings exact)
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint((low1 + low) * sa.y), ro, i * 4u, j * n * 4u, 0);
            });
            cu.next();
        }
        __syncthreads();
    }
    s[VCS_LOW * n + i] = low;
    s[VCS_BAND * n + i] = band;
}

// Roles by SIMD.  The roles' VALU loads differ (per 8-sample chunk FILT ~218, OSC ~190, FREQ
// ~159, ENV ~111 instructions) and the two co-resident workgroups of a CU put wave w on the
// same SIMD, so role = wave stacks two FILTs on one SIMD.  Each wave reads its SIMD (HW_ID
// bits 5:4) and slot (bits 3:0); a workgroup whose wave 0 sits in an odd slot takes the roles in
// mirrored SIMD order, pairing ENV with FILT and the source role with FREQ on every SIMD.  Waves
// that do not sit on four distinct SIMDs keep role = wave (any assignment is correct; this one only
// balances).  hw_simd: 5 words of LDS ([4]: wave 0's slot parity).  Contains a __syncthreads().
__device__ __forceinline__ uint32_t voice_role_of_wave(uint32_t *hw_simd, uint32_t lane, uint32_t wave) {
    {
        const uint32_t hw = __builtin_amdgcn_s_getreg(4 | (0 << 6) | (31 << 11));   // HW_REG_HW_ID
        if (lane == 0) {
            hw_simd[wave] = (hw >> 4) & 3u;
            if (wave == 0) hw_simd[4] = hw & 1u;
        }
    }
    __syncthreads();
    uint32_t role = wave;
    {
        const uint32_t m = (1u << hw_simd[0]) | (1u << hw_simd[1]) | (1u << hw_simd[2]) | (1u << hw_simd[3]);
        const uint32_t sm = hw_simd[wave];
        if (m == 15u) role = hw_simd[4] ? 3u - sm : sm;
        role = __builtin_amdgcn_readfirstlane(role);
    }
    return role;
}

}  // namespace olfx
