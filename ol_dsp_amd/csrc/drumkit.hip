// ol_dsp_amd/csrc/drumkit.hip -- the reference's drum machine (a VoiceMap of sample voices, summed, into the
// effect rack) in one launch, gfx950, wave64: drumkit_block_v1, OLFX_KIND_DRUMKIT.
//
// Per frame and kit, every operation in fp32:
//   v[p]  = voice slot p: SynthVoice(SampleSoundSource<1>(Sample), SvfFilter) -- sampler_block_v1's arithmetic,
//           operation for operation: Sample::Process as sampler.hip restates it, then svf_voice.h's ENV, FREQ and
//           FILT around that frame (svf_voice_tick_src; Port and Oscillator are not run).  Each slot has its own
//           coefficients and its own Sample;
//   frame = 0.0f; frame += v[o[0]]; frame += v[o[1]]; ...      VoiceMap::Process (VoiceMap.h:64-73): the kit's
//           mapped voices by ascending note, the order the host derived from the map (DKC_ORDER: four bits per
//           voice slot, kDkOrderEnd ends the list; an empty map sums nothing).  A voice that sits at no note is
//           not summed but still ticks, as in the engines this kernel replaces;
//   rack on (frame, 0.0f) at the kit's topology, exactly as synth_svf_block_v1 (synth.hip): 1 = the firmware
//           callback, 0 = FxRack<2>::Process with its master volume.
// which is what sampler_block_v1 + voice_mix + fxrack_block_v3 compute in three launches, bit for bit.
//
// The pipeline is synth.hip's: a workgroup owns 64 kits and runs seven single-role waves over LDS queues of
// 16-frame chunks with the progress counters of lds_flags.h -- V0..V3 (voice slots w and w + 4, lane = kit, both
// voices' state in registers for the block), D0 / D1 (fr::delay_stage_from over 32 kits x 2 channel lanes, its
// input callback forming the ordered sum from queue V), F (the stub reverb's balance mix, the filter, the
// stores).  Counters, waits and the no-deadlock argument are synth.hip's, unchanged: the Sample changes what V
// computes, not what it waits for.  The spins are bounded (kDkSpinMax).
//
// The fetch.  Lane = kit means lane = voice: left alone, every load would be a 64-row gather of 4 B, which the
// sampler measured 1.74x slower than wide fetches ("Sample voice").  So per chunk and voice
// slot the common case is cooperative: 16 load instructions, instruction j covering kits 4 j .. 4 j + 3 x 16
// consecutive frames -- lane l loads frame l & 15 of kit 4 j + (l >> 4), the kit's byte offset fetched from its
// lane with ds_bpermute, 64 contiguous bytes per voice -- all 16 in flight at once, then transposed through the
// wave's own padded LDS tile [16][65]: the writes of a 32-lane group fall on 17 banks two deep (free for
// ds_write_b32), the reads (one row, 64 consecutive columns) on distinct banks.  The loads are issued before the
// wave waits for its queue-V buffer, so their latency hides under the previous chunk's consumers.
// That serves a voice whose chunk is one run: playing, and neither the sample's end nor its loop turn inside
// the chunk.  Voices that read nothing (paused, unassigned, exhausted) feed 0.0f.  The others -- a turn or an end
// inside the chunk, loops shorter than it -- walk Sample::Process's rule frame by frame into byte offsets and
// gather them, 16 loads in flight.  -DOLFX_DRUMKIT_PER_LANE sends every playing voice down that path (the
// A/B variant, tools/synth_ab.py).  Measured ("Drum kit"): a mixed result -- the cooperative
// fetch is 4 - 5 us per block faster at P = 1 and P = 8 and 1.6 us slower at P = 4 (16,384 kits); the loads are
// issued ahead of the wave's wait either way, so neither fetch is on the critical path as the sampler's was.
//
// Bounds.  Every bank load goes through a buffer resource over the bank allocation with the offset in the
// range-checked vector operand; base / len / loop points are clamped to what the host laid out (bank_plan:
// kSmAlign-aligned starts, a padded tail), the cursor to len, and lanes past the chunk's frames do not load --
// as sampler.hip.  No load depends on unclamped words.  The sum order's nibbles are compared with the kit's
// voice count before they index queue V.
// LDS: 79,680 B per workgroup at P = 4, 112,448 B at 8 (synth.hip's plus the four tiles).
#include "rack_delay_stage.h"
#include "svf_voice.h"
#include "lds_flags.h"

namespace olfx {

namespace {
constexpr int kDkVWaves = 4;                              // voice waves
constexpr int kDkThreads = (kDkVWaves + 3) * 64;          // + D0, D1, F
constexpr int kDkChunk = fr::kChunk;
constexpr int kDkQ = kDkChunk * 64;                       // floats of one (voice, chunk) or one queue-A buffer
constexpr int kDkDepthV = 2, kDkDepthA = 2;
constexpr int kDkFlags = 16;
constexpr uint32_t kDkTileStride = 65;                    // floats per tile row: row + column = the bank
constexpr uint32_t kDkTile = kDkChunk * kDkTileStride;    // a V wave's transpose tile
constexpr uint32_t kDkSpinMax = 1u << 22;                 // x s_sleep(1): ~0.1 s, five orders above any real wait
constexpr uint32_t kDkNone = 0xFFFFFFFFu;                 // per-frame path: this frame reads nothing
enum { F_V0 = 0, F_R0 = kDkVWaves, F_R1, F_D0, F_D1, F_FIN };
constexpr size_t dk_lds_floats(uint32_t voices) {
    return 2 * (size_t)fr::kRegion + (size_t)kDkDepthV * voices * kDkQ + (size_t)kDkDepthA * kDkQ + kDkFlags +
           (size_t)kDkVWaves * 64 * 2 + (size_t)kDkVWaves * kDkTile;
}
static_assert(dk_lds_floats(kDkMaxVoices) * 4 < 160 * 1024, "LDS budget");
static_assert((2 * fr::kRegion) % 4 == 0, "16-byte aligned queues");
static_assert(kDkChunk == 16 && kSmAlign >= (uint32_t)kDkChunk, "a cooperative load is 4 kits x 16 frames, inside the bank's padding");

template <class Cond>
__device__ __forceinline__ void dk_wait(Cond &&cond) {
    for (uint32_t t = 0; !cond() && t < kDkSpinMax; ++t) __builtin_amdgcn_s_sleep(1);
}

// one dword at byte offset `off` of the bank (range-checked against the resource: 0 outside)
__device__ __forceinline__ float dk_bank_load(__amdgpu_buffer_rsrc_t bank, uint32_t off) {
    return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(bank, off, 0, 0));
}

// One sample voice of this lane: the Svf voice's envelopes and filter with its own coefficients, and its Sample.
struct DkVoice {
    Env ea, ef;
    float low, band;
    bool gate, gprev_a, gprev_f;
    SvfVoiceCoef kc;
    uint32_t base, len, ls, le, limit, pos, mg;
    bool loop, playing;
};
}  // namespace

__global__ __launch_bounds__(kDkThreads) void drumkit_block_v1(DrumkitArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const uint32_t tid = threadIdx.x;
    const uint32_t wib = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const uint32_t lane = tid & 63u;
    const uint32_t n = a.n, nf = a.n_frames, P = a.voices;
    const uint32_t nchunks = (nf + kDkChunk - 1) / kDkChunk;
    const uint32_t g = blockIdx.x;                         // the group: kits 64 g ..
    float *vq = lds + 2 * fr::kRegion;                     // voices -> delay   [kDkDepthV][P][16][64]
    float *aq = vq + (size_t)kDkDepthV * P * kDkQ;         // delay -> filter   [kDkDepthA][16][64]
    uint32_t *flags = (uint32_t *)(aq + kDkDepthA * kDkQ);
    uint2 *evslots = (uint2 *)(flags + kDkFlags);          // [kDkVWaves][64]
    float *tiles = (float *)(evslots + kDkVWaves * 64);    // [kDkVWaves][16][65]
    if (tid < kDkFlags) flags[tid] = 0;
    __syncthreads();                                       // the only barrier
    const bool d1_on = g * 64u + 32u < n;                  // the group's upper half holds a kit
    const uint32_t nvw = min(P, (uint32_t)kDkVWaves);

    if (wib < (uint32_t)kDkVWaves) {
        // ---------------- V: voice slots wib and wib + 4, lane = kit ----------------
        if (wib >= nvw) return;
        const uint32_t i_raw = g * 64u + lane;
        // lanes past n mirror kit n - 1 exactly (same state, coefficients, Sample and events), so their
        // stores write the values its own lane writes
        const uint32_t i = i_raw < n ? i_raw : n - 1;
        const uint32_t me = i - g * 64u;
        const uint32_t sn = P * a.npad;                    // voice slots: the stride of every voice plane
        const float *c = a.vc_coef;
        float *s = a.vc_state;
        const uint32_t *sm = a.smp;
        uint2 *evslot = evslots + wib * 64u;
        float *tile = tiles + wib * kDkTile;
        const bool two = wib + (uint32_t)kDkVWaves < P;
        const __amdgpu_buffer_rsrc_t bank =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.bank), (short)0, (int)a.bank_bytes, 0x00020000);
        // a Sample clamped to the allocation: base + len + the fetch width <= the bank
        const uint32_t bank_f = a.bank_bytes >> 2;
        const uint32_t room = bank_f > kSmAlign ? bank_f - kSmAlign : 0u;

        auto load = [&](DkVoice &v, uint32_t p) {
            const uint32_t si = p * a.npad + i;
            uint32_t flags0 = __float_as_uint(s[VCS_FLAGS * sn + si]);
            float xa0 = s[VCS_ENVA_X * sn + si], xf0 = s[VCS_ENVF_X * sn + si];
            const VoiceEv ev = voice_event_of(a.ev, a.ev_more, evslot, lane, me, p * (a.npad >> 6) + g);
            apply_gate_events(ev, flags0, xa0, xf0);
            v.gate = (flags0 >> 8) & 1u;
            v.gprev_a = (flags0 >> 6) & 1u;
            v.gprev_f = (flags0 >> 7) & 1u;
            v.ea.begin(v.gate, v.gprev_a, flags0 & 7u, xa0, c[VCC_ATK_D0A * sn + si], c[VCC_ATK_TGT_A * sn + si],
                       c[VCC_DEC_D0A * sn + si], c[VCC_REL_D0A * sn + si], c[VCC_SUS_A * sn + si]);
            v.ef.begin(v.gate, v.gprev_f, (flags0 >> 3) & 7u, xf0, c[VCC_ATK_D0F * sn + si], c[VCC_ATK_TGT_F * sn + si],
                       c[VCC_DEC_D0F * sn + si], c[VCC_REL_D0F * sn + si], c[VCC_SUS_F * sn + si]);
            v.low = s[VCS_LOW * sn + si];
            v.band = s[VCS_BAND * sn + si];
            // the slot's own coefficients, as voice_role_env / voice_role_freq form them (Port and Oscillator unused)
            v.kc = SvfVoiceCoef{0.5f * c[VCC_AMP_AMT * sn + si], 0.0f, 0.0f, c[VCC_CUTOFF * sn + si],
                                c[VCC_FENV_AMT * sn + si], c[VCC_FC_MAX * sn + si], c[VCC_DRIVE * sn + si],
                                c[VCC_DAMP_RES * sn + si], 1.0f / (c[VCC_SR * sn + si] * 2.0f)};
            // the slot's Sample (sampler.hip's SRC role): clamps, freshness, then the block's events
            v.base = min(sm[SMC_BASE * sn + si], room);
            v.len = min(sm[SMC_LEN * sn + si], room - v.base);
            v.ls = min(sm[SMC_LS * sn + si], v.len);
            const uint32_t le0 = sm[SMC_LE * sn + si];
            v.le = le0 < v.len ? le0 : 0u;
            v.mg = sm[SMC_MODE * sn + si];
            v.loop = v.mg & 1u;
            v.pos = __float_as_uint(s[VCS_SM_POS * sn + si]);
            uint32_t fl = __float_as_uint(s[VCS_SM_FLAGS * sn + si]);
            if ((fl >> 1) != (v.mg >> 1)) {                // another Sample object since the last block: fresh
                v.pos = 0u;
                fl = 0u;
            }
            v.playing = fl & 1u;
            v.pos = min(v.pos, v.len);
            // any NoteOn is Seek(0), the last gate call Play() or Pause() (SampleSoundSource.h:21-26); the pitch
            // is stored (SynthVoice::freq_)
            if (ev.op & VEV_SEEK) v.pos = 0u;
            if (ev.op & VEV_GATE_SET) v.playing = (ev.op & VEV_GATE_ON) != 0u;
            if (ev.op & VEV_FREQ) s[VCS_FREQ * sn + si] = ev.freq;
            // reads without a turn stop before `limit`: the end, or loop_end (the turn follows the read that
            // makes current_frame_ > loop_end_)
            v.limit = (v.loop && v.le) ? v.le : v.len;
        };
        auto store = [&](const DkVoice &v, uint32_t p) {
            const uint32_t si = p * a.npad + i;
            s[VCS_ENVA_X * sn + si] = v.ea.x;
            s[VCS_ENVF_X * sn + si] = v.ef.x;
            s[VCS_FLAGS * sn + si] = __uint_as_float(v.ea.mode | v.ef.mode << 3 | (uint32_t)v.gprev_a << 6 |
                                                     (uint32_t)v.gprev_f << 7 | (uint32_t)v.gate << 8);
            s[VCS_LOW * sn + si] = v.low;
            s[VCS_BAND * sn + si] = v.band;
            s[VCS_SM_POS * sn + si] = __uint_as_float(v.pos);
            s[VCS_SM_FLAGS * sn + si] = __uint_as_float((v.mg & ~1u) | (v.playing ? 1u : 0u));
        };
        // Sample::Process over a chunk of m frames (m is wave-uniform): x[k] = the frame the voice's filter is fed
        auto fetch = [&](DkVoice &v, uint32_t m, float (&x)[kDkChunk]) {
            const bool silent = !v.playing || (v.pos >= v.len && (!v.loop || v.ls >= v.len));
#ifdef OLFX_DRUMKIT_PER_LANE
            const bool plain = false;                      // the variant build: lane = voice gathers only
#else
            const bool plain = v.playing && v.pos + m <= v.limit;
#endif
            const bool slow = !plain && !silent;
#pragma unroll
            for (int k = 0; k < kDkChunk; ++k) x[k] = 0.0f;
            if (__builtin_amdgcn_ballot_w64(plain)) {
                // instruction j: kits 4 j .. 4 j + 3, 16 consecutive frames each; kits that are not plain
                // re-read the bank's first line and are not used
                const uint32_t boff = plain ? (v.base + v.pos) * 4u : 0u;
                const uint32_t fl = lane & 15u, gl = lane >> 4;
                float y[kDkChunk];
#pragma unroll
                for (uint32_t j = 0; j < (uint32_t)kDkChunk; ++j) {
                    const uint32_t off = (uint32_t)__builtin_amdgcn_ds_bpermute((int)((4u * j + gl) << 2), (int)boff);
                    y[j] = fl < m ? dk_bank_load(bank, off + fl * 4u) : 0.0f;
                }
#pragma unroll
                for (uint32_t j = 0; j < (uint32_t)kDkChunk; ++j) tile[fl * kDkTileStride + 4u * j + gl] = y[j];
                // one wave writes and reads its tile: LDS operations of a wave complete in order; the fences keep
                // the compiler from moving the reads above the other lanes' writes
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
                for (uint32_t k = 0; k < (uint32_t)kDkChunk; ++k) {
                    const float t = tile[k * kDkTileStride + lane];
                    x[k] = plain ? t : 0.0f;
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
            if (plain) v.pos += m;
            if (__builtin_amdgcn_ballot_w64(slow)) {
                // Sample::Process frame by frame: the byte offset each frame reads (or none), then the gather
                uint32_t o[kDkChunk];
#pragma unroll
                for (uint32_t k = 0; k < (uint32_t)kDkChunk; ++k) {
                    const bool on = slow && k < m;
                    const bool rd = on && v.pos < v.len;
                    o[k] = rd ? (v.base + v.pos) * 4u : kDkNone;
                    v.pos += rd ? 1u : 0u;
                    if (on && v.loop && (!rd || (v.le && v.pos > v.le))) v.pos = v.ls;
                }
#pragma unroll
                for (uint32_t k = 0; k < (uint32_t)kDkChunk; ++k) {
                    const float yk = dk_bank_load(bank, o[k] == kDkNone ? 0u : o[k]);
                    x[k] = o[k] == kDkNone ? x[k] : yk;
                }
            }
        };
        // the voice's samples of a chunk of m frames -> q[k * 64] (its column of queue V)
        auto run = [&](DkVoice &v, const float (&x)[kDkChunk], float *q, uint32_t m) {
            if (m == (uint32_t)kDkChunk) {
#pragma unroll 4
                for (uint32_t k = 0; k < (uint32_t)kDkChunk; ++k)
                    q[k * 64u] = svf_voice_tick_src(v.ea, v.ef, v.low, v.band, x[k], v.kc);
            } else {
#pragma unroll
                for (uint32_t k = 0; k < (uint32_t)kDkChunk; ++k)
                    if (k < m) q[k * 64u] = svf_voice_tick_src(v.ea, v.ef, v.low, v.band, x[k], v.kc);
            }
        };

        DkVoice va, vb;
        load(va, wib);
        if (two) load(vb, wib + kDkVWaves);
        else vb = va;                                      // (never run, never stored)
        for (uint32_t ck = 0; ck < nchunks; ++ck) {
            const uint32_t m = min((uint32_t)kDkChunk, nf - ck * kDkChunk);
            float xa[kDkChunk], xb[kDkChunk];
            fetch(va, m, xa);
            if (two) fetch(vb, m, xb);
            dk_wait([&] {
                return flag_get(flags + F_R0) + kDkDepthV > ck && (!d1_on || flag_get(flags + F_R1) + kDkDepthV > ck);
            });
            float *q = vq + (size_t)(ck % kDkDepthV) * P * kDkQ + lane;
            run(va, xa, q + wib * kDkQ, m);
            if (two) run(vb, xb, q + (wib + kDkVWaves) * kDkQ, m);
            flag_put(flags + F_V0 + wib, ck + 1);
        }
        store(va, wib);
        if (two) store(vb, wib + kDkVWaves);
    } else if (wib < (uint32_t)kDkVWaves + 2u) {
        // ---------------- D: the delay stage, per (kit, channel) lane ----------------
        const uint32_t dw = wib - kDkVWaves;
        const uint32_t inst0 = g * 64u + 32u * dw;
        if (inst0 >= n) return;                            // D1 of a group whose upper half is empty
        const uint32_t col = 32u * dw + (lane >> 1);       // this lane's kit within the group
        const uint32_t kit = min(inst0 + (lane >> 1), n - 1u);
        // FxRack<2>::Process runs on the frame (sum, 0.0f): the channel-1 lane of a topology-0 kit
        const bool ch1_zero = (lane & 1u) != 0u && a.fr_coef[FRC_TOPO * n + kit] == 0u;
        const uint32_t order = a.order[kit];               // the map is the block's: delivered ahead of the launch
        auto mono = [&](uint32_t f0, int Cx, float (&xv)[kDkChunk]) {
            if (Cx == 0) {                                 // past the block's end: nothing to wait for
#pragma unroll
                for (int k = 0; k < kDkChunk; ++k) xv[k] = 0.f;
                return;
            }
            const uint32_t ck = f0 / kDkChunk;
            dk_wait([&] {
                bool ok = true;
                for (uint32_t w = 0; w < nvw; ++w) ok = ok && flag_get(flags + F_V0 + w) > ck;
                return ok;
            });
            // VoiceMap::Process: frame = 0; frame += voice at the lowest mapped note; ... (one add per voice)
            const float *q = vq + (size_t)(ck % kDkDepthV) * P * kDkQ + col;
            float m[kDkChunk];
#pragma unroll
            for (int k = 0; k < kDkChunk; ++k) m[k] = 0.0f;
            for (uint32_t t = 0; t < P; ++t) {
                const uint32_t p = (order >> (4u * t)) & 0xFu;
                const bool on = p < P;                     // kDkOrderEnd (and anything else out of range): no voice
                const float *qp = q + (on ? p : 0u) * kDkQ;
#pragma unroll
                for (int k = 0; k < kDkChunk; ++k) {
                    const float sum = m[k] + qp[k * 64];
                    m[k] = on ? sum : m[k];
                }
            }
            flag_put(flags + F_R0 + dw, ck + 1);          // (the release waits for these reads)
#pragma unroll
            for (int k = 0; k < kDkChunk; ++k) xv[k] = k < Cx && !ch1_zero ? m[k] : 0.f;
        };
        auto put = [&](uint32_t ck, const float (&av)[kDkChunk]) {
            dk_wait([&] { return flag_get(flags + F_FIN) + kDkDepthA > ck; });
            float *q = aq + (ck % kDkDepthA) * kDkQ + col;
            if ((lane & 1u) == 0u) {                       // channel 0's at either topology (the even lane's own)
#pragma unroll
                for (int k = 0; k < kDkChunk; ++k) q[k * 64] = av[k];
            }
            flag_put(flags + F_D0 + dw, ck + 1);
        };
        fr::delay_stage_from(a.ring, a.fr_state, a.fr_coef, n, nf, a.t0, lds + dw * fr::kRegion, lane, inst0, mono, put);
    } else {
        // ---------------- F: the stub reverb's balance mix, the filter, the stores; lane = kit ----------------
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
        const bool fw = a.fr_coef[FRC_TOPO * n + i] == 1u;
        float flow = __uint_as_float(a.fr_state[FRS_FLOW * n + i]);
        float fband = __uint_as_float(a.fr_state[FRS_FBAND * n + i]);
        float *const o0 = a.out + i, *const o1 = a.out + a.plane + i;
        for (uint32_t ck = 0; ck < nchunks; ++ck) {
            const uint32_t f0 = ck * kDkChunk;
            const uint32_t C = min((uint32_t)kDkChunk, nf - f0);
            dk_wait([&] { return flag_get(flags + F_D0) > ck && (!d1_on || flag_get(flags + F_D1) > ck); });
            const float *q = aq + (ck % kDkDepthA) * kDkQ + lane;
            float a0[kDkChunk];
#pragma unroll
            for (int k = 0; k < kDkChunk; ++k) a0[k] = q[k * 64];
            flag_put(flags + F_FIN, ck + 1);               // (the release waits for these reads)
#pragma unroll
            for (int k = 0; k < kDkChunk; ++k) {
                if ((uint32_t)k < C) {                     // C is wave-uniform
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
}

hipError_t launch_drumkit(const DrumkitArgs &a, hipStream_t s) {
    if (a.n == 0 || a.n_frames == 0) return hipSuccess;
    if ((a.n_frames & 3u) || (a.t0 & 1u) || a.t0 >= kFrMaxDelay || a.voices < 1u || a.voices > kDkMaxVoices ||
        a.npad != ((a.n + 63u) & ~63u) || a.plane < (uint64_t)a.n_frames * a.n || (a.bank_bytes && !a.bank))
        return hipErrorInvalidValue;
    // one workgroup per 64 kits; its seven waves are dispatched together
    const dim3 grid(a.npad / 64u), block(kDkThreads);
    const size_t lds = dk_lds_floats(a.voices) * sizeof(float);
    hipLaunchKernelGGL(drumkit_block_v1, grid, block, lds, s, a);
    return hipGetLastError();
}

}  // namespace olfx
