// ol_dsp_amd/csrc/drumkit.hip -- the reference's drum machine (a VoiceMap of sample voices, summed, into the
// effect rack) in one launch, gfx950, wave64: drumkit_block_v1 = drumkit_block<false>, OLFX_KIND_DRUMKIT (and
// drumkit_block_v1_seg = drumkit_block<true>, the launch of a block with timed notes inside it).
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
// The seven-wave pipeline (roles, queues, counters, waits) is synth_pipeline.h's, with a kit for an instrument;
// here are the sample voice with its fetch and the VoiceMap's sum.
//
// The fetch.  Lane = kit means lane = voice: left alone, every load would be a 64-row gather of 4 B, which the
// sampler measured 1.74x slower than wide fetches ("Sample voice").  So per chunk and voice
// slot the common case is cooperative: 16 load instructions, instruction j covering kits 4 j .. 4 j + 3 x 16
// consecutive frames -- lane l loads frame l & 15 of kit 4 j + (l >> 4), the kit's byte offset fetched from its
// lane with ds_bpermute, 64 contiguous bytes per voice -- all 16 in flight at once, then transposed through the
// wave's own padded LDS tile [16][65]: the writes of a 32-lane group fall on 17 banks two deep (free for
// ds_write_b32), the reads (one row, 64 consecutive columns) on distinct banks.  The loads are issued before the
// wave waits for its queue-V buffer (role_v's fetch step), so their latency hides under the previous chunk's
// consumers.
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
// LDS: 79,680 B per workgroup at P = 4, 112,448 B at 8 (the pipeline's plus the four tiles).
#include "synth_pipeline.h"
#include "svf_voice.h"

namespace olfx {

namespace {
constexpr uint32_t kDkTileStride = 65;                    // floats per tile row: row + column = the bank
constexpr uint32_t kDkTile = sy::kChunk * kDkTileStride;    // a V wave's transpose tile
constexpr uint32_t kDkNone = 0xFFFFFFFFu;                 // per-frame path: this frame reads nothing
static_assert(sy::lds_floats(4, kDkTile) * 4 == 79680 && sy::lds_floats(8, kDkTile) * 4 == 112448, "LDS per workgroup");
static_assert(sy::lds_floats(kDkMaxVoices, kDkTile) * 4 < 160 * 1024, "LDS budget");
static_assert(sy::kChunk == 16 && kSmAlign >= (uint32_t)sy::kChunk, "a cooperative load is 4 kits x 16 frames, inside the bank's padding");

// one dword at byte offset `off` of the bank (range-checked against the resource: 0 outside)
__device__ __forceinline__ float dk_bank_load(__amdgpu_buffer_rsrc_t bank, uint32_t off) {
    return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(bank, off, 0, 0));
}

// One sample voice of this lane: the Svf voice's envelopes and filter with its own coefficients, and its Sample.
struct DkVoice : VoiceEnvs {
    float low, band;
    SvfVoiceCoef kc;
    uint32_t base, len, ls, le, limit, pos, mg;
    uint32_t crec;                                         // SEG: the slot's latest timed voice record, or kNoCoef
    bool loop, playing;
};
}  // namespace

// SEG (drumkit_block_v1_seg; olfx_timed_notes): the launch's frames are a.n_seg segments with note events of their
// own; the V waves split their chunks at the segment starts (sy::role_v) and fetch per piece, so a cooperative load
// never spans a Seek -- its latency is exposed once per segment start.  D and F are the same code.
// TP (drumkit_block_v1_seg_tp; a.tp; olfx_timed_instrument_params; a SEG launch whose packet has timed records -- one
// without runs the SEG kernel as it was): a voice slot with a voice record at a segment
// start takes its coefficients (v.kc) from it ahead of the segment's events and remembers the record, whose
// envelope words voice_envs_restart reads from then on.  F takes the kit's rack records (sy::role_f).
template <bool SEG, bool TP = false>
__global__ __launch_bounds__(sy::kThreads) void drumkit_block(std::conditional_t<TP, DrumkitSegArgs, DrumkitArgs> a) {
    static_assert(SEG || !TP, "timed records come with segments");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const sy::Wg b = sy::enter(a, lds);
    const uint32_t P = b.P;

    if (sy::is_v(b)) {
        const uint32_t lane = b.lane, i = sy::v_instrument(b);
        const uint32_t sn = P * a.npad;                    // voice slots: the stride of every voice plane
        const float *c = a.vc_coef;
        float *s = a.vc_state;
        const uint32_t *sm = a.smp;
        float *tile = b.extra + b.wib * kDkTile;           // [16][65]
        const __amdgpu_buffer_rsrc_t bank =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.bank), (short)0, (int)a.bank_bytes, 0x00020000);
        // a Sample clamped to the allocation: base + len + the fetch width <= the bank
        const uint32_t bank_f = a.bank_bytes >> 2;
        const uint32_t room = bank_f > kSmAlign ? bank_f - kSmAlign : 0u;

        auto load = [&](DkVoice &v, uint32_t p) {
            const uint32_t si = p * a.npad + i;
            const VoiceEv ev = voice_envs_load(v, s, sn, si, c, sn, si, a.ev, a.ev_more, b.evslots + b.wib * 64u, lane,
                                               i - b.g * 64u, p * (a.npad >> 6) + b.g);
            v.low = s[VCS_LOW * sn + si];
            v.band = s[VCS_BAND * sn + si];
            v.crec = kNoCoef;
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
            voice_envs_store(v, s, sn, si);
            s[VCS_LOW * sn + si] = v.low;
            s[VCS_BAND * sn + si] = v.band;
            s[VCS_SM_POS * sn + si] = __uint_as_float(v.pos);
            s[VCS_SM_FLAGS * sn + si] = __uint_as_float((v.mg & ~1u) | (v.playing ? 1u : 0u));
        };
        // Sample::Process over a chunk of m frames (m is wave-uniform): x[k] = the frame the voice's filter is fed
        auto fetch = [&](DkVoice &v, uint32_t m, float (&x)[sy::kChunk]) {
            const bool silent = !v.playing || (v.pos >= v.len && (!v.loop || v.ls >= v.len));
#ifdef OLFX_DRUMKIT_PER_LANE
            const bool plain = false;                      // the variant build: lane = voice gathers only
#else
            const bool plain = v.playing && v.pos + m <= v.limit;
#endif
            const bool slow = !plain && !silent;
#pragma unroll
            for (int k = 0; k < sy::kChunk; ++k) x[k] = 0.0f;
            if (__builtin_amdgcn_ballot_w64(plain)) {
                // instruction j: kits 4 j .. 4 j + 3, 16 consecutive frames each; kits that are not plain
                // re-read the bank's first line and are not used
                const uint32_t boff = plain ? (v.base + v.pos) * 4u : 0u;
                const uint32_t fl = lane & 15u, gl = lane >> 4;
                float y[sy::kChunk];
#pragma unroll
                for (uint32_t j = 0; j < (uint32_t)sy::kChunk; ++j) {
                    const uint32_t off = (uint32_t)__builtin_amdgcn_ds_bpermute((int)((4u * j + gl) << 2), (int)boff);
                    y[j] = fl < m ? dk_bank_load(bank, off + fl * 4u) : 0.0f;
                }
#pragma unroll
                for (uint32_t j = 0; j < (uint32_t)sy::kChunk; ++j) tile[fl * kDkTileStride + 4u * j + gl] = y[j];
                // one wave writes and reads its tile: LDS operations of a wave complete in order; the fences keep
                // the compiler from moving the reads above the other lanes' writes
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
                for (uint32_t k = 0; k < (uint32_t)sy::kChunk; ++k) {
                    const float t = tile[k * kDkTileStride + lane];
                    x[k] = plain ? t : 0.0f;
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
            if (plain) v.pos += m;
            if (__builtin_amdgcn_ballot_w64(slow)) {
                // Sample::Process frame by frame: the byte offset each frame reads (or none), then the gather
                uint32_t o[sy::kChunk];
#pragma unroll
                for (uint32_t k = 0; k < (uint32_t)sy::kChunk; ++k) {
                    const bool on = slow && k < m;
                    const bool rd = on && v.pos < v.len;
                    o[k] = rd ? (v.base + v.pos) * 4u : kDkNone;
                    v.pos += rd ? 1u : 0u;
                    if (on && v.loop && (!rd || (v.le && v.pos > v.le))) v.pos = v.ls;
                }
#pragma unroll
                for (uint32_t k = 0; k < (uint32_t)sy::kChunk; ++k) {
                    const float yk = dk_bank_load(bank, o[k] == kDkNone ? 0u : o[k]);
                    x[k] = o[k] == kDkNone ? x[k] : yk;
                }
            }
        };
        auto run = [&](DkVoice &v, const float (&x)[sy::kChunk], float *q, uint32_t m) {
            if (m == (uint32_t)sy::kChunk) {
#pragma unroll 4
                for (uint32_t k = 0; k < (uint32_t)sy::kChunk; ++k)
                    q[k * 64u] = svf_voice_tick_src(v.ea, v.ef, v.low, v.band, x[k], v.kc);
            } else {
#pragma unroll
                for (uint32_t k = 0; k < (uint32_t)sy::kChunk; ++k)
                    if (k < m) q[k * 64u] = svf_voice_tick_src(v.ea, v.ef, v.low, v.band, x[k], v.kc);
            }
        };
        if constexpr (SEG && !TP) {
            // a segment's events on the live voice, as load applies the block's: the gate and the envelopes, Seek(0),
            // Play() / Pause(), and the stored pitch (the last segment's value wins)
            auto start = [&](DkVoice &v, uint32_t p, const VoiceEv &ev) {
                const uint32_t si = p * a.npad + i;
                voice_envs_restart(v, ev, c, sn, si);
                if (ev.op & VEV_SEEK) v.pos = 0u;
                if (ev.op & VEV_GATE_SET) v.playing = (ev.op & VEV_GATE_ON) != 0u;
                if (ev.op & VEV_FREQ) s[VCS_FREQ * sn + si] = ev.freq;
            };
            sy::role_v<DkVoice, float[sy::kChunk], true>(b, load, run, store, fetch, &a, start);
        } else if constexpr (TP) {
            // ... and ahead of them the slot's voice record of the segment, if it has one
            auto start = [&](DkVoice &v, uint32_t p, const VoiceEv &ev, uint32_t r) {
                const uint32_t si = p * a.npad + i;
                const float *t = a.tp.vrec;
                const uint32_t T = a.tp.n_v;
                if (r != kNoCoef) {
                    v.crec = r;
                    v.kc = SvfVoiceCoef{0.5f * t[VCC_AMP_AMT * T + r], 0.0f, 0.0f, t[VCC_CUTOFF * T + r],
                                        t[VCC_FENV_AMT * T + r], t[VCC_FC_MAX * T + r], t[VCC_DRIVE * T + r],
                                        t[VCC_DAMP_RES * T + r], 1.0f / (t[VCC_SR * T + r] * 2.0f)};
                }
                const bool rec = v.crec != kNoCoef;
                voice_envs_restart(v, ev, rec ? t : c, rec ? T : sn, rec ? v.crec : si);
                if (ev.op & VEV_SEEK) v.pos = 0u;
                if (ev.op & VEV_GATE_SET) v.playing = (ev.op & VEV_GATE_ON) != 0u;
                if (ev.op & VEV_FREQ) s[VCS_FREQ * sn + si] = ev.freq;
            };
            sy::role_v<DkVoice, float[sy::kChunk], true, true>(b, load, run, store, fetch, &a, start, &a.tp);
        } else {
            sy::role_v<DkVoice, float[sy::kChunk]>(b, load, run, store, fetch);
        }
    } else if (sy::is_d(b)) {
        const uint32_t order = a.order[sy::d_instrument(b)];   // the map is the block's: delivered ahead of the launch
        // VoiceMap::Process: frame = 0; frame += voice at the lowest mapped note; ... (one add per voice)
        sy::role_d<true>(b, a, [&](const float *q, float (&m)[sy::kChunk]) {
            for (uint32_t t = 0; t < P; ++t) {
                const uint32_t p = (order >> (4u * t)) & 0xFu;
                const bool on = p < P;                     // kDkOrderEnd (and anything else out of range): no voice
                const float *qp = q + (on ? p : 0u) * sy::kQ;
#pragma unroll
                for (int k = 0; k < sy::kChunk; ++k) {
                    const float sum = m[k] + qp[k * 64];
                    m[k] = on ? sum : m[k];
                }
            }
        });
    } else {
        sy::role_f<true, TP>(b, a, [&]() -> const InstrumentTimed * {
            if constexpr (TP) return &a.tp;
            else return nullptr;
        }());
    }
}

hipError_t launch_drumkit(const DrumkitSegArgs &a, hipStream_t s) {
    if (a.n == 0 || a.n_frames == 0) return hipSuccess;
    if (!instrument_args_ok(a, kDkMaxVoices) || (a.bank_bytes && !a.bank) || !instrument_timed_ok(a, a.tp, true))
        return hipErrorInvalidValue;
    if (a.tp.vtab) return sy::launch(drumkit_block<true, true>, a, kDkTile, s);
    const DrumkitArgs &plain = a;                          // (the other kernels take the arguments they always took)
    return sy::launch(a.n_seg > 1u ? drumkit_block<true> : drumkit_block<false>, plain, kDkTile, s);
}

}  // namespace olfx
