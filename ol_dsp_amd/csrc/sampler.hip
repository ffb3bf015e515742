// ol_dsp_amd/csrc/sampler.hip -- the sample-playback voice, OLFX_KIND_VOICE_SAMPLE:
// SynthVoice(SampleSoundSource<1>(Sample), SvfFilter) over a device-resident bank of mono PCM.
//
// Reference call sequence per sample: SynthVoice::Process (modules/synthlib/SynthVoice.h:41-53), as
// voice.hip, with sound_source_->Process(frame) = Sample::Process (Sample.cpp:9-23) on the caller's
// zeroed frame:
//   if (playing) { n = Read(frame); current_frame_ += n;
//                  if (Loop && (!n || (loop_end_ && current_frame_ > loop_end_))) Seek(loop_start_); }
// over the in-memory source (Read: frame = pcm[pos++], 1 while pos < len, else nothing, 0;
// Seek(k): pos = min(k, len)).  SetFreq only stores the pitch (SampleSoundSource.h:28-30): the
// portamento has no audible effect and is not run.  One cursor: current_frame_ and the data position
// differ only after Seek(loop_start >= len), and nothing is read from then on.
//
// sampler_block_v1 is voice_block_v5's four-role pipeline (voice_roles.h: ENV, FREQ and FILT are the
// same code, so the envelopes and the Svf are the saw voice's, operation for operation) with a SRC
// role in OSC's place.  One workgroup = 64 voices; SRC hands FILT the source through an LDS ring in
// [frame][voice] order.
//
// The fetch.  Lane = voice would make every load a 64-row gather (4 B from each of 64 samples: the
// access shape MI355X serves ~17x below its streaming rate).  Instead a voice's next kSmWin = 64
// frames are one instruction: 64 lanes x 4 B = 256 contiguous bytes of ONE voice (its byte offset
// broadcast with v_readlane), 64 such loads per window all in flight at once (register staging, 64
// VGPRs), then written transposed into the ring: lane l holds frame f0 + l and writes row f0 + l,
// column = voice.  Rows are kSmStride = 65 floats apart, so those 64 writes fall in 64 different
// banks ((row + column) mod 64), and FILT's reads (one row, 64 consecutive columns) do too.
// A window is fetched at the step SRC owes its first chunk (step 8 w + 1) and holds 8 chunks; FILT
// still reads the previous window's last chunk during that step, so the ring holds two windows:
// 128 rows x 65 floats = 33,280 B, 54.3 KB of LDS per workgroup with the other queues -- two
// workgroups per CU (160 KB) as v5.
// The wide fetch serves a voice whose window is one run: playing, and neither the sample's end nor
// its loop turn inside the window.  Voices that read nothing (paused, unassigned, exhausted) write
// zeros.  The others -- a turn or an end inside the window, loops shorter than it -- take a
// per-frame path: the lane walks Sample::Process's rule frame by frame into byte offsets (kept in
// its ring column), then gathers them eight loads at a time.
//
// Bounds.  Every load goes through a buffer resource over the bank allocation, offsets in the
// vector operand (the one the hardware range-checks): no load can touch memory outside it, whatever
// the words hold.  On top, base / len / loop points are clamped here to what the host laid out
// (olfx_host.cpp bank_plan: kSmAlign-aligned starts, a padded tail of kSmAlign floats), the cursor
// to len, and lanes past the window's frames do not load.
#include "voice_roles.h"

namespace olfx {

namespace {

constexpr uint32_t kSmWin = 64;                 // frames per window = lanes per voice and load
constexpr uint32_t kSmRows = 2 * kSmWin;        // ring rows (a power of two)
constexpr uint32_t kSmStride = 65;              // floats per ring row: row + column = the bank
constexpr uint32_t kSmNone = 0xFFFFFFFFu;       // per-frame path: this frame reads nothing
static_assert(kSmWin == kSmAlign, "the bank's padding is the fetch width");
static_assert(kSmWin % kVcChunk == 0 && kSmWin == 64, "a window is whole chunks and one wave wide");

// one dword at byte offset `off` of the bank (range-checked against the resource: 0 outside)
__device__ __forceinline__ float bank_load(__amdgpu_buffer_rsrc_t bank, uint32_t off) {
    return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(bank, off, 0, 0));
}

}  // namespace

// SEG (sampler_block_v1_seg, timed events: voice_roles.h VoiceSegs): the block is its segments' chunks.  SRC
// takes a segment's VEV_SEEK and `playing` at that segment's first chunk, where a window starts too (a window
// lies inside one segment: at most 8 chunks, all full but the segment's last), and stores the last
// frequency at the end.  The ring is addressed by chunk, 8 rows each whatever the chunk's frames: that is the
// frame while the chunks are full, and keeps a short chunk's successor off FILT's rows.
template <bool SEG>
__device__ __forceinline__ void sampler_v1(const VoiceArgs &a) {
    __shared__ VoiceEnvQ eq;                    // ENV -> FREQ (fc_in), FILT (amp)
    __shared__ float win[kSmRows * kSmStride];  // SRC -> FILT: the source, [frame mod 128][voice], padded rows
    __shared__ VoiceFreqQ fdq;                  // FREQ -> FILT: (-damp, fq)
    __shared__ uint2 evslot[64];                // ENV's staging of the block's events (SRC reads it)
    __shared__ uint32_t hw_simd[5];
    VoiceSegs *sg = nullptr;
    if constexpr (SEG) {
        __shared__ VoiceSegs segs;
        sg = &segs;
        voice_segs_bounds(a, segs);               // published by voice_role_of_wave's barrier
    }
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // roles by SIMD, as v5: ENV with FILT, SRC (in OSC's place) with FREQ
    const uint32_t role = voice_role_of_wave(hw_simd, lane, wave);
    if (role == 3u) __builtin_amdgcn_s_setprio(2);
    const VoiceLane v = SEG ? voice_lane_seg(a) : voice_lane(a);

    if (role == 0) {
        voice_role_env<SEG>(a, v, eq, evslot, sg);
    } else if (role == 1) {
        // ---- SRC: Sample::Process over the bank ----
        const uint32_t n = v.n, i = v.i, nf = v.nf, nsteps = v.nsteps;
        float *s = a.state;
        const uint32_t *sm = a.smp;
        const __amdgpu_buffer_rsrc_t bank =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.bank), (short)0, (int)a.bank_bytes, 0x00020000);
        // the voice's Sample, clamped to the allocation: base + len + the fetch width <= the bank
        const uint32_t bank_f = a.bank_bytes >> 2;
        const uint32_t room = bank_f > kSmWin ? bank_f - kSmWin : 0u;
        const uint32_t base = min(sm[SMC_BASE * n + i], room);
        const uint32_t len = min(sm[SMC_LEN * n + i], room - base);
        const uint32_t ls = min(sm[SMC_LS * n + i], len);
        const uint32_t le0 = sm[SMC_LE * n + i], le = le0 < len ? le0 : 0u;
        const uint32_t mg = sm[SMC_MODE * n + i];
        const bool loop = mg & 1u;
        uint32_t pos = __float_as_uint(s[VCS_SM_POS * n + i]);
        uint32_t fl = __float_as_uint(s[VCS_SM_FLAGS * n + i]);
        if ((fl >> 1) != (mg >> 1)) {            // another Sample object since the last block: fresh
            pos = 0u;
            fl = 0u;
        }
        bool playing = fl & 1u;
        pos = min(pos, len);
        // reads without a turn stop before `limit`: the end, or loop_end (the turn follows the read
        // that makes current_frame_ > loop_end_)
        [[maybe_unused]] const uint32_t limit = (loop && le) ? le : len;
        const uint32_t lane4 = lane * 4u;
        // SEG: the frame the current window ends at; the last frequency a segment set
        [[maybe_unused]] uint32_t wend = 0u, fbits = 0u;
        [[maybe_unused]] bool fset = false;
        SegCursor<SEG> cu(sg, a.n_seg);

        for (uint32_t k = 0; k < nsteps; ++k) {
            if (!SEG && k == 1) {
                // the block's events, staged by ENV before the first barrier: any NoteOn / GateOn is
                // Seek(0), the last gate call Play() or Pause() (SampleSoundSource.h:21-26); the pitch
                // is stored (SynthVoice::freq_)
                const VoiceEv ev = staged_event(a, evslot, v.me);
                if (ev.op & VEV_SEEK) pos = 0u;
                if (ev.op & VEV_GATE_SET) playing = (ev.op & VEV_GATE_ON) != 0u;
                if (ev.op & VEV_FREQ) s[VCS_FREQ * n + i] = ev.freq;
            }
            if constexpr (SEG) {
                if (k >= 1 && k + 1 < nsteps && cu.first) {
                    const VoiceEv ev = seg_event(*sg, cu.seg, v.me);
                    if (ev.op & VEV_SEEK) pos = 0u;
                    if (ev.op & VEV_GATE_SET) playing = (ev.op & VEV_GATE_ON) != 0u;
                    if (ev.op & VEV_FREQ) {
                        fbits = __float_as_uint(ev.freq);
                        fset = true;
                    }
                }
            }
            if (k >= 1 && k + 1 < nsteps &&
                (SEG ? (cu.first || cu.f0 == wend) : ((k - 1) & (kSmWin / kVcChunk - 1)) == 0)) {
                // window w = (k - 1) / 8: frames [f0, f0 + nwin) in ring rows f0 ... (SEG: the rows of chunk
                // k - 1 ..., the frames left of the segment)
                const uint32_t f0 = (k - 1) * kVcChunk;
                const uint32_t left = SEG ? cu.end - cu.f0 : nf - f0;
                const uint32_t nwin = left < kSmWin ? left : kSmWin;
                if constexpr (SEG) wend = cu.f0 + nwin;
                const bool silent = !playing || (pos >= len && (!loop || ls >= len));
#ifdef OLFX_SAMPLER_PER_LANE
                // variant build (tools/sampler_ab.py): every playing voice on the per-frame gather, i.e.
                // the lane = voice fetch this kernel is designed around avoiding
                const bool plain = false;
#else
                const bool plain = playing && pos + nwin <= limit;
#endif
                const bool slow = !plain && !silent;
                const uint64_t pm = __builtin_amdgcn_ballot_w64(plain);
                if (pm) {
                    // one load per voice: its next 64 frames, frame f0 + lane in this lane (voices
                    // that are not plain re-read the bank's first line and are not written)
                    const uint32_t boff = plain ? (base + pos) * 4u : 0u;
                    float x[64];
#pragma unroll
                    for (uint32_t r = 0; r < 64; ++r) {
                        const uint32_t off = (uint32_t)__builtin_amdgcn_readlane((int)boff, (int)r);
                        x[r] = lane < nwin ? bank_load(bank, off + lane4) : 0.0f;
                    }
                    float *wrow = &win[((f0 + lane) & (kSmRows - 1)) * kSmStride];
#pragma unroll
                    for (uint32_t r = 0; r < 64; ++r)
                        if ((pm >> r) & 1ull) wrow[r] = x[r];
                }
                if (plain) pos += nwin;
                float *wcol = &win[lane];
                auto row = [&](uint32_t f) { return ((f0 + f) & (kSmRows - 1)) * kSmStride; };
                if (silent)
                    for (uint32_t f = 0; f < nwin; ++f) wcol[row(f)] = 0.0f;
                if (__builtin_amdgcn_ballot_w64(slow)) {
                    if (slow) {
                        // Sample::Process frame by frame: the byte offset each frame reads (or none)
                        for (uint32_t f = 0; f < nwin; ++f) {
                            const bool rd = pos < len;
                            wcol[row(f)] = __uint_as_float(rd ? (base + pos) * 4u : kSmNone);
                            pos += rd ? 1u : 0u;
                            if (loop && (!rd || (le && pos > le))) pos = ls;
                        }
                        // the gather, eight loads in flight
                        for (uint32_t f = 0; f < nwin; f += 8) {
                            uint32_t o[8];
                            float y[8];
#pragma unroll
                            for (uint32_t u = 0; u < 8; ++u)
                                o[u] = f + u < nwin ? __float_as_uint(wcol[row(f + u)]) : kSmNone;
#pragma unroll
                            for (uint32_t u = 0; u < 8; ++u) y[u] = bank_load(bank, o[u] == kSmNone ? 0u : o[u]);
#pragma unroll
                            for (uint32_t u = 0; u < 8; ++u)
                                if (f + u < nwin) wcol[row(f + u)] = o[u] == kSmNone ? 0.0f : y[u];
                        }
                    }
                }
            }
            if constexpr (SEG)
                if (k >= 1 && k + 1 < nsteps) cu.next();
            __syncthreads();
        }
        if constexpr (SEG)
            if (fset) s[VCS_FREQ * n + i] = __uint_as_float(fbits);     // the last segment's
        s[VCS_SM_POS * n + i] = __uint_as_float(pos);
        s[VCS_SM_FLAGS * n + i] = __uint_as_float((mg & ~1u) | (playing ? 1u : 0u));
    } else if (role == 2) {
        voice_role_freq<SEG>(a, v, eq, fdq, sg);
    } else {
        // chunk c's source samples: ring rows (8 c + j) mod 128, this lane's column
        voice_role_filt<kSmStride, SEG>(a, v, eq, fdq, [&](uint32_t c2) {
            return &win[((c2 * kVcChunk) & (kSmRows - 1)) * kSmStride + lane];
        }, sg);
    }
}
__global__ __launch_bounds__(256) void sampler_block_v1(VoiceArgs a) { sampler_v1<false>(a); }
__global__ __launch_bounds__(256) void sampler_block_v1_seg(VoiceArgs a) { sampler_v1<true>(a); }

hipError_t launch_sampler(const VoiceArgs &a, hipStream_t s) {
    if (a.n == 0 || a.n_frames == 0) return hipSuccess;
    if ((uint64_t)kVcChunk * a.n * 4u > 0xFFFFFFFFull) return hipErrorInvalidValue;   // FILT's chunk output resource
    if (a.n_seg > 1) {                    // timed events: the segmented kernel
        if (a.n_seg > kSegCap || !a.seg || !a.ev) return hipErrorInvalidValue;
        hipLaunchKernelGGL(sampler_block_v1_seg, dim3((a.n + 63) / 64), dim3(256), 0, s, a);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(sampler_block_v1, dim3((a.n + 63) / 64), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace olfx
