// ol_dsp_amd/csrc/voice.hip -- synthlib SynthVoice, one lane per voice, state in registers.
//
// Reference call sequence per sample: modules/synthlib/SynthVoice.h:41-53
//   amp = ampEnv.Process(gate) * amp_env_amount
//   osc.SetFreq(port.Process(freq)); s = osc.Process()          (WAVE_POLYBLEP_SAW, amp 0.5)
//   fc = cutoff + ((filtEnv.Process(gate) * 20000) * filter_env_amount)
//   svf.SetFreq(fc); svf.Process(s); out = svf.Low() * amp
// DaisySP (Oscillator, Adsr, Svf) is not in the reference tree: the arithmetic restates its
// published algorithm ("parity unpinned").  Setter-side transcendentals
// (expf/logf/powf in Adsr/Svf/Port setters, mtof) run on the host; the per-sample sinf of
// Svf::SetFreq runs here.  VALU-bound: ~5 B of HBM traffic per sample.
//
// MOOG = true is the Daisy synth firmware's voice, SynthVoice(OscillatorSoundSource, MoogFilter)
// (ol_daisy/app/synth/main.cpp:49-52, Filter.h:35-63): MoogFilter::Process is a no-op and
// Low(frame) = daisysp::LadderFilter::Process(frame) with SetFreq(fc) (-> SetAlpha) every sample,
// unclamped.  LadderFilter: 4x linear-interpolated oversampling, Pade tanh of the feedback sum,
// four one-zero/one-pole stages, LP24 output (restated, [unverified] like the rest of DaisySP;
// oracle/voice_ref.c ladder_process).  ~4x the Svf voice's VALU work per sample.
#include "moog_voice.h"

namespace olfx {

// (the Moog voice's per-sample arithmetic, with the note on contraction: moog_voice.h)

// voice_block_v4: the MoogFilter voice.  One workgroup = 64 voices, the voice pipelined over two
// waves that hand each sample's values on through an LDS double buffer (one barrier per 8-sample
// chunk):
//   feed wave   : amp envelope, portamento, oscillator, filter envelope, cutoff,
//                 LadderFilter::SetFreq -> SetAlpha          -> (src * drive, amp, alpha, Qadjust)
//   filter wave : LadderFilter::Process, output store
// The ladder's serial recurrence dominates the voice, so the feed roles share one wave.  (The Svf
// voice runs voice_block_v5 below, over four role waves.)
// SEG (voice_block_v4_seg, timed events: voice_roles.h VoiceSegs): the block is its segments' chunks; at a
// segment's first chunk the feed wave applies that segment's events to its live registers -- the gate
// events and Env::begin as at a launch's start, the segment's frequency -- and the state is stored once.
template <bool SEG>
__device__ __forceinline__ void voice_v4(const VoiceArgs &a) {
    constexpr uint32_t kRoles = 2u;
    __shared__ float4 q[2][kVcChunk][64];
    __shared__ uint32_t fflags[64];
    __shared__ uint2 evslot[64];
    VoiceSegs *sg = nullptr;
    if constexpr (SEG) {
        __shared__ VoiceSegs segs;
        sg = &segs;
        voice_segs_bounds(a, segs);
        __syncthreads();
    }
    const uint32_t n = a.n;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t i0 = blockIdx.x * 64 + lane;
    // dead lanes of the last workgroup mirror voice n-1 exactly (same state, same coefficients,
    // same events), so their stores write the values voice n-1's lane writes
    const uint32_t i = i0 < n ? i0 : n - 1;
    const uint32_t me = i - blockIdx.x * 64;
    const uint32_t nf = a.n_frames;
    const uint32_t nchunks = SEG ? a.n_chunks : (nf + kVcChunk - 1) / kVcChunk;
    const float *c = a.coef;
    float *s = a.state;
    const bool filt_role = wave == kRoles - 1;

    // ---------------- amp and/or cutoff roles (compile-time role flags: straight-line chunks) ----------------
    auto feed = [&](auto amp_c, auto cut_c) {
        constexpr bool AMP = decltype(amp_c)::value, CUT = decltype(cut_c)::value;
        // the block's note events first (one feed wave per workgroup applies them); the state loads
        // are issued before the event read, so their latency hides under its host-link round trip
        uint32_t flags0 = __float_as_uint(s[VCS_FLAGS * n + i]);
        float xa0 = s[VCS_ENVA_X * n + i], xf0 = s[VCS_ENVF_X * n + i];
        const float freq_s = s[VCS_FREQ * n + i];
        VoiceEv ev{0u, 0.0f};
        if constexpr (SEG) {
            voice_events_stage(a, *sg, lane, blockIdx.x);
        } else {
            ev = voice_event(a, evslot, lane, me);
            apply_gate_events(ev, flags0, xa0, xf0);
        }
        bool gate = (flags0 >> 8) & 1u;
        // (SEG: the coefficients are loop-carried -- a segment with VEV_COEF replaces them)
        float amp_amt = c[VCC_AMP_AMT * n + i], port_c = c[VCC_PORT_COEF * n + i];
        const float inv_sr = c[VCC_INV_SR * n + i];
        float freq = (ev.op & VEV_FREQ) ? ev.freq : freq_s;
        [[maybe_unused]] bool fset = false;               // SEG: some segment set the frequency
        float cutoff = c[VCC_CUTOFF * n + i], fenv_amt = c[VCC_FENV_AMT * n + i];
        // ladder: drive_scaled (VCC_DRIVE), 1/(4 sr) (VCC_FC_MAX)
        float drive = c[VCC_DRIVE * n + i];
        float fc_max = c[VCC_FC_MAX * n + i];
        float phase = s[VCS_PHASE * n + i];
        float port_z = s[VCS_PORT_Z * n + i];
        bool gprev_a = (flags0 >> 6) & 1u, gprev_f = (flags0 >> 7) & 1u;
        Env ea, ef;
        // (SEG: the envelope coefficients stay in registers for the segment starts)
        [[maybe_unused]] float ca[5], cf[5];
        if constexpr (SEG) {
            ca[0] = c[VCC_ATK_D0A * n + i]; ca[1] = c[VCC_ATK_TGT_A * n + i]; ca[2] = c[VCC_DEC_D0A * n + i];
            ca[3] = c[VCC_REL_D0A * n + i]; ca[4] = c[VCC_SUS_A * n + i];
            cf[0] = c[VCC_ATK_D0F * n + i]; cf[1] = c[VCC_ATK_TGT_F * n + i]; cf[2] = c[VCC_DEC_D0F * n + i];
            cf[3] = c[VCC_REL_D0F * n + i]; cf[4] = c[VCC_SUS_F * n + i];
        } else {
            if constexpr (AMP)
                ea.begin(gate, gprev_a, flags0 & 7u, xa0, c[VCC_ATK_D0A * n + i],
                         c[VCC_ATK_TGT_A * n + i], c[VCC_DEC_D0A * n + i], c[VCC_REL_D0A * n + i], c[VCC_SUS_A * n + i]);
            if constexpr (CUT)
                ef.begin(gate, gprev_f, (flags0 >> 3) & 7u, xf0, c[VCC_ATK_D0F * n + i],
                         c[VCC_ATK_TGT_F * n + i], c[VCC_DEC_D0F * n + i], c[VCC_REL_D0F * n + i], c[VCC_SUS_F * n + i]);
        }

        SegCursor<SEG> cu(sg, a.n_seg);
        for (uint32_t k = 0; k <= nchunks; ++k) {
            if (k < nchunks) {
                if constexpr (SEG) {
                    if (cu.first) {
                        if (k) {                 // the live state as the flags word and levels a launch would load
                            flags0 = ea.mode | ef.mode << 3 | (uint32_t)gprev_a << 6 | (uint32_t)gprev_f << 7 |
                                     (uint32_t)gate << 8;
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
                            port_c = seg_coef(a, r, VCC_PORT_COEF);
                            drive = seg_coef(a, r, VCC_LADDER_DRIVE);
                        }
                        apply_gate_events(sev, flags0, xa0, xf0);
                        gate = (flags0 >> 8) & 1u;
                        gprev_a = (flags0 >> 6) & 1u;
                        gprev_f = (flags0 >> 7) & 1u;
                        if (sev.op & VEV_FREQ) {
                            freq = sev.freq;
                            fset = true;
                        }
                        ea.begin(gate, gprev_a, flags0 & 7u, xa0, ca[0], ca[1], ca[2], ca[3], ca[4]);
                        ef.begin(gate, gprev_f, (flags0 >> 3) & 7u, xf0, cf[0], cf[1], cf[2], cf[3], cf[4]);
                    }
                }
                const uint32_t f0 = k * kVcChunk;
                const uint32_t m = SEG ? cu.len() : (nf - f0 < (uint32_t)kVcChunk ? nf - f0 : (uint32_t)kVcChunk);
                float4 *qb = &q[k & 1][0][lane];
                for_chunk(m, [&](uint32_t j) {
                    float2 ab, cd;
                    if constexpr (AMP) ab = moog_amp_tick(ea, port_z, phase, freq, amp_amt, port_c, inv_sr, drive);
                    if constexpr (CUT) cd = moog_cut_tick(ef, fenv_amt, cutoff, fc_max);
                    if constexpr (AMP && CUT) {
                        qb[j * 64] = make_float4(ab.x, ab.y, cd.x, cd.y);
                    } else if constexpr (AMP) {
                        reinterpret_cast<float2 *>(&qb[j * 64])[0] = ab;
                    } else {
                        reinterpret_cast<float2 *>(&qb[j * 64])[1] = cd;
                    }
                });
                cu.next();
            }
            __syncthreads();
        }
        // the flags word holds both envelopes: the cutoff role hands its bits to the amp role
        if constexpr (CUT && !AMP) fflags[lane] = ef.mode << 3 | (uint32_t)gprev_f << 7;
        __syncthreads();
        if constexpr (AMP) {
            const uint32_t fbits = CUT ? (ef.mode << 3 | (uint32_t)gprev_f << 7) : fflags[lane];
            s[VCS_PHASE * n + i] = phase;
            s[VCS_PORT_Z * n + i] = port_z;
            s[VCS_ENVA_X * n + i] = ea.x;
            s[VCS_FLAGS * n + i] = __uint_as_float(ea.mode | fbits | (uint32_t)gprev_a << 6 | (uint32_t)gate << 8);
            if (SEG ? fset : (ev.op & VEV_FREQ) != 0u) s[VCS_FREQ * n + i] = freq;     // SEG: the last segment's
        }
        if constexpr (CUT) s[VCS_ENVF_X * n + i] = ef.x;
    };
    if (!filt_role) {
        feed(std::true_type{}, std::true_type{});
    } else {
        // ---------------- filter role: LadderFilter::Process ----------------
        float k_or_unused = c[VCC_DAMP_RES * n + i];           // ladder: K (VCC_LADDER_K); SEG: loop-carried
        Ladder L;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            L.z0[k] = s[(VCS_LZ0 + k) * n + i];
            L.z1[k] = s[(VCS_LZ1 + k) * n + i];
        }
        L.old = s[VCS_LOLD * n + i];
        float *out = a.out + i;
        SegCursor<SEG> cu(sg, a.n_seg);
        for (uint32_t k = 0; k <= nchunks; ++k) {
            if (k > 0) {
                if constexpr (SEG) {
                    if (cu.first && a.tc)        // timed parameters: this segment's resonance
                        if (const uint32_t r = seg_coef_record(a, *sg, cu.seg, seg_event(*sg, cu.seg, me), n, me); r != kNoCoef)
                            k_or_unused = seg_coef(a, r, VCC_LADDER_K);
                }
                const uint32_t f0 = SEG ? (uint32_t)cu.f0 : (k - 1) * kVcChunk;
                const uint32_t m = SEG ? cu.len() : (nf - f0 < (uint32_t)kVcChunk ? nf - f0 : (uint32_t)kVcChunk);
                const float4 *qb = &q[(k - 1) & 1][0][lane];
                for_chunk(m, [&](uint32_t j) {
                    const float4 v = qb[j * 64];
                    const float y = ladder_tick(L, v, k_or_unused);
                    out[(size_t)(f0 + j) * n] = y;
                });
                cu.next();
            }
            __syncthreads();
        }
        __syncthreads();                                      // the flags hand-off barrier
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            s[(VCS_LZ0 + k) * n + i] = L.z0[k];
            s[(VCS_LZ1 + k) * n + i] = L.z1[k];
        }
        s[VCS_LOLD * n + i] = L.old;
    }
}
__global__ __launch_bounds__(128) void voice_block_v4(VoiceArgs a) { voice_v4<false>(a); }
__global__ __launch_bounds__(128) void voice_block_v4_seg(VoiceArgs a) { voice_v4<true>(a); }

// ---------------------------------------------------------------------------------------------
// voice_block_v5 (SvfFilter voices): v4's arithmetic, operation for operation, over
// FOUR role waves per workgroup of 64 voices (two workgroups per CU, two waves per SIMD):
//   ENV  : the amp and filter Adsr, the cutoff sum, its clamp                 -> (amp, fc)
//   OSC  : Port, the oscillator's phase, the polyBLEP saw                     -> src
//   FREQ : Svf::SetFreq(fc_in)                                                -> (-damp, fq)
//   FILT : the two Svf passes, Low() * amp, the output store
// A three-stage pipeline over 8-sample chunks (kVcChunk): at step k ENV makes chunk k, OSC and FREQ chunk
// k-1, FILT chunk k-2 (and reads that chunk's amp straight from ENV's queue, which holds three
// chunks); one barrier per step; 24 KB of LDS per workgroup.  Measured per role (16-sample chunks,
// 18 steps; the others skipping their arithmetic): the skeleton (launch, state,
// 18 barriers) 9.7 us, FREQ 10.0, FILT 15, OSC 20, ENV 26 of the kernel's 43.6 us.  The envelopes
// of a full chunk run speculatively (Env::step_spec, no per-sample lane vote and branch) and the
// chunk is redone exactly when a lane's segment ended in it.  Roles are assigned by SIMD (below).
// ---------------------------------------------------------------------------------------------
// FILT (the Svf recurrence, the critical chain of the ENV + FILT pair) issues ahead of ENV on
// their SIMD at wave priority 2: ~2 % same-box; OSC raised too was slower.
// SEG (voice_block_v5_seg, timed events): as voice_block_v4_seg; ENV stages every segment's records, OSC
// takes a segment's frequency at that segment's first chunk and stores the last one at the end.
template <bool SEG>
__device__ __forceinline__ void voice_v5(const VoiceArgs &a) {
    __shared__ VoiceEnvQ eq;                    // ENV -> OSC, FREQ (fc_in), FILT (amp): three chunks live
    __shared__ float sq[2][kVcChunk][64];       // OSC -> FILT: src
    __shared__ VoiceFreqQ fdq;                  // FREQ -> FILT: (-damp, fq)
    __shared__ uint2 evslot[64];                // ENV's staging of the block's events (OSC reads it)
    __shared__ uint32_t hw_simd[5];             // the SIMD of each wave; [4]: wave 0's slot parity
    VoiceSegs *sg = nullptr;
    if constexpr (SEG) {
        __shared__ VoiceSegs segs;
        sg = &segs;
        voice_segs_bounds(a, segs);               // published by voice_role_of_wave's barrier
    }
    const uint32_t n = a.n;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // roles by SIMD (voice_roles.h): ENV with FILT and OSC with FREQ on every SIMD
    const uint32_t role = voice_role_of_wave(hw_simd, lane, wave);
    // the role with the per-sample recurrence (FILT) ahead of its SIMD partner at issue
    if (role == 3u) __builtin_amdgcn_s_setprio(2);
    const VoiceLane v = SEG ? voice_lane_seg(a) : voice_lane(a);   // dead lanes mirror voice n-1, as in v4
    const uint32_t i = v.i, me = v.me, nsteps = v.nsteps;
    const float *c = a.coef;
    float *s = a.state;
    if (role == 0) {
        voice_role_env<SEG>(a, v, eq, evslot, sg);
    } else if (role == 1) {
        // ---- OSC (SynthVoice.h:44-45): Port::Process, Oscillator::SetFreq / Process, WAVE_POLYBLEP_SAW,
        //      amp 0.5 ----
        float port_c = c[VCC_PORT_COEF * n + i];          // (SEG: a segment with VEV_COEF replaces it)
        const float inv_sr = c[VCC_INV_SR * n + i];
        float freq = s[VCS_FREQ * n + i];
        float phase = s[VCS_PHASE * n + i], port_z = s[VCS_PORT_Z * n + i];
        [[maybe_unused]] bool fset = false;               // SEG: some segment set the frequency
        SegCursor<SEG> cu(sg, a.n_seg);
        for (uint32_t k = 0; k < nsteps; ++k) {
            if (!SEG && k == 1) {
                // the block's pitch events (NoteOn: mtof(note), SetFrequency: Hz), staged by ENV
                // before the first barrier; OSC's first chunk is step 1
                const VoiceEv ev = staged_event(a, evslot, me);
                if (ev.op & VEV_FREQ) {
                    freq = ev.freq;
                    s[VCS_FREQ * n + i] = freq;
                }
            }
            if (k >= 1 && k + 1 < nsteps) {
                if constexpr (SEG) {
                    if (cu.first) {              // the segment's pitch events, staged by ENV before the first barrier
                        const VoiceEv ev = seg_event(*sg, cu.seg, me);
                        if (const uint32_t r = seg_coef_record(a, *sg, cu.seg, ev, n, me); r != kNoCoef)
                            port_c = seg_coef(a, r, VCC_PORT_COEF);       // timed parameters: this segment's portamento
                        if (ev.op & VEV_FREQ) {
                            freq = ev.freq;
                            fset = true;
                        }
                    }
                }
                const uint32_t m = [&] { if constexpr (SEG) return cu.len(); else return v.len(k - 1); }();
                float *qo = &sq[(k - 1) & 1][0][lane];
                if (m == (uint32_t)kVcChunk) {
                    // only Port and the phase are recurrences: run them for the chunk, then the
                    // polyBLEP saw per sample over four packed sample pairs (stage by stage, as FREQ)
                    constexpr int P = kVcChunk / 2;
                    f2 t[P], dt[P];
#pragma unroll
                    for (int q = 0; q < P; ++q) {
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            port_z = freq + port_c * (port_z - freq);     // Port::Process (Portamento.h:218-221)
                            const float inc = port_z * inv_sr;             // Oscillator::SetFreq
                            t[q][h] = phase;                               // Oscillator::Process reads, then advances
                            dt[q][h] = inc;
                            phase += inc;
                            phase = phase > 1.0f ? phase - 1.0f : phase;
                        }
                    }
                    f2 num[P], qv[P], qq[P], rlo[P], rhi[P], o[P];
                    bool lo[P][2], hi[P][2];
#pragma unroll
                    for (int q = 0; q < P; ++q) {
                        const f2 one_m = 1.0f - dt[q];
                        const f2 tm1 = t[q] - 1.0f;
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            lo[q][h] = t[q][h] < dt[q][h];
                            hi[q][h] = t[q][h] > one_m[h];          // (lo wins the selects below)
                            num[q][h] = lo[q][h] ? t[q][h] : tm1[h];
                        }
                    }
#pragma unroll
                    for (int q = 0; q < P; ++q)
                        qv[q] = num[q] * (f2){__builtin_amdgcn_rcpf(dt[q].x), __builtin_amdgcn_rcpf(dt[q].y)};
                    // q + q - q q - 1 and q q + q + q + 1 as fma(-q, q, 2q) - 1 and fma(q, q, 2q) + 1
#pragma unroll
                    for (int q = 0; q < P; ++q) qq[q] = qv[q] + qv[q];
#pragma unroll
                    for (int q = 0; q < P; ++q) {
                        rlo[q] = __builtin_elementwise_fma(-qv[q], qv[q], qq[q]);
                        rhi[q] = __builtin_elementwise_fma(qv[q], qv[q], qq[q]);
                    }
#pragma unroll
                    for (int q = 0; q < P; ++q) { rlo[q] = rlo[q] - 1.0f; rhi[q] = rhi[q] + 1.0f; o[q] = 0.5f - t[q]; }
#pragma unroll
                    for (int q = 0; q < P; ++q) {
                        f2 blep;
#pragma unroll
                        for (int h = 0; h < 2; ++h) blep[h] = lo[q][h] ? rlo[q][h] : (hi[q][h] ? rhi[q][h] : 0.0f);
                        // -((2t - 1) - blep) / 2 as fma(1/2, blep, 1/2 - t): 2t - 1 = 2 (t - 1/2) and the
                        // halving are exact, so both round the same sum once (saw_out below)
                        const f2 y = __builtin_elementwise_fma((f2)0.5f, blep, o[q]);
                        qo[(2 * q) * 64] = y.x;
                        qo[(2 * q + 1) * 64] = y.y;
                    }
                } else {
                    for (uint32_t j = 0; j < m; ++j) {
                        port_z = freq + port_c * (port_z - freq);
                        const float inc = port_z * inv_sr;
                        const float t = phase;
                        phase += inc;
                        phase = phase > 1.0f ? phase - 1.0f : phase;
                        qo[j * 64] = saw_out(t, polyblep(inc, t));
                    }
                }
                cu.next();
            }
            __syncthreads();
        }
        if constexpr (SEG)
            if (fset) s[VCS_FREQ * n + i] = freq;         // the last segment's
        s[VCS_PHASE * n + i] = phase;
        s[VCS_PORT_Z * n + i] = port_z;
    } else if (role == 2) {
        voice_role_freq<SEG>(a, v, eq, fdq, sg);
    } else {
        // chunk c's source samples: sq[c & 1], 64 floats apart
        voice_role_filt<64, SEG>(a, v, eq, fdq, [&](uint32_t c2) { return &sq[c2 & 1][0][lane]; }, sg);
    }
}
__global__ __launch_bounds__(256) void voice_block_v5(VoiceArgs a) { voice_v5<false>(a); }
__global__ __launch_bounds__(256) void voice_block_v5_seg(VoiceArgs a) { voice_v5<true>(a); }

hipError_t launch_voice(const VoiceArgs &a, hipStream_t s) {
    if (a.n == 0 || a.n_frames == 0) return hipSuccess;
    if ((uint64_t)kVcChunk * a.n * 4u > 0xFFFFFFFFull) return hipErrorInvalidValue;   // v5's chunk output resource
    const dim3 grid((a.n + 63) / 64);     // 64 voices per workgroup, one wave per role
    if (a.n_seg > 1) {                    // timed events: the segmented kernels
        if (a.n_seg > kSegCap || !a.seg || !a.ev) return hipErrorInvalidValue;
        if (a.moog) hipLaunchKernelGGL(voice_block_v4_seg, grid, dim3(128), 0, s, a);
        else hipLaunchKernelGGL(voice_block_v5_seg, grid, dim3(256), 0, s, a);
        return hipGetLastError();
    }
    if (a.moog) hipLaunchKernelGGL(voice_block_v4, grid, dim3(128), 0, s, a);
    else hipLaunchKernelGGL(voice_block_v5, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace olfx
