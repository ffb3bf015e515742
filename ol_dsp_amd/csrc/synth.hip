// ol_dsp_amd/csrc/synth.hip -- a whole polyphonic instrument (voices, Polyvoice sum, effect rack) in
// one launch, gfx950, wave64.  One kernel template over the voice type, synth_block<SVF, SEG>, whose
// instantiations go by the names olfx_kernel_name reports (SEG: the same name with _seg, the launch of a block
// with timed notes inside it):
//
// synth_block_v1 = synth_block<false, false> (OLFX_KIND_SYNTH): the Daisy synth firmware's audio callback
// (ol_daisy/app/synth/main.cpp:78-86):
//
//   mono = 0; voice.Process(&mono);       Polyvoice over P x SynthVoice(OscillatorSoundSource, MoogFilter)
//   delay_fx.Process(&mono, &mono);       DelayFx<1>
//   stereo[0] = stereo[1] = mono;
//   reverb_fx.Process(stereo, stereo);    ReverbFx<2> over the ReverbSc stub
//   filter_fx.Process(stereo, stereo);    FilterFx<2> in place
//
// Per frame and instrument, every operation in fp32:
//   v[p]  = voice p: voice_block_v4's arithmetic, operation for operation (moog_voice.h)
//   mono  = 0.0f; mono += v[0]; ... mono += v[P-1]         Polyvoice.h:28-33, in that order from +0.0f
//   a     = DelayFx<1>::Process(mono)                       rack_delay_stage.h (fr::delay_stage_from)
//   b     = (a 0.8) balance + a (1 - balance)               ReverbFx over the stub, both channels equal
//   out 0 = FilterFx's Svf on b, out 1 = b                  (x 1.0f: the rack's topology 1 has no master)
// which is what voice_block_v4 + voice_mix + fxrack_block_v3 at OLFX_FR_TOPOLOGY 1 compute in three
// launches, bit for bit; the voice samples and the sum stay in LDS.
//
// synth_svf_block_v1 = synth_block<true, false> (OLFX_KIND_SYNTH_SVF): the library's own voice, SynthVoice(OscillatorSoundSource,
// SvfFilter), behind the same Polyvoice, into the rack at the instrument's topology:
//   v[p]  = voice p: voice_block_v5's arithmetic, operation for operation (svf_voice.h)
//   topology 1: as above
//   topology 0: FxRack<2>::Process (Fx.h:432-440) on the frame (mono, 0.0f): DelayFx<2> -> ReverbFx<2> ->
//               filter1 into the zeroed buf_c -> x master: out 0 = c0 master, out 1 = 0.0f master
// which is voice_block_v5 + voice_mix + fxrack_block_v3 with the sum in input channel 0 and zeros in
// channel 1.  The topology is per instrument: D and F select per lane (FRC_TOPO), so one wave may hold
// both.  (Channel 1's delay line reaches no output at either topology.)
//
// The seven-wave pipeline (roles, queues, counters, waits) is synth_pipeline.h's; here are the two voices and
// Polyvoice's sum.  The Svf voice keeps the pipeline's mapping although it is about a quarter of the Moog
// voice's work: a wave64 VALU instruction issues over four cycles, so a lane's dependent chain leaves no bubble
// to fill with a second wave, and a SIMD's time is its instruction total, which one voice per wave over eight
// waves would not change; eleven waves per workgroup would cap the kernel at 168 VGPRs where D needs more
// ("Svf synth").
// LDS: 63,040 B per workgroup at P = 4, 95,808 B at 8.
// Bound: the voice waves' per-sample recurrence, one wave per SIMD ("Synth"); the
// Svf synth: the D role's chunk chain for P <= 4, the voice wave that runs two voices from P = 5 on
// (measured, "Svf synth").
#include "synth_pipeline.h"
#include "svf_voice.h"

namespace olfx {

namespace {
constexpr uint32_t kSyMaxVoices = 8;
static_assert(sy::lds_floats(4, 0) * 4 == 63040 && sy::lds_floats(8, 0) * 4 == 95808, "LDS per workgroup");
static_assert(sy::lds_floats(kSyMaxVoices, 0) * 4 < 160 * 1024, "LDS budget");

// One MoogFilter SynthVoice of this lane: voice_block_v4's feed and ladder roles in one lane.
struct SyVoice : VoiceEnvs {
    float phase, port_z, freq;
    Ladder L;
    bool set_freq;
};
// One SvfFilter SynthVoice of this lane: voice_block_v5's four roles in one lane.
struct SySvfVoice : VoiceEnvs {
    float phase, port_z, freq;
    float low, band;
    bool set_freq;
};
}  // namespace

// SVF: SvfFilter voices and the rack's topology per instrument, 0 or 1 (synth_svf_block_v1); else
// MoogFilter voices and topology 1 (synth_block_v1).
// SEG (synth_block_v1_seg, synth_svf_block_v1_seg; olfx_timed_notes): the launch's frames are a.n_seg segments
// with note events of their own; the V waves split their chunks at the segment starts (sy::role_v), D and F are
// the same code.  The per-sample voice functions make the pieces bit-exact with a launch per segment.
// TP (synth_block_v1_seg_tp, synth_svf_block_v1_seg_tp; a.tp; olfx_timed_instrument_params; a SEG launch whose packet
// has timed records -- one without runs the SEG kernel as it was): the voice coefficients are loop-carried -- at a
// segment start a lane whose instrument has a voice record there takes amp_amt .. K (and kc) from it, ahead of the
// segment's events, and remembers the record: voice_envs_restart reads the envelope words of the instrument's
// latest record, the device array's until the first.  The kernels never write the coefficient arrays.  F takes
// the rack records (sy::role_f).
template <bool SVF, bool SEG, bool TP = false>
__global__ __launch_bounds__(sy::kThreads) void synth_block(std::conditional_t<TP, SynthSegArgs, SynthArgs> a) {
    static_assert(SEG || !TP, "timed records come with segments");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const sy::Wg b = sy::enter(a, lds);
    const uint32_t n = b.n, P = b.P;

    if (sy::is_v(b)) {
        const uint32_t i = sy::v_instrument(b);
        const uint32_t sn = P * a.npad;                    // voice slots: the state planes' stride
        const float *c = a.vc_coef;                        // the instrument's: shared by its voices
        float *s = a.vc_state;

        // (SEG: loop-carried -- a segment with a voice record replaces them)
        float amp_amt = c[VCC_AMP_AMT * n + i], port_c = c[VCC_PORT_COEF * n + i];
        float inv_sr = c[VCC_INV_SR * n + i];
        float cutoff = c[VCC_CUTOFF * n + i], fenv_amt = c[VCC_FENV_AMT * n + i];
        float drive = c[VCC_DRIVE * n + i], fc_max = c[VCC_FC_MAX * n + i];
        float K = c[VCC_LADDER_K * n + i];                 // the Svf voice: VCC_DAMP_RES (the same word)
        SvfVoiceCoef kc{};
        if constexpr (SVF)                                 // as voice_role_env / voice_role_freq form them
            kc = SvfVoiceCoef{0.5f * amp_amt, port_c, inv_sr, cutoff, fenv_amt, fc_max, drive, K,
                              1.0f / (c[VCC_SR * n + i] * 2.0f)};

        using V = std::conditional_t<SVF, SySvfVoice, SyVoice>;
        auto load = [&](V &v, uint32_t p) {
            const uint32_t si = p * a.npad + i;
            const float freq_s = s[VCS_FREQ * sn + si];
            const VoiceEv ev = voice_envs_load(v, s, sn, si, c, n, i, a.ev, a.ev_more, b.evslots + b.wib * 64u, b.lane,
                                               i - b.g * 64u, p * (a.npad >> 6) + b.g);
            v.set_freq = (ev.op & VEV_FREQ) != 0u;
            v.freq = v.set_freq ? ev.freq : freq_s;
            v.phase = s[VCS_PHASE * sn + si];
            v.port_z = s[VCS_PORT_Z * sn + si];
            if constexpr (SVF) {
                v.low = s[VCS_LOW * sn + si];
                v.band = s[VCS_BAND * sn + si];
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    v.L.z0[k] = s[(VCS_LZ0 + k) * sn + si];
                    v.L.z1[k] = s[(VCS_LZ1 + k) * sn + si];
                }
                v.L.old = s[VCS_LOLD * sn + si];
            }
        };
        auto store = [&](const V &v, uint32_t p) {
            const uint32_t si = p * a.npad + i;
            s[VCS_PHASE * sn + si] = v.phase;
            s[VCS_PORT_Z * sn + si] = v.port_z;
            voice_envs_store(v, s, sn, si);
            if (v.set_freq) s[VCS_FREQ * sn + si] = v.freq;
            if constexpr (SVF) {
                s[VCS_LOW * sn + si] = v.low;
                s[VCS_BAND * sn + si] = v.band;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    s[(VCS_LZ0 + k) * sn + si] = v.L.z0[k];
                    s[(VCS_LZ1 + k) * sn + si] = v.L.z1[k];
                }
                s[VCS_LOLD * sn + si] = v.L.old;
            }
        };
        auto run = [&](V &v, float *q, uint32_t m) {
            auto tick = [&](uint32_t k) {
                if constexpr (SVF) {
                    q[k * 64u] = svf_voice_tick(v.ea, v.ef, v.port_z, v.phase, v.low, v.band, v.freq, kc);
                } else {
                    const float2 ab = moog_amp_tick(v.ea, v.port_z, v.phase, v.freq, amp_amt, port_c, inv_sr, drive);
                    const float2 cd = moog_cut_tick(v.ef, fenv_amt, cutoff, fc_max);
                    q[k * 64u] = ladder_tick(v.L, make_float4(ab.x, ab.y, cd.x, cd.y), K);
                }
            };
            if (m == (uint32_t)sy::kChunk) {
#pragma unroll 4
                for (uint32_t k = 0; k < (uint32_t)sy::kChunk; ++k) tick(k);
            } else {
                for (uint32_t k = 0; k < m; ++k) tick(k);
            }
        };
        if constexpr (SEG && !TP) {
            // a segment's events on the live voice: the gate and the envelopes, and NoteOn's pitch
            auto start = [&](V &v, uint32_t, const VoiceEv &ev) {
                voice_envs_restart(v, ev, c, n, i);
                if (ev.op & VEV_FREQ) {
                    v.freq = ev.freq;
                    v.set_freq = true;
                }
            };
            sy::role_v<V, true>(b, load, run, store, &a, start);
        } else if constexpr (TP) {
            // ... and ahead of them the instrument's voice record of the segment, if it has one
            // (both voices of a wave get the instrument's record: the second reload repeats the first)
            uint32_t crec = kNoCoef;                       // the instrument's latest voice record of this launch
            auto start = [&](V &v, uint32_t, const VoiceEv &ev, uint32_t r) {
                const float *t = a.tp.vrec;
                const uint32_t T = a.tp.n_v;
                if (r != kNoCoef) {
                    crec = r;
                    amp_amt = t[VCC_AMP_AMT * T + r], port_c = t[VCC_PORT_COEF * T + r];
                    inv_sr = t[VCC_INV_SR * T + r];
                    cutoff = t[VCC_CUTOFF * T + r], fenv_amt = t[VCC_FENV_AMT * T + r];
                    drive = t[VCC_DRIVE * T + r], fc_max = t[VCC_FC_MAX * T + r];
                    K = t[VCC_LADDER_K * T + r];
                    if constexpr (SVF)
                        kc = SvfVoiceCoef{0.5f * amp_amt, port_c, inv_sr, cutoff, fenv_amt, fc_max, drive, K,
                                          1.0f / (t[VCC_SR * T + r] * 2.0f)};
                }
                const bool rec = crec != kNoCoef;
                voice_envs_restart(v, ev, rec ? t : c, rec ? T : n, rec ? crec : i);
                if (ev.op & VEV_FREQ) {
                    v.freq = ev.freq;
                    v.set_freq = true;
                }
            };
            sy::role_v<V, true, true>(b, load, run, store, &a, start, &a.tp);
        } else {
            sy::role_v<V>(b, load, run, store);
        }
    } else if (sy::is_d(b)) {
        // Polyvoice::Process: mono = 0; mono += v[0]; ... mono += v[P-1]
        sy::role_d<SVF>(b, a, [&](const float *q, float (&m)[sy::kChunk]) {
            for (uint32_t p = 0; p < P; ++p) {
#pragma unroll
                for (int k = 0; k < sy::kChunk; ++k) m[k] += q[p * sy::kQ + k * 64];
            }
        });
    } else {
        sy::role_f<SVF, TP>(b, a, [&]() -> const InstrumentTimed * {
            if constexpr (TP) return &a.tp;
            else return nullptr;
        }());
    }
}

hipError_t launch_synth(const SynthSegArgs &a, hipStream_t s) {
    if (a.n == 0 || a.n_frames == 0) return hipSuccess;
    if (!instrument_args_ok(a, kSyMaxVoices) || !instrument_timed_ok(a, a.tp, false)) return hipErrorInvalidValue;
    if (a.tp.vtab) return sy::launch(a.svf ? synth_block<true, true, true> : synth_block<false, true, true>, a, 0, s);
    const SynthArgs &plain = a;                            // (the other kernels take the arguments they always took)
    if (a.n_seg > 1u) return sy::launch(a.svf ? synth_block<true, true> : synth_block<false, true>, plain, 0, s);
    return sy::launch(a.svf ? synth_block<true, false> : synth_block<false, false>, plain, 0, s);
}

}  // namespace olfx
