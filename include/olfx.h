/*
 * include/olfx.h -- C-ABI of the MI355X bulk audio-effect engine (libolfx.so).
 *
 * One engine = one effect kind x N independent instances on one GPU.  Every call processes a
 * block of frames for ALL instances at once on a HIP stream; per-instance parameters and note
 * events are applied at the next block boundary (the JUCE-host pattern, reference
 * modules/juce/host/host.cpp:646-653).  No torch types, plain pointers and sizes only.
 *
 * What each entry point replaces in the reference (/root/reference):
 *   olfx_create / olfx_destroy  <- DattorroVerb_create / _delete (libs/dattorro-verb/verb.h:5-8,
 *                                  verb.cpp:225-251); fxlib XxxFx::Init(sr) (modules/fxlib/Fx.h:183,
 *                                  :290); SynthVoice::Init(sr) (modules/synthlib/SynthVoice.h:31-39);
 *                                  README ChorusEffect::init(sr) (README.md:117-127)
 *   olfx_set_params             <- DattorroVerb_set* (verb.h:10-16, verb.cpp:137-170);
 *                                  ChorusEffect::setDepth/setRate (README.md:120-121) and the RNBO
 *                                  chorus params (modules/rnbo/patcher/mono-chorus.rnbopat:431-4353);
 *                                  SynthVoice::UpdateConfig/Update (SynthVoice.h:55-98)
 *   olfx_note_events            <- SynthVoice::NoteOn/NoteOff (SynthVoice.h:245-256)
 *   olfx_process                <- the per-frame loops DattorroVerb_process + getLeft/getRight
 *                                  (verb.cpp:258-325), ReverbFx glue (modules/fxlib/ReverbFx.cpp:11-27),
 *                                  ChorusEffect::process(sample) (README.md:124), SynthVoice::Process
 *                                  (SynthVoice.h:41-53) -- batched: n_frames x n_inst per call
 *   olfx_mix_config / olfx_mix  <- Polyvoice::Process (modules/synthlib/Polyvoice.h:28-33) and
 *                                  VoiceMap::Process (VoiceMap.h:64-73): voices added into one
 *                                  frame, voice by voice
 *   olfx_sample_bank / olfx_sample_voices <- ol::synth::Sample over its data source and its setters
 *                                  (modules/synthlib/Sample.h:16-51, Sample.cpp:9-62) behind
 *                                  SampleSoundSource<1> (SampleSoundSource.h:13-40)
 *   OLFX_KIND_SYNTH             <- the Daisy synth firmware as a whole (modules/ol_daisy/app/synth/main.cpp):
 *                                  its globals (:49-67: four SynthVoices behind a Polyvoice, delay_fx,
 *                                  reverb_fx, filter_fx) are one instrument, its audio callback (:78-86) one
 *                                  olfx_process, handleMidi (:187-214) olfx_note_events and olfx_control
 *   olfx_last_error             <- (reference has none: void returns / NULL, verb.cpp:89-90,227)
 *
 * Audio layout (both host and device pointers accepted, see OLFX_IO_*):
 *   in  : [in_channels ][n_frames][n_inst]  float32, instance index fastest
 *   out : [out_channels][n_frames][n_inst]  float32
 * Channel counts per kind are given by olfx_kind_info().
 *
 * Errors: every function returns 0 on success or a negative OLFX_E_* code; no C++ exception
 * crosses this boundary.  An engine is not re-entrant: one host thread drives one engine.
 */
#ifndef OLFX_H
#define OLFX_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OLFX_ABI_VERSION 2

/* ---- status codes ---- */
enum {
    OLFX_OK          = 0,
    OLFX_E_ARG       = -1,   /* bad argument (null, out of range, wrong size) */
    OLFX_E_NOMEM     = -2,   /* host or device allocation failed */
    OLFX_E_HIP       = -3,   /* a HIP runtime call failed; see olfx_last_error */
    OLFX_E_NODEVICE  = -4,   /* no GPU / device index invalid */
    OLFX_E_KIND      = -5,   /* unknown effect kind */
    OLFX_E_STATE     = -6    /* call not valid in the engine's current state */
};

/* ---- effect kinds ---- */
enum {
    OLFX_KIND_DATTORRO   = 1,  /* libs/dattorro-verb: stereo in -> (l+r)/2 -> stereo out (ReverbFx.cpp:11-27),
                                  or mono in (verb.h:19) */
    OLFX_KIND_CHORUS     = 2,  /* RNBO stereo-chorus (mono-chorus x2, shared params) */
    OLFX_KIND_PITCHSHIFT = 3,  /* gen~ pitchshift, stereo */
    OLFX_KIND_VOICE      = 4,  /* synthlib SynthVoice: polyBLEP saw -> SVF LP (env cutoff) -> amp env; mono out */
    OLFX_KIND_CHAIN      = 5,  /* fused chorus -> pitch-shift -> dattorro, stereo */
    OLFX_KIND_FXRACK     = 6,  /* fxlib ol::fx::FxRack<2>: delay -> reverb -> filter -> master (Fx.h:398-492) */
    OLFX_KIND_VOICE_MOOG = 7,  /* SynthVoice(OscillatorSoundSource, MoogFilter): the Daisy synth firmware voice
                                  (ol_daisy/app/synth/main.cpp:49-52); daisysp::LadderFilter LP24 in place of the
                                  SVF (Filter.h:35-63).  Same OLFX_VC_* parameters (FILTER_DRIVE is ignored:
                                  MoogFilter::SetDrive is a no-op), note events and control changes. */
    OLFX_KIND_PLATERACK  = 8,  /* the effect rack with the Dattorro plate as its reverb stage: DelayFx<2> ->
                                  Dattorro((a0 + a1) / 2) mixed by REVERB_BALANCE -> FilterFx<2> -> master, one
                                  launch (platerack.hip).  The stage the reference's rack was written for: its
                                  ol::fx::Reverb interface (Reverb.h:44-65) is the DattorroVerb_set* list and
                                  ReverbFx.cpp:11-37 still holds the glue, commented out.  OLFX_PR_* fields. */
    /* 9 stays unassigned: tests/test_platerack_host.py pins it as "a kind nobody has" (OLFX_E_KIND) */
    OLFX_KIND_VOICE_SAMPLE = 10, /* SynthVoice(SampleSoundSource<1>(Sample), SvfFilter): sample playback from a
                                  device-resident bank (olfx_sample_bank / olfx_sample_voices) -> SVF LP -> amp
                                  env; mono out, no input.  OLFX_VC_* parameters, note events, control changes,
                                  olfx_set_member, olfx_update and the voice buses as OLFX_KIND_VOICE.  GateOn /
                                  NoteOn also Seek(0) and Play() the sample, GateOff / NoteOff Pause() it
                                  (SampleSoundSource.h:21-26); SetFreq only stores the pitch (:28-30). */
    OLFX_KIND_SYNTH = 11,      /* the Daisy synth firmware's audio callback (ol_daisy/app/synth/main.cpp:78-86) in
                                  one launch (synth.hip): per instrument, P MoogFilter SynthVoices behind a
                                  Polyvoice (mono = 0; mono += v[0]; ... += v[P-1]) -> DelayFx<1> -> stereo copy
                                  -> ReverbFx<2> over the ReverbSc stub -> FilterFx<2> in place.  No input;
                                  out [2][n_frames][n_inst]: channel 0 is filter_fx's output, channel 1 the
                                  reverb's channel 1, which FilterFx<2> leaves in place -- bit for bit what
                                  OLFX_KIND_VOICE_MOOG + olfx_mix + OLFX_KIND_FXRACK at OLFX_FR_TOPOLOGY 1 give
                                  for the sum in input channel 0.  P = 4 (olfx_create) or 1..8
                                  (olfx_create_synth).  OLFX_SY_* fields and rules below. */
    OLFX_KIND_SYNTH_SVF = 12,  /* the library's own voice as a polyphonic instrument, one launch (synth.hip):
                                  per instrument, P SynthVoice(OscillatorSoundSource, SvfFilter) -- the default-
                                  constructed SynthVoice, OLFX_KIND_VOICE's -- behind a Polyvoice, into the rack
                                  at the instrument's OLFX_FR_TOPOLOGY: 1 as OLFX_KIND_SYNTH, or 0,
                                  FxRack<2>::Process (Fx.h:432-440) with its master volume on the frame
                                  (mono, 0.0f), the path SynthEngine::Process (app/synth/SynthEngine.h:24-32)
                                  hands the voice sum to.  No input; out [2][n_frames][n_inst] -- bit for bit what
                                  OLFX_KIND_VOICE + olfx_mix + OLFX_KIND_FXRACK at that topology give for the sum
                                  in input channel 0 and zeros in channel 1.  P = 4 (olfx_create) or 1..8
                                  (olfx_create_synth_kind).  OLFX_SY_* fields; rules below. */
    /* 13 stays unassigned: tests/cpp/dump_kinds.cpp (tests/golden/host_kinds.txt), tests/cpp/test_synth_svf_host.cpp
       and tests/test_synth_svf_host.py pin it as "a kind nobody has" (OLFX_E_KIND) */
    OLFX_KIND_DRUMKIT = 14,    /* the reference's drum machine, one launch (drumkit.hip): per kit, P sample voices
                                  (SynthVoice(SampleSoundSource<1>(Sample), SvfFilter), OLFX_KIND_VOICE_SAMPLE's, each
                                  with its own Voice::Config and Sample) behind a VoiceMap (VoiceMap.h:27-82), into
                                  the rack at the kit's OLFX_FR_TOPOLOGY, 0 or 1 as OLFX_KIND_SYNTH_SVF:
                                    frame = 0; voicemap.Process(&frame);   for note 0..127 ascending, if a voice sits
                                                                           there: frame += voice.Process()
                                    rack on (frame, 0.0f)
                                  No input; out [2][n_frames][n_kits] -- bit for bit what OLFX_KIND_VOICE_SAMPLE over
                                  the kit's voices + olfx_mix with one bus per kit listing its mapped voices in
                                  ascending note order + OLFX_KIND_FXRACK at that topology give for the sum in input
                                  channel 0 and zeros in channel 1.  P = 4 (olfx_create) or 1..8 (olfx_create_drumkit).
                                  OLFX_DK_* fields, olfx_drumkit_map; rules below. */
    OLFX_KIND_METER = 15,      /* a level meter on the device (meter.hip): per signal -- one channel of one instance
                                  -- ol::core::Rms (corelib/ol_corelib.h:61-85) paired with the peak-hold follower of
                                  its one caller, the sandbox firmware's callback (ol_daisy/workouts/sandbox/
                                  main.cpp:98-137).  In [2][n_frames][n_inst], the effect and instrument kinds' output;
                                  the two channels are independent signals.  out [2][n_frames][n_inst] = the value
                                  Rms::Process returns at each frame, or NULL: levels only (olfx_meter_read).
                                  OLFX_MT_* fields; rules below. */
    OLFX_KIND_METER_MONO = 16  /* the same over [n_frames][n_inst]: the voice kinds' output, or olfx_mix's buses */
};

/* ---- parameters (field index, value is what the reference setter takes) ---- */
/* Dattorro: verb.h:10-16 */
enum {
    OLFX_DT_PREDELAY = 0,        /* setPreDelay: [0,1] x 4800 samples, per instance */
    OLFX_DT_PREFILTER,           /* setPreFilter */
    OLFX_DT_INPUT_DIFFUSION1,    /* setInputDiffusion1 */
    OLFX_DT_INPUT_DIFFUSION2,    /* setInputDiffusion2 */
    OLFX_DT_DECAY_DIFFUSION,     /* setDecayDiffusion */
    OLFX_DT_DECAY,               /* setDecay (also derives decay diffusion 2, verb.cpp:164) */
    OLFX_DT_DAMPING,             /* setDamping */
    OLFX_DT_NPARAMS
};
/* Chorus (RNBO params, clamped to @min/@max like RNBO; mono-chorus.rnbopat line of each param) */
enum {
    OLFX_CH_PITCH = 0,   /* [0,3]      default 0    :431   pitch-shifter phasor rate, Hz */
    OLFX_CH_MIX,         /* [0,1]      default 0.5  :1772 */
    OLFX_CH_Q,           /* [0,1]      default 0.5  :2226  lores~ resonance */
    OLFX_CH_CUTOFF,      /* [0,1]      default 0.3  :2660  -> 300..15000 Hz (:2242) */
    OLFX_CH_PHASE,       /* [0,1]      default 1    :3420  cycle~ phase offset */
    OLFX_CH_DEPTH,       /* [0.08,1]   default 0.5  :3854  -> 1..12 ms (:3436) */
    OLFX_CH_RATE,        /* [0.01,1]   default 0.2  :4353  -> 0.01..0.5 Hz (:3935) */
    OLFX_CH_WINDOW,      /* [4,10] ms  default 10   pitchshift.gendsp "Param window" */
    OLFX_CH_NPARAMS
};
/* Pitch-shift stage (gen~ pitchshift.gendsp) */
enum {
    OLFX_PS_SHIFT = 0,   /* [0,3] Hz phasor rate (inlet 2 of pitchshift.gendsp) */
    OLFX_PS_WINDOW,      /* [4,10] ms */
    OLFX_PS_NPARAMS
};
/* Voice: Voice::Config field order (modules/synthlib/Voice.h:14-31) */
enum {
    OLFX_VC_FILTER_CUTOFF = 0, OLFX_VC_FILTER_RESONANCE, OLFX_VC_FILTER_DRIVE, OLFX_VC_FILTER_ENV_AMOUNT,
    OLFX_VC_FILTER_ATTACK, OLFX_VC_FILTER_ATTACK_SHAPE, OLFX_VC_FILTER_DECAY, OLFX_VC_FILTER_SUSTAIN,
    OLFX_VC_FILTER_RELEASE, OLFX_VC_AMP_ENV_AMOUNT, OLFX_VC_AMP_ATTACK, OLFX_VC_AMP_ATTACK_SHAPE,
    OLFX_VC_AMP_DECAY, OLFX_VC_AMP_SUSTAIN, OLFX_VC_AMP_RELEASE, OLFX_VC_PORTAMENTO,
    OLFX_VC_NPARAMS
};
/* Effect rack: ol::fx::FxRack<2> members (modules/fxlib/Fx.h; defaults in brackets) */
enum {
    OLFX_FR_DELAY_TIME = 0,      /* DelayFx time [0,1] -> 0..48000 samples            [0.5]   Fx.h:172,214 */
    OLFX_FR_DELAY_FEEDBACK,      /* DelayFx feedback                                   [0.5]   Fx.h:173 */
    OLFX_FR_DELAY_BALANCE,       /* DelayFx wet/dry                                    [0.33]  Fx.h:174 */
    OLFX_FR_DELAY_CUTOFF,        /* DelayFx filter_ cutoff, Hz              [scale(64,0,127,0,20000)] :188 */
    OLFX_FR_DELAY_RESONANCE,     /* DelayFx filter_ resonance [0,1]            [scale(24,0,127,0,1)] :189 */
    OLFX_FR_REVERB_BALANCE,      /* ReverbFx balance (over the ReverbSc stub)   [0.1]   Fx.h:282 */
    OLFX_FR_FILTER_CUTOFF,       /* FxRack filter1 cutoff, Hz                  [20000]  Fx.h:75 */
    OLFX_FR_FILTER_RESONANCE,    /* [0] */
    OLFX_FR_FILTER_DRIVE,        /* [0] */
    OLFX_FR_FILTER_TYPE,         /* 0 low, 1 band, 2 high, 3 notch, 4 peak      [0]     Fx.h:67-73 */
    OLFX_FR_MASTER_VOLUME,       /* [0.8] Fx.h:405 */
    OLFX_FR_TOPOLOGY,            /* [0] 0: FxRack<2>::Process (Fx.h:432-440): delay -> reverb -> filter1 into the
                                    zeroed buf_c -> x master (output channel 1 is 0).
                                    1: the Daisy synth firmware's audio callback (ol_daisy/app/synth/main.cpp:
                                    78-86): DelayFx<1> on channel 0 -> stereo[0] = stereo[1] -> ReverbFx<2>
                                    -> FilterFx<2> in place (channel 1 keeps the reverb's output), no master
                                    volume (MASTER_VOLUME ignored).  Input: the mono signal in channel 0.
                                    Controls (olfx_control) follow the firmware too (main.cpp:201-207): the
                                    voice-filter CCs 41-44 drive FILTER_*, CCs 45-48 and 7 are ignored.
                                    2, 3, 4: one component alone, as the firmware's objects (main.cpp:82-85):
                                    2 DelayFx<2>::Process (Fx.h:193-206; DELAY_* fields; channel 0 filtered
                                      by its filter_, channel 1 not; DelayFx<1> = channel 0);
                                    3 ReverbFx<2>::Process over the ReverbSc stub (Fx.h:293-299; REVERB_BALANCE):
                                      per channel 0.8 in balance + in (1 - balance);
                                    4 FilterFx<2>::Process (Fx.h:88-108; FILTER_*): the Svf on channel 0, and
                                      channel 1 passes through (the reference leaves frame_out[1] unwritten:
                                      in place, as the firmware calls it, that is channel 1 of the input).
                                    olfx_control gives each its own controls only (DelayFx 35-39, ReverbFx 34,
                                    FilterFx 41-44).  One engine may mix every topology. */
    OLFX_FR_NPARAMS
};
/* Chain: chorus params, then pitch-shift params, then dattorro params */
#define OLFX_CN_CHORUS0   0
#define OLFX_CN_PITCH0    (OLFX_CH_NPARAMS)
#define OLFX_CN_VERB0     (OLFX_CH_NPARAMS + OLFX_PS_NPARAMS)
#define OLFX_CN_NPARAMS   (OLFX_CH_NPARAMS + OLFX_PS_NPARAMS + OLFX_DT_NPARAMS)

/* Plate rack: the rack's fields (OLFX_FR_*), then the plate's (OLFX_DT_*, what the verb.h setters take,
   validated as OLFX_KIND_DATTORRO validates them; a pre-delay change lands at the next block boundary).
   OLFX_FR_TOPOLOGY is 0 (FxRack<2>::Process) or 1 (the firmware callback: DelayFx<1>, stereo[0] = stereo[1],
   the reverb, FilterFx<2> in place -- channel 1 keeps the plate's right output mixed with the dry signal --
   and no master volume); 2..4 are refused.
   Defaults.  Rack fields: as OLFX_KIND_FXRACK.  Plate fields: what ReverbFx::Init -> Update() would hand
   the plate through the glue of ReverbFx.cpp:29-37 wherever the ReverbFx member (Fx.h:274-281) lies in the
   setter's domain: decay_time 0.5 -> setDecay, pre_cutoff 0.5 -> setPreFilter, input_diffusion1 / 2 0.5,
   decay_diffusion 0.5.  The member `cutoff` is 12000, a frequency in Hz meant for ReverbSc::SetLpFreq and
   outside setDamping's [0, 1], and the glue never calls setPreDelay: DAMPING (0.95) and PREDELAY (0.1) keep
   DattorroVerb_create's own defaults (verb.cpp:215-221).
   Controls (olfx_control_map / olfx_control): ReverbFx::UpdateMidiControl / UpdateHardwareControl
   (Fx.h:313-391) composed with that glue: CC_REVERB_TIME -> DECAY, CC_REVERB_PREFILTER -> PREFILTER,
   CC_REVERB_INPUT_DIFFUSION_1 -> INPUT_DIFFUSION1, CC_REVERB_DECAY_DIFFUSION and (the reference's quirk,
   Fx.h:323-324, kept) CC_REVERB_INPUT_DIFFUSION_2 -> DECAY_DIFFUSION, CC_REVERB_BALANCE -> REVERB_BALANCE,
   CC_REVERB_CUTOFF -> DAMPING in the 0..1 form (`//cutoff = scaled`, Fx.h:328; the live Hz form addresses
   ReverbSc), CC_REVERB_PREDELAY and CC_EARLY_PREDELAY -> OLFX_FIELD_UPDATE_ONLY (the glue forwards
   neither).  MIDI values are scaled 0..1, hardware values taken as given.  Delay, filter and volume
   controls and the topology-1 routing: as OLFX_KIND_FXRACK. */
#define OLFX_PR_RACK0     0
#define OLFX_PR_VERB0     (OLFX_FR_NPARAMS)
#define OLFX_PR_NPARAMS   (OLFX_FR_NPARAMS + OLFX_DT_NPARAMS)

/* Synth (OLFX_KIND_SYNTH): the sixteen voice fields (OLFX_VC_*), then the rack's twelve (OLFX_FR_*).
     field                      meaning                                            default, validation
     OLFX_SY_VOICE0 + OLFX_VC_* the Voice::Config member of ALL voices of the      as OLFX_KIND_VOICE_MOOG
                                instrument (Polyvoice fans UpdateConfig, Update
                                and both control calls out to every voice,
                                Polyvoice.h:53-67)
     OLFX_SY_RACK0 + OLFX_FR_*  delay_fx / reverb_fx / filter_fx members           as OLFX_KIND_FXRACK, but
                                                                                   TOPOLOGY defaults to 1 and only
                                                                                   1 is accepted (else OLFX_E_ARG,
                                                                                   nothing changes); MASTER_VOLUME
                                                                                   is stored and ignored
   olfx_set_params / olfx_set_param / olfx_set_param_list / olfx_get_param work on the 28 fields; a write
   that touches a voice field is UpdateConfig + Update of every voice of the instrument.  olfx_set_member on
   a voice field is the voice kind's member-without-Update for all P voices (the firmware's set-up, main.cpp:
   114-128 before Init at :149-154); on a rack field it is olfx_set_param.  olfx_update is Polyvoice::Update.
   Note events (olfx_note_events / olfx_voice_events; `inst` is the instrument) are Polyvoice's calls
   (Polyvoice.h:35-77), routed on the host at the call and queued per voice for the next block boundary:
     NOTE_ON        the first voice with Playing() == 0 gets NoteOn; none free: the event is dropped
     NOTE_OFF       the first voice with Playing() == note gets NoteOff
     GATE_ON / OFF  every voice
     SET_FREQUENCY  accepted, does nothing (Polyvoice.h:77)
   Playing() is the last NoteOn's note and 0 after NoteOff (SynthVoice.h:245-260) and changes at the call;
   olfx_synth_playing reads it back; olfx_reset clears it.  The reference's quirks are kept: NoteOn(0) gates
   a voice whose Playing() stays 0, so the voice stays "free" and the next NoteOn takes it again; NoteOff(0)
   hits the first free voice (Playing() == 0 == note) and gates it off.
   Controls: olfx_control on an instrument is the firmware's handleMidi (main.cpp:201-207): the event goes
   in turn to the voices (SynthVoice's mapping, every voice), delay_fx, reverb_fx and filter_fx (the rack's
   topology-1 mapping), so CCs 41-44 move both the voice filter and FILTER_*; hardware-source events follow
   the same route through the UpdateHardwareControl handlers.  olfx_synth_control_map gives the fields hit;
   olfx_control_map(OLFX_KIND_SYNTH, ...) returns OLFX_E_KIND (it has one field to give).
   Refused on this kind, with the code each call uses for a wrong kind (OLFX_E_STATE): olfx_mix_config and
   olfx_mix (there are no buses: the sum never leaves the kernel), olfx_sample_bank, olfx_sample_voices.

   Svf synth (OLFX_KIND_SYNTH_SVF): the same 28 fields in the same layout and every rule above, except:
     OLFX_SY_VOICE0 + OLFX_VC_* defaults and validation as OLFX_KIND_VOICE; FILTER_DRIVE is live (SvfFilter::SetDrive)
     OLFX_SY_RACK0 + OLFX_FR_*  as OLFX_KIND_FXRACK, but TOPOLOGY defaults to 1 and accepts 0 or 1 (else
                                OLFX_E_ARG, nothing changes), per instrument -- one engine may mix both, and a
                                change lands at the next block boundary like every parameter change;
                                MASTER_VOLUME is live at topology 0, stored and ignored at topology 1
   Topology 0: DelayFx<2> -> ReverbFx<2> over the stub -> filter1 into the zeroed buf_c -> x master: out 0 =
   c0 * master, out 1 = 0.0f * master.  Channel 1's delay line reaches no output at either topology; its
   contents are unspecified.
   Controls: olfx_control sends the event to the voices (SynthVoice's mapping as OLFX_KIND_VOICE has it, every
   voice), then to the rack with the mapping olfx_control uses on an OLFX_KIND_FXRACK instance of the
   instrument's current topology: at 1 the firmware's direct routing (CCs 41-44 hit both filters), at 0
   FxRack::UpdateMidiControl / UpdateHardwareControl (CCs 45-48 drive FILTER_*, CC 7 the master volume).
   olfx_synth_control_map_at gives the fields hit; olfx_control_map(OLFX_KIND_SYNTH_SVF, ...) is OLFX_E_KIND. */
#define OLFX_SY_VOICE0    0
#define OLFX_SY_RACK0     (OLFX_VC_NPARAMS)
#define OLFX_SY_NPARAMS   (OLFX_VC_NPARAMS + OLFX_FR_NPARAMS)

/* Drum kit (OLFX_KIND_DRUMKIT): eight voice slots of sixteen fields each, then the rack's twelve -- 140 fields
   whatever the kit's voice count P.
     field                               meaning                                   default, validation
     OLFX_DK_VOICE0 + 16 p + OLFX_VC_*   voice slot p's own Voice::Config member   as OLFX_KIND_VOICE_SAMPLE
                                         (p = 0..7; every pad has its own sample,
                                         envelopes and filter: SamplePool.h:37-53).
                                         Slots p >= P are validated and stored like
                                         the rest and read by nothing, so one
                                         [140][n] draw fits every P
     OLFX_DK_RACK0 + OLFX_FR_*           the rack's members                        as OLFX_KIND_SYNTH_SVF: TOPOLOGY
                                                                                   defaults to 1, accepts 0 or 1
   olfx_set_params / olfx_set_param_list imply Update() of exactly the voice slots whose fields the call touches (and
   re-derive the rack when rack fields are touched); olfx_set_member stores a voice member without Update() (refused
   with OLFX_E_STATE once that slot is Update()d, except the members Process reads, as for the voice kinds);
   olfx_update(first, count) is Update() of every voice of those kits and of their racks.
   The map (olfx_drumkit_map) is VoiceMap's two tables per kit, note2voice[128] and channel2voice[16]; it starts
   empty, is configuration (olfx_reset keeps it, like bank and sample assignments) and takes effect in call order:
   note events queued earlier were routed by the old map, the next olfx_process sums by the new one.
   Two departures from VoiceMap, both consequences of the contract above:
     - a voice that sits at no note is not summed and gets no note events, but it still ticks (its envelopes and
       its Sample advance), as it does in the composed engines; the reference does not tick it;
     - a voice may sit at one note only: a call that would leave a voice at two notes is refused (the reference
       would tick such a voice twice per frame, which olfx_mix_config refuses too).
   Notes: olfx_note_events NOTE_ON(kit, note, vel) is SynthVoice::NoteOn(note, vel) of the voice at note2voice[note]
   (with the sample voice's Seek(0) and Play()), NOTE_OFF its NoteOff; a note nobody sits at is ignored
   (VoiceMap.h:27-43).  GATE_ON, GATE_OFF and SET_FREQUENCY are OLFX_E_ARG: VoiceMap has no such call.
   olfx_synth_playing / olfx_synth_voices work as for the synth kinds (a voice's Playing() is its last NoteOn's
   note, 0 after NoteOff; olfx_reset clears it).
   Controls: olfx_control_event.pad is the MIDI channel (this kind only).  Channel c < 16: the voice at
   channel2voice[c] gets OLFX_KIND_VOICE_SAMPLE's control mapping on its own fields OLFX_DK_VOICE0 + 16 p + ...,
   with Update() of that voice only (VoiceMap.h:75-82); an empty entry is ignored.  Channel OLFX_DK_CHANNEL_RACK:
   the rack's mapping at the kit's topology, as olfx_control has it for OLFX_KIND_SYNTH_SVF's rack.  Other channel
   values are ignored.  olfx_control_map(OLFX_KIND_DRUMKIT, ...) is OLFX_E_KIND (the mapping needs a channel): use
   OLFX_KIND_VOICE_SAMPLE's map and add 16 p.
   Samples: olfx_sample_bank as for OLFX_KIND_VOICE_SAMPLE; olfx_sample_voices takes inst = kit * P + p.
   Refused (OLFX_E_STATE): olfx_mix_config, olfx_mix (the sum never leaves the kernel). */
#define OLFX_DK_MAX_VOICES   8
#define OLFX_DK_VOICE0       0
#define OLFX_DK_RACK0        (OLFX_DK_MAX_VOICES * OLFX_VC_NPARAMS)
#define OLFX_DK_NPARAMS      (OLFX_DK_RACK0 + OLFX_FR_NPARAMS)
#define OLFX_DK_NO_VOICE     0xFFFFFFFFu   /* olfx_drumkit_voice.voice: clear the entries (SetVoice(.., nullptr)) */
#define OLFX_DK_NO_NOTE      0xFFu         /* olfx_drumkit_voice.note: leave note2voice alone (an extension) */
#define OLFX_DK_NO_CHANNEL   0xFFu         /* olfx_drumkit_voice.channel: leave channel2voice alone (an extension) */
#define OLFX_DK_CHANNEL_RACK 16            /* olfx_control_event.pad: the kit's rack */

/* Level meter (OLFX_KIND_METER, OLFX_KIND_METER_MONO): two fields per instance, shared by its channels.
   Per signal the state is five floats, all 0 after create and olfx_reset; per frame with input x, in this order:
     if (count == window) { sum = 0; count = 0; }          before the add (ol_corelib.h:76-79)
     sum = sum + x * x;  count = count + 1.0f;
     rms = sqrtf(sum / count);                              what Rms::Process returns
     peak = (peak < fabsf(x)) ? fabsf(x) : peak;            sandbox/main.cpp:132
     peak_count = peak_count + 1.0f;
     if (peak_count == hold) { peak_count = 0; peak = 0; }  :133-137
   all in fp32, the counters included (t_sample sample_count, t_sample peak_hold), no contraction.  The firmware
   writes abs(...); it is taken as fabsf here.  What follows from fp32 counters is kept: a window that is no whole
   number (Init(44100): 44100 / 375 = 117.6) or lies below the running count never matches, so the sum grows for
   ever; a NaN sample poisons rms until the next window reset and never enters peak (the compare is false).
     OLFX_MT_WINDOW     what Rms::Init(sample_rate, window) takes: 0 = sample_rate / 375 in fp32; default 0.
                        Setting it is Init again: the window changes, nothing is reset
     OLFX_MT_PEAK_HOLD  the firmware's peak_hold, default 96000 (2 * 48000, a literal: it does not follow the rate)
   Any finite value is accepted (a negative or fractional one never matches); a non-finite one is OLFX_E_ARG.  A
   change lands at the next block boundary like every parameter.  olfx_reset clears the state and keeps both
   fields (configuration, as a voice engine's buses are).  No control maps to a meter: olfx_control_map
   and olfx_control are OLFX_E_KIND.
   olfx_process with out == NULL (these two kinds only) is summary mode: the state advances, nothing is written
   per frame, and rms is that of the call's last frame (the member is overwritten every frame, so no other is
   observable).  It reads 4 B per signal-frame, half of what olfx_algorithmic_bytes_per_frame reports (the
   envelope mode's 4 B in + 4 B out).  The two modes leave the same state in any alternation, bit for bit. */
enum { OLFX_MT_WINDOW = 0, OLFX_MT_PEAK_HOLD, OLFX_MT_NPARAMS };

/* ---- note events (voices) ----
   The ol::synth::Voice calls that change a voice's gate or pitch (Voice.h:33-57), as SynthVoice
   implements them (SynthVoice.h:231-268):
     NOTE_ON        NoteOn(note, vel)  = GateOn + freq_ = mtof(note) + Retrigger(true) on both envelopes
     NOTE_OFF       NoteOff(note, vel) = GateOff
     GATE_ON        GateOn()           = gate = true (the envelopes see the rising edge, no retrigger)
     GATE_OFF       GateOff()          = gate = false
     SET_FREQUENCY  SetFrequency(hz)   = freq_ = hz (olfx_voice_event.value; olfx_voice_events only) */
enum { OLFX_EV_NOTE_OFF = 0, OLFX_EV_NOTE_ON = 1, OLFX_EV_GATE_ON = 2, OLFX_EV_GATE_OFF = 3,
       OLFX_EV_SET_FREQUENCY = 4 };
typedef struct olfx_event {
    uint32_t inst;      /* instance index */
    uint8_t  type;      /* OLFX_EV_* (not SET_FREQUENCY) */
    uint8_t  note;      /* MIDI note (NoteOn: freq = mtof(note)) */
    uint8_t  velocity;  /* unused by SynthVoice (SynthVoice.h:245) */
    uint8_t  pad;
} olfx_event;
typedef struct olfx_voice_event {
    uint32_t inst;      /* instance index */
    uint8_t  type;      /* OLFX_EV_* */
    uint8_t  note;      /* NOTE_ON: MIDI note */
    uint8_t  velocity;  /* unused by SynthVoice */
    uint8_t  pad;
    float    value;     /* SET_FREQUENCY: Hz (finite); else unused */
} olfx_voice_event;
/* A note event at a frame inside the block (olfx_timed_events): `frame` counts from the first frame of
   the next olfx_process and is a multiple of 4, the engine's frame granularity (the firmware's
   AUDIO_BLOCK_SIZE, a MidiBuffer position rounded to it). */
typedef struct olfx_timed_event {
    uint32_t frame;         /* multiple of 4, below 2^31 */
    olfx_voice_event ev;
} olfx_timed_event;
/* A note at a frame inside the block for an instrument (olfx_timed_notes): instrument-addressed, routed through
   Polyvoice / the VoiceMap when the engine reaches its frame. */
typedef struct olfx_timed_note {
    uint32_t frame;         /* multiple of 4, below 2^31 */
    olfx_event ev;
} olfx_timed_note;

/* ---- control changes (MIDI CC / hardware controls; corelib/cc_map.h numbers) ----
   The reference's UpdateMidiControl(control, 0..127) / UpdateHardwareControl(control, float)
   mapped to one parameter field, per kind:
     OLFX_KIND_VOICE : SynthVoice::UpdateMidiControl / UpdateHardwareControl (SynthVoice.h:100-229)
     OLFX_KIND_FXRACK: FxRack::UpdateMidiControl / UpdateHardwareControl (Fx.h:451-489) and the
                       DelayFx / ReverbFx / FilterFx handlers it forwards to (Fx.h:116-163, 218-267, 313-391);
                       olfx_control_map gives topology 0's mapping, olfx_control uses each instance's
                       topology (OLFX_FR_TOPOLOGY 1: the firmware's direct FilterFx routing)
     OLFX_KIND_PLATERACK: the rack's, with the reverb CCs reaching the plate (the table at OLFX_PR_*)
   Controls the reference ignores for a kind (its `default: update = false`) are skipped. */
enum { OLFX_CTL_MIDI = 0, OLFX_CTL_HARDWARE = 1 };
#define OLFX_IGNORED 1                 /* olfx_control_map: the reference ignores this control */
#define OLFX_FIELD_UPDATE_ONLY 0xFFFFFFFFu   /* handled control that sets no modelled field (Update() only) */
typedef struct olfx_control_event {
    uint32_t inst;
    uint8_t  control;   /* CC number, corelib/cc_map.h */
    uint8_t  source;    /* OLFX_CTL_MIDI (value 0..127) or OLFX_CTL_HARDWARE (value as given) */
    uint16_t pad;       /* OLFX_KIND_DRUMKIT: the MIDI channel 0..15, or OLFX_DK_CHANNEL_RACK; other kinds ignore it */
    float    value;
} olfx_control_event;

/* ---- the drum kit's VoiceMap (OLFX_KIND_DRUMKIT) ----
   Each record is VoiceMap::SetVoice(channel, note, voice) on kit `kit` (VoiceMap.h:45-58): note2voice[note] = voice;
   channel2voice[channel] = voice.  Whatever sat at that note or channel is displaced (the reference overwrites the
   entry); voice = OLFX_DK_NO_VOICE clears the entries.  Extensions: note = OLFX_DK_NO_NOTE or channel =
   OLFX_DK_NO_CHANNEL leaves that table alone.  Records apply in order and the call is judged on the state after its
   last record: if a voice of a kit would then sit at two notes, or a kit (>= n), voice (>= P), note (128..254) or
   channel (16..254) is out of range, the call returns OLFX_E_ARG and changes nothing.  (Two voices may swap their
   notes in one call.) */
typedef struct olfx_drumkit_voice {
    uint32_t kit;
    uint32_t voice;     /* voice slot 0..P-1, or OLFX_DK_NO_VOICE */
    uint8_t  channel;   /* 0..15, or OLFX_DK_NO_CHANNEL */
    uint8_t  note;      /* 0..127, or OLFX_DK_NO_NOTE */
    uint16_t pad;
} olfx_drumkit_voice;

/* ---- I/O flags ---- */
enum {
    OLFX_IO_DEVICE = 0,  /* in/out are device pointers (no copies; the fast path) */
    OLFX_IO_HOST   = 1   /* in/out are host pointers: staged through pinned buffers, PCIe-inclusive */
};

typedef struct olfx_engine olfx_engine;

typedef struct olfx_kind_info {
    int      kind;
    uint32_t n_params;
    uint32_t in_channels;       /* channels olfx_process reads */
    uint32_t out_channels;      /* channels olfx_process writes */
    uint64_t state_bytes_per_instance;   /* device state (rings + scalars + params); a reverb
                                            engine of 2 x 64 x CUs instances or more whose
                                            pre-delays come to differ adds 32 KB per instance (a
                                            copy of the pre-delay ring while its layout changes,
                                            DESIGN.md section 4), allocated at the first such
                                            block, kept until destroy */
} olfx_kind_info;

int olfx_abi_version(void);
int olfx_kind_info_get(int kind, float sample_rate, olfx_kind_info *info);

/* Create an engine of `kind` with n_inst instances on HIP device `device`.  All instances start
   in the reference's freshly-created state (zeroed rings, default parameters).
   block = the frames per olfx_process call the caller intends (any multiple of 4 is accepted). */
int olfx_create(int kind, int device, uint32_t n_inst, float sample_rate, uint32_t block,
                olfx_engine **out);
/* An OLFX_KIND_SYNTH engine of n_inst instruments with `voices` (1..8) SynthVoices each;
   olfx_create(OLFX_KIND_SYNTH, ...) is the firmware's 4. */
int olfx_create_synth(int device, uint32_t n_inst, uint32_t voices, float sample_rate, uint32_t block,
                      olfx_engine **out);
/* The same for either synth kind: kind is OLFX_KIND_SYNTH or OLFX_KIND_SYNTH_SVF (else OLFX_E_KIND). */
int olfx_create_synth_kind(int kind, int device, uint32_t n_inst, uint32_t voices, float sample_rate, uint32_t block,
                           olfx_engine **out);
/* An OLFX_KIND_DRUMKIT engine of n_kits kits with `voices` (1..8) sample voices each; olfx_create(OLFX_KIND_DRUMKIT,
   ...) gives 4.  (olfx_create_synth_kind refuses the kind: it is no synth.) */
int olfx_create_drumkit(int device, uint32_t n_kits, uint32_t voices, float sample_rate, uint32_t block,
                        olfx_engine **out);
int olfx_destroy(olfx_engine *e);

/* Zero all state and restore defaults (== destroy + create, without reallocating).  Like
   olfx_destroy and olfx_sync it waits for THIS engine's queued work only (the stream of its latest
   olfx_process / olfx_mix, its own streams, its control packets), never for the whole device:
   other engines and the host's own kernels keep running.  The caller keeps the stream it passed
   last alive until then (and until the next olfx_process / olfx_mix on another stream, which the
   engine orders after its previous launch itself: switching streams between calls needs no event
   from the caller; the caller's own buffers stay the caller's to order). */
int olfx_reset(olfx_engine *e);

/* Set parameters of instances [first, first+count): `values` is field-major
   [n_fields][count] for fields [field0, field0+n_fields).  Host pointer.  Applied at the start
   of the next olfx_process. */
int olfx_set_params(olfx_engine *e, uint32_t first, uint32_t count, uint32_t field0,
                    uint32_t n_fields, const float *values);
/* Convenience: one field of one instance. */
int olfx_set_param(olfx_engine *e, uint32_t inst, uint32_t field, float value);
/* One field of `count` scattered instances: inst[k] gets values[k] (the per-instance setter called
   on each, e.g. one MIDI CC fanned out to many objects).  Validated first: a rejected call changes
   nothing.  Applied at the start of the next olfx_process, like every parameter change; the
   engine re-derives and uploads the coefficients of changed instances only, asynchronously. */
int olfx_set_param_list(olfx_engine *e, uint32_t field, const uint32_t *inst, const float *values,
                        uint32_t count);
/* A member value without Update(): the state the reference's setters leave when they are called
   BEFORE Init (the Daisy firmware configures its voices that way, ol_daisy/app/synth/main.cpp:114-128
   then :149).  For voices, SynthVoice::Init resets the components to DaisySP's defaults, while
   Process keeps reading the members filter_cutoff, filter_env_amount, amp_env_amount and Init hands
   portamento_htime to the Port (SynthVoice.h:31-53): the field is stored without the Update() that
   olfx_set_params implies.  For the other kinds it is olfx_set_param. */
int olfx_set_member(olfx_engine *e, uint32_t inst, uint32_t field, float value);
/* Read back the current (host shadow) value of one parameter. */
int olfx_get_param(olfx_engine *e, uint32_t inst, uint32_t field, float *value);

/* Map one control change to (field, value) exactly as the reference handler scales it
   (ol::core::scale, corelib/ol_corelib.h:31-44).  Returns OLFX_OK, OLFX_IGNORED, or an error.
   Pure host function: no engine, no device.  OLFX_KIND_SYNTH, OLFX_KIND_SYNTH_SVF: OLFX_E_KIND -- a control
   can hit two of their fields, see olfx_synth_control_map / olfx_synth_control_map_at. */
int olfx_control_map(int kind, uint8_t control, int source, float value, uint32_t *field, float *param_value);
/* The same for an OLFX_KIND_SYNTH instrument (the firmware's handleMidi fan-out, main.cpp:201-207): the
   voices' mapping first (OLFX_SY_VOICE0 + ..., or OLFX_FIELD_UPDATE_ONLY), then the rack's topology-1
   mapping (OLFX_SY_RACK0 + ...).  Returns the number of fields hit (0..2) or an error.  Pure host function. */
int olfx_synth_control_map(uint8_t control, int source, float value, uint32_t field[2], float param_value[2]);
/* The same for either synth kind at a rack topology: the voices' mapping of that kind, then the mapping
   olfx_control uses on an OLFX_KIND_FXRACK instance of that topology (0: FxRack's handlers, 1: the firmware's
   direct routing).  kind OLFX_KIND_SYNTH at topology 1 equals olfx_synth_control_map; OLFX_E_ARG for a topology
   the kind does not accept (OLFX_KIND_SYNTH: anything but 1; OLFX_KIND_SYNTH_SVF: anything but 0 or 1),
   OLFX_E_KIND for another kind.  Pure host function. */
int olfx_synth_control_map_at(int kind, uint32_t topology, uint8_t control, int source, float value, uint32_t field[2],
                              float param_value[2]);
/* Apply control changes in order (each: the mapped olfx_set_param; ignored controls skipped).
   Replaces UpdateMidiControl / UpdateHardwareControl per instance. */
int olfx_control(olfx_engine *e, const olfx_control_event *ev, uint32_t n);

/* Queue note events (voices); applied in order at the start of the next olfx_process. */
int olfx_note_events(olfx_engine *e, const olfx_event *ev, uint32_t n);
/* The same queue with SET_FREQUENCY (Voice::SetFrequency, SynthVoice.h:264-267) as well. */
int olfx_voice_events(olfx_engine *e, const olfx_voice_event *ev, uint32_t n);
/* Note events at a frame inside the block (OLFX_KIND_VOICE, OLFX_KIND_VOICE_MOOG, OLFX_KIND_VOICE_SAMPLE).
   Events apply in order of (frame, queueing order): olfx_note_events and olfx_voice_events queue at
   frame 0, ties keep call order, and the events of one frame on one voice compose as a block's do.  One
   olfx_process(N) computes, bit for bit, what a process call per distinct event frame below N computes
   with that frame's events queued by olfx_voice_events before it -- output and state.  An event at or
   past N stays queued with its frame reduced by N when the call returns (frame == N: frame 0 of the next
   call), so a whole score can be queued up front and rendered block by block.  Parameter changes,
   olfx_control, olfx_update, olfx_sample_voices and olfx_sample_bank still land at the block boundary,
   before frame 0's events; olfx_reset drops pending timed events with the untimed ones.
   OLFX_E_ARG (nothing is queued): a frame that is no multiple of 4 or not below 2^31, or a record
   olfx_voice_events refuses.  OLFX_E_KIND: the synth kinds and the drum kit -- these events address a voice,
   and an instrument's notes are routed: olfx_timed_notes, below.  OLFX_E_STATE: effect and meter kinds. */
int olfx_timed_events(olfx_engine *e, const olfx_timed_event *ev, uint32_t n);
/* Notes at a frame inside the block for OLFX_KIND_SYNTH, OLFX_KIND_SYNTH_SVF and OLFX_KIND_DRUMKIT.  The
   contract of olfx_timed_events carries over: one olfx_process(N) computes, bit for bit in output and stored
   state, what one process call per distinct event frame below N computes with that frame's notes handed to
   olfx_note_events just before it, and olfx_synth_playing reads the same after both.  So a note is routed when
   the engine reaches its frame, not at this call:
     - a note at frame 0 is routed here and joins the untimed queue, exactly as olfx_note_events does (ties keep
       call order);
     - a note at frame f > 0 stays pending, unrouted, and is routed inside the olfx_process whose frames contain
       f, in order of (frame, queueing order), against Playing() as the earlier frames' notes left it: a NoteOn
       at frame 8 finds free the voice a NoteOff at frame 4 released, and a NoteOn with no free voice at its
       frame is dropped, as Polyvoice drops it.  A drum kit uses the VoiceMap in force at that olfx_process:
       olfx_drumkit_map between queueing and processing reroutes pending notes;
     - a note at or past N stays pending with its frame reduced by N; one whose frame becomes 0 is routed as that
       olfx_process returns, ahead of anything queued afterwards;
     - GATE_ON / GATE_OFF fan out to every voice at their frame.
   olfx_synth_playing is Playing() as of the frames processed so far, plus the frame-0 notes queued since.
   Parameter, control, map and sample changes still land at the block boundary, before frame 0's notes;
   olfx_reset drops pending timed notes.  A launch takes 16 distinct times; a call with more runs as several.
   OLFX_E_ARG (nothing is queued, Playing() untouched): null with n > 0, a frame that is no multiple of 4 or
   not below 2^31, or a record olfx_note_events refuses on that kind (inst out of range, note > 127,
   type > GATE_OFF; a drum kit: type > NOTE_ON).  OLFX_E_KIND: the three voice kinds (olfx_timed_events).
   OLFX_E_STATE: effect and meter kinds. */
int olfx_timed_notes(olfx_engine *e, const olfx_timed_note *ev, uint32_t n);
/* Parameter and control changes at a frame inside the block (OLFX_KIND_VOICE, OLFX_KIND_VOICE_MOOG,
   OLFX_KIND_VOICE_SAMPLE).  A parameter record is olfx_set_param(inst, field, value) at its frame, a control
   record olfx_control(&ev, 1) at its frame: UpdateConfig + Update() of that voice there, as olfx_set_param
   implies it.  A control that maps to OLFX_FIELD_UPDATE_ONLY is Update() at its frame (the voice becomes
   configured there); a control the reference ignores is skipped.  One olfx_process(N) computes, bit for bit in
   output and stored state, what one process call per distinct time below N computes -- a time being the frame
   of a timed event or of a timed parameter record -- when before each call that time's parameter records are
   applied by olfx_set_param / olfx_control in queueing order (both calls share one order) and that time's
   events are then queued by olfx_voice_events.  At a frame, parameter changes precede events whatever the
   queueing order: the block-boundary rule.
     - a record at frame 0 is exactly olfx_set_param / olfx_control now;
     - a record at or past N stays pending with its frame reduced by N; one whose frame becomes 0 is applied as
       that olfx_process returns, ahead of anything set afterwards; olfx_reset drops pending records;
     - olfx_get_param reads the value as of the frames processed so far, plus the frame-0 writes made since, and
       olfx_set_member's OLFX_E_STATE rule is judged on that same state;
     - olfx_set_params, olfx_set_param_list, olfx_control, olfx_update, olfx_sample_voices and olfx_sample_bank
       keep landing at the block boundary, before every pending timed record;
     - parameter times and event times share the 16 segments of a launch, and a launch carries at most n_inst
       changed-voice records; a call with more runs as several launches.
   OLFX_E_ARG (nothing is queued, the shadow is untouched): null with n > 0, a frame that is no multiple of 4 or
   not below 2^31, inst or field out of range, a value olfx_set_param refuses, a control record olfx_control
   refuses.  OLFX_E_KIND: every kind but the three voice kinds. */
typedef struct olfx_timed_param {
    uint32_t frame;         /* multiple of 4, below 2^31 */
    uint32_t inst;
    uint32_t field;
    float    value;
} olfx_timed_param;
/* (a struct tag only: the record shares its name with the call, which a typedef name could not) */
struct olfx_timed_control {
    uint32_t frame;         /* multiple of 4, below 2^31 */
    olfx_control_event ev;
};
int olfx_timed_params(olfx_engine *e, const olfx_timed_param *rec, uint32_t n);
int olfx_timed_control(olfx_engine *e, const struct olfx_timed_control *rec, uint32_t n);
/* The same for OLFX_KIND_SYNTH, OLFX_KIND_SYNTH_SVF and OLFX_KIND_DRUMKIT, with the same record types: `inst` is the
   instrument or kit, `field` an OLFX_SY_* / OLFX_DK_* index, and for a kit ev.pad the MIDI channel or
   OLFX_DK_CHANNEL_RACK.  So a MIDI buffer of notes (olfx_timed_notes) and CCs can be queued whole.  One
   olfx_process(N) computes, bit for bit in output and stored state, what one olfx_process per distinct time below N
   computes -- a time being the frame of a timed note or of one of these records -- when before each call that
   time's records are applied by olfx_set_param / olfx_control in queueing order (both calls share one order) and
   that time's notes are then handed to olfx_note_events; olfx_synth_playing and olfx_get_param read the same after
   both.  At a frame, parameter changes precede notes whatever the queueing order: the block-boundary rule.
     - a record at frame 0 is exactly olfx_set_param / olfx_control now;
     - a record at or past N stays pending with its frame reduced by N; one whose frame becomes 0 is applied as
       that olfx_process returns, ahead of anything set afterwards; olfx_reset drops pending records;
     - a control is mapped when the engine reaches its frame, not here (unlike the voice kinds'): under the
       instrument's topology at that frame -- a TOPOLOGY record at frame 8 changes what CC 45 at frame 12 maps to
       -- and, for a kit, the channel2voice table in force at that olfx_process, as timed notes use the map;
     - the fan-out is olfx_control's: on the synths the voices, then the rack (CCs 41-44 hit the voice filter and
       FILTER_* at topology 1); on a kit the channel's voice alone, or the rack.  OLFX_FIELD_UPDATE_ONLY is Update()
       of the voices it reaches, at that frame; a control the reference ignores is skipped;
     - a write to a voice field is UpdateConfig + Update() of every voice of the instrument on the synths and
       Update() of exactly that voice slot on a kit, as olfx_set_param; fields of slots p >= P are stored only;
     - olfx_set_params, olfx_set_param_list, olfx_control, olfx_update, olfx_drumkit_map, olfx_sample_voices and
       olfx_sample_bank keep landing at the block boundary, ahead of every pending record.
   Cost.  Record times and note times share the 16 segments of a launch.  The voice fields and REVERB_BALANCE,
   FILTER_CUTOFF, FILTER_RESONANCE, FILTER_DRIVE, FILTER_TYPE and MASTER_VOLUME change at their frame inside one
   launch.  DELAY_TIME, DELAY_FEEDBACK, DELAY_BALANCE, DELAY_CUTOFF, DELAY_RESONANCE and TOPOLOGY obey the same
   contract, but the delay stage's geometry is fixed per launch: a call with such a change -- or with CC 35-39 to a
   rack, which may map to one -- runs as several launches, one ending at each such time.  A launch also takes at
   most n_inst raw records (a kit: voices x n_inst; a time's records count as that many at the most, so one time
   always fits); a call with more runs as several launches.
   OLFX_E_ARG (nothing is queued, the shadow is untouched): null with n > 0, a frame that is no multiple of 4 or
   not below 2^31, inst or field out of range, a value olfx_set_param refuses (a topology the kind does not accept
   among them), a control record olfx_control refuses on that kind under any topology the kind accepts.
   OLFX_E_KIND: the three voice kinds (olfx_timed_params).  OLFX_E_STATE: effect and meter kinds. */
int olfx_timed_instrument_params(olfx_engine *e, const olfx_timed_param *rec, uint32_t n);
int olfx_timed_instrument_control(olfx_engine *e, const struct olfx_timed_control *rec, uint32_t n);
/* OLFX_KIND_SYNTH / OLFX_KIND_SYNTH_SVF / OLFX_KIND_DRUMKIT: Playing() of the `voices` voices of instrument (kit) inst,
   as of the calls made so far (with timed notes: as of the frames processed so far). */
int olfx_synth_playing(olfx_engine *e, uint32_t inst, uint8_t *playing /*[voices]*/);

/* Update() of instances [first, first + count) with their current parameters (SynthVoice.h:66-98,
   Fx.h Update()): for voices, the first Update() ends SynthVoice::Init's component defaults
   (olfx_set_params and olfx_control imply it).  Applied at the next olfx_process. */
int olfx_update(olfx_engine *e, uint32_t first, uint32_t count);

/* Process n_frames (multiple of 4) for all instances.  `stream` is a hipStream_t; NULL is the
   HIP default (null) stream, as everywhere in HIP; olfx_stream(e) is the engine's own stream.
   With OLFX_IO_DEVICE the call is asynchronous on that stream.  out == NULL is OLFX_E_ARG, except on the
   level-meter kinds, where it selects their summary mode (OLFX_MT_*, above). */
int olfx_process(olfx_engine *e, const float *in, float *out, uint32_t n_frames, int io_flags,
                 void *stream);

/* ---- voice buses (voice engines): the Polyvoice / VoiceMap sums ----
   Polyvoice::Process (modules/synthlib/Polyvoice.h:28-33) and VoiceMap::Process (VoiceMap.h:64-73)
   add their voices' samples into the caller's frame one voice at a time (`*frame_out += sample`).
   A bus is such a list.  olfx_mix_config sets the buses (host arrays, copied): bus b adds the
   voices order[offsets[b] .. offsets[b+1]) in that order; offsets has n_buses + 1 entries and
   starts at 0.  A voice may appear at most once over all buses (listed twice, the reference would
   run it twice per frame); n_buses = 0 removes the buses.
   olfx_mix adds, for every frame f and bus b, the bus's voice samples voice_out[f][v] into
   bus_out[f][b] in list order: the reference's float adds, bit for bit.  voice_out is
   [n_frames][n_inst] (this engine's olfx_process output); bus_out is [n_frames][n_buses] and is
   accumulated into (the reference's caller zeroes its frame).  Both host (OLFX_IO_HOST) or both
   device pointers (OLFX_IO_DEVICE: asynchronous on `stream`, as olfx_process). */
int olfx_mix_config(olfx_engine *e, uint32_t n_buses, const uint32_t *offsets, const uint32_t *order);
int olfx_mix(olfx_engine *e, const float *voice_out, float *bus_out, uint32_t n_frames, int io_flags,
             void *stream);

/* ---- sample voices (OLFX_KIND_VOICE_SAMPLE): ol::synth::Sample over a device-resident bank ----
   The bank is n_samples mono float32 buffers: sample k is pcm[offsets[k] .. offsets[k+1]) (frames; offsets
   has n_samples + 1 entries, starts at 0 and never decreases; each sample has fewer than 2^32 - 1 frames).
   olfx_sample_bank copies the host arrays to the device and replaces the whole bank; it waits for this
   engine's queued work only (as olfx_reset).  After it every voice's Sample is fresh (not playing, cursor 0);
   a voice keeps its assignment if the index is still valid, else it becomes unassigned.  n_samples = 0
   removes the bank.  OLFX_E_NOMEM (allocation failed) leaves the old bank in place.
   The data source is the in-memory one: Read writes pcm[pos++] and returns 1 while pos < len, else writes
   nothing and returns 0; Seek(k) sets pos = min(k, len).  The frame handed to Sample::Process is the
   caller's zeroed frame (0.0f), as with olfx_mix: a paused, unassigned or exhausted voice feeds zeros into
   its filter.  Sample::Process's loop rule is the reference's (Sample.cpp:13-20): in Loop mode,
   Seek(loop_start) when nothing was read or when loop_end != 0 and the frame count passed loop_end; loop
   points may be any value (an end past the sample gives one silent tick per turn, a start past it silence
   after the first pass).  OneShot at the end keeps `playing` and reads nothing.
   olfx_sample_voices gives voices their Sample: validated first (a rejected call changes nothing), applied
   at the next block boundary, before that boundary's note events.  A new `sample` index, or OLFX_NO_SAMPLE,
   constructs a fresh Sample (OneShot unless the record says Loop, not playing, cursor 0); the same index
   with a new mode or loop points is SetPlayMode / SetLoopStart / SetLoopEnd: no seek, the cursor is kept.
   olfx_reset keeps the bank and the assignments, as it keeps the olfx_mix_config buses (configuration, not
   state); every Sample is fresh after it. */
#define OLFX_NO_SAMPLE 0xFFFFFFFFu
enum { OLFX_SAMPLE_ONESHOT = 0, OLFX_SAMPLE_LOOP = 1 };   /* ol::synth::SamplePlayMode (Sample.h:11-14) */
typedef struct olfx_sample_voice {
    uint32_t inst;          /* voice */
    uint32_t sample;        /* index into the bank, or OLFX_NO_SAMPLE */
    uint32_t play_mode;     /* OLFX_SAMPLE_* */
    uint32_t pad;
    uint64_t loop_start;    /* frames */
    uint64_t loop_end;      /* frames; 0 = none */
} olfx_sample_voice;
int olfx_sample_bank(olfx_engine *e, uint32_t n_samples, const uint64_t *offsets, const float *pcm);
int olfx_sample_voices(olfx_engine *e, const olfx_sample_voice *recs, uint32_t n);
/* OLFX_KIND_DRUMKIT: apply n VoiceMap records (above); OLFX_E_STATE on another kind. */
int olfx_drumkit_map(olfx_engine *e, const olfx_drumkit_voice *recs, uint32_t n);

/* ---- level meters (OLFX_KIND_METER, OLFX_KIND_METER_MONO) ----
   The five state floats of every channel of instances [first, first + count), copied to the host:
   levels[(k * channels) + c] is channel c of instance first + k.  Waits for this engine's queued work only (as
   olfx_reset).  OLFX_E_STATE on another kind. */
typedef struct olfx_meter_level { float rms, peak, sum, count, peak_count; } olfx_meter_level;
int olfx_meter_read(olfx_engine *e, uint32_t first, uint32_t count, olfx_meter_level *levels /*[count][channels]*/);

/* Block until all work queued by this engine is done (engine-scoped, see olfx_reset). */
int olfx_sync(olfx_engine *e);
/* The engine's own non-blocking hipStream_t (valid until olfx_destroy). */
void *olfx_stream(const olfx_engine *e);

/* Engine facts. */
uint32_t olfx_num_instances(const olfx_engine *e);
int      olfx_kind(const olfx_engine *e);
uint64_t olfx_frames_processed(const olfx_engine *e);   /* per instance, since create/reset */
uint32_t olfx_num_buses(const olfx_engine *e);          /* voice buses (olfx_mix_config) */
uint32_t olfx_synth_voices(const olfx_engine *e);       /* voices per instrument (the synth kinds, the drum kit), else 0 */
/* Algorithmic ("compulsory") HBM bytes per instance-frame of the dominant kernel, the figure
   bench.py's roofline uses. */
double   olfx_algorithmic_bytes_per_frame(const olfx_engine *e);
/* The read share of the same figure: tap reads of data older than the block plus the input (the
   north star's "HBM-read roofline", SURVEY.md section 8d "read-only variant"). */
double   olfx_algorithmic_read_bytes_per_frame(const olfx_engine *e);
const char *olfx_kernel_name(const olfx_engine *e);
/* OLFX_KIND_CHORUS: 1 if the next olfx_process would run the ring-free kernel (chorus_block_rf1: the
   pitch-shifter's past output rebuilt from the input ring), 0 if the ring kernel olfx_kernel_name
   reports (while a pitch or window change is younger than the chorus history); -1 for other kinds. */
int      olfx_chorus_ring_free(const olfx_engine *e);
const char *olfx_last_error(const olfx_engine *e);   /* e may be NULL: last global error */

#ifdef __cplusplus
}
#endif
#endif /* OLFX_H */
