/*
 * tests/sampler_ref/sampler_ref.c -- CPU reference for the sample-playback voice
 * (OLFX_KIND_VOICE_SAMPLE).  TEST INFRASTRUCTURE ONLY.
 *
 * A C restatement of SynthVoice(new SampleSoundSource<1>(sample), new SvfFilter, ...):
 *   - the sound source: ol::synth::Sample (modules/synthlib/Sample.cpp:9-62) over an in-memory mono
 *     source (Read: frame = pcm[pos++], 1 while pos < len, else nothing, 0; Seek(k): pos = min(k, len)),
 *     driven by SampleSoundSource<1> (SampleSoundSource.h:13-40: GateOn = Seek(0) + Play(), GateOff =
 *     Pause(), SetFreq stores).  Both of the reference's cursors are kept (current_frame_ and the
 *     source's position), literally;
 *   - the voice tick, setters and Adsr of oracle/voice_ref.c (SynthVoice.h:41-53, 55-98, 231-268), in
 *     both arithmetics: the unfused restatement (voice_tick) and the kernels' (voice_tick_k), with the
 *     oscillator's sample replaced by Sample::Process on a zeroed frame.  tests/test_sampler_ref.py
 *     pins this copy to oracle/voice_ref.c bit for bit (a constant sample against the oscillator at 0 Hz).
 * v_rcp_f32 in the kernels' arithmetic is liboracle's oracle_rcp_model, handed in as a function
 * pointer (sref_set_rcp), so the model is the table the tests install there.
 * Compiled with the oracle's flags: -O2 -ffp-contract=off -fno-fast-math.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

enum { SEG_IDLE = 0, SEG_ATTACK = 1, SEG_DECAY = 2, SEG_RELEASE = 3 };
enum { P_FILTER_CUTOFF = 0, P_FILTER_RESONANCE, P_FILTER_DRIVE, P_FILTER_ENV_AMOUNT, P_FILTER_ATTACK,
       P_FILTER_ATTACK_SHAPE, P_FILTER_DECAY, P_FILTER_SUSTAIN, P_FILTER_RELEASE, P_AMP_ENV_AMOUNT,
       P_AMP_ATTACK, P_AMP_ATTACK_SHAPE, P_AMP_DECAY, P_AMP_SUSTAIN, P_AMP_RELEASE, P_PORTAMENTO, P_N };

typedef struct {
    float x, atk_d0, atk_tgt, dec_d0, rel_d0, sus;
    int mode, gate_prev;
} adsr_t;

/* ol::synth::Sample + its in-memory SampleDataSource */
typedef struct {
    int sample;                 /* bank index, -1: none (a zero-length source) */
    int loop;                   /* play_mode_ == Loop */
    int playing;
    uint64_t loop_start, loop_end, current_frame, pos;
} sample_t;

typedef struct {
    sample_t smp;
    float sr, fc_max, res, pre_drive, drive, low, band;
    adsr_t amp_env, filt_env;
    float freq, amp_env_amount, filter_cutoff, filter_env_amount;
    int gate;
} voice_t;

typedef struct {
    int n;
    float sr;
    voice_t *v;
    int n_samples;
    uint64_t *off;              /* [n_samples + 1] */
    float *pcm;
} sref;

static float (*g_rcp)(float);
void sref_set_rcp(float (*fn)(float)) { g_rcp = fn; }
static float rcp(float x) { return g_rcp ? g_rcp(x) : 1.0f / x; }

/* ---- the data source and Sample ---- */
static uint64_t src_len(const sref *o, const sample_t *s)
{
    return s->sample >= 0 && s->sample < o->n_samples ? o->off[s->sample + 1] - o->off[s->sample] : 0;
}
static void sample_seek(const sref *o, sample_t *s, uint64_t k)
{
    const uint64_t len = src_len(o, s);
    s->pos = k < len ? k : len;         /* data_source_.Seek */
    s->current_frame = k;
}
/* Sample::Process (Sample.cpp:9-23) */
static void sample_process(const sref *o, sample_t *s, float *frame)
{
    if (s->playing) {
        uint64_t frames_read = 0;
        if (s->pos < src_len(o, s)) { *frame = o->pcm[o->off[s->sample] + s->pos++]; frames_read = 1; }
        s->current_frame += frames_read;
        if (s->loop) {
            if (!frames_read || (s->loop_end && s->current_frame > s->loop_end)) sample_seek(o, s, s->loop_start);
        }
    }
}
static void sample_fresh(sample_t *s, int sample)
{
    memset(s, 0, sizeof(*s));
    s->sample = sample;
}

/* ---- daisysp::Adsr, as oracle/voice_ref.c ---- */
static void adsr_attack(adsr_t *e, float T, float shape, float sr)
{
    float target = 9.f * powf(shape, 10.f) + 0.3f * shape + 1.01f;
    e->atk_tgt = target;
    if (T > 0.f) {
        float logTarget = logf(1.f - (1.f / target));
        e->atk_d0 = 1.f - expf(logTarget / (T * sr));
    } else {
        e->atk_d0 = 1.f;
    }
}
static float adsr_tc(float T, float sr)
{
    if (T > 0.f) {
        const float target = logf((float)(1. / M_E));
        return 1.f - expf(target / (T * sr));
    }
    return 1.f;
}
static float adsr_sus(float s) { return (s <= 0.f) ? -0.01f : (s > 1.f ? 1.f : s); }
static void adsr_init(adsr_t *e, float sr)
{
    memset(e, 0, sizeof(*e));
    e->sus = 0.7f;
    e->mode = SEG_IDLE;
    adsr_attack(e, 0.1f, 0.0f, sr);
    e->dec_d0 = adsr_tc(0.1f, sr);
    e->rel_d0 = adsr_tc(0.1f, sr);
}
static float adsr_process(adsr_t *e, int gate)
{
    if (gate && !e->gate_prev) e->mode = SEG_ATTACK;
    else if (!gate && e->gate_prev) e->mode = SEG_RELEASE;
    e->gate_prev = gate;
    float d0 = e->atk_d0;
    if (e->mode == SEG_DECAY) d0 = e->dec_d0;
    else if (e->mode == SEG_RELEASE) d0 = e->rel_d0;
    float target = e->mode == SEG_DECAY ? e->sus : -0.01f;
    float out = 0.0f;
    switch (e->mode) {
    case SEG_ATTACK:
        e->x += d0 * (e->atk_tgt - e->x);
        out = e->x;
        if (out > 1.f) { e->x = out = 1.f; e->mode = SEG_DECAY; }
        break;
    case SEG_DECAY:
    case SEG_RELEASE:
        e->x += d0 * (target - e->x);
        out = e->x;
        if (out < 0.0f) { e->x = out = 0.f; e->mode = SEG_IDLE; }
        break;
    default: break;
    }
    return out;
}

static float fclampf(float in, float mn, float mx) { return fminf(fmaxf(in, mn), mx); }
#define MINF(a, b) ((a) < (b) ? (a) : (b))

/* SynthVoice::Init: the components' DaisySP defaults (the Sample itself is not touched: Sample::Init
   only stores the rate) */
static void voice_init(voice_t *v, float sr)
{
    const sample_t keep = v->smp;
    memset(v, 0, sizeof(*v));
    v->smp = keep;
    v->sr = sr; v->fc_max = sr / 3.f;
    v->res = 0.5f; v->pre_drive = 0.5f; v->drive = 0.5f;
    adsr_init(&v->amp_env, sr);
    adsr_init(&v->filt_env, sr);
    v->amp_env_amount = 0.8f;
    v->filter_cutoff = 0.0f;
    v->filter_env_amount = 1.0f;
}

/* SynthVoice::UpdateConfig -> Update (SynthVoice.h:55-98); the portamento feeds only SetFreq */
static void voice_update(voice_t *v, const float *p, float sr)
{
    v->filter_cutoff = p[P_FILTER_CUTOFF];
    v->filter_env_amount = p[P_FILTER_ENV_AMOUNT];
    v->amp_env_amount = p[P_AMP_ENV_AMOUNT];
    v->res = fclampf(p[P_FILTER_RESONANCE], 0.f, 1.f);
    v->drive = v->pre_drive * v->res;
    v->pre_drive = fclampf(p[P_FILTER_DRIVE] * 0.1f, 0.f, 1.f);
    v->drive = v->pre_drive * v->res;
    adsr_attack(&v->filt_env, p[P_FILTER_ATTACK], p[P_FILTER_ATTACK_SHAPE], sr);
    v->filt_env.dec_d0 = adsr_tc(p[P_FILTER_DECAY], sr);
    v->filt_env.sus = adsr_sus(p[P_FILTER_SUSTAIN]);
    v->filt_env.rel_d0 = adsr_tc(p[P_FILTER_RELEASE], sr);
    adsr_attack(&v->amp_env, p[P_AMP_ATTACK], p[P_AMP_ATTACK_SHAPE], sr);
    v->amp_env.dec_d0 = adsr_tc(p[P_AMP_DECAY], sr);
    v->amp_env.sus = adsr_sus(p[P_AMP_SUSTAIN]);
    v->amp_env.rel_d0 = adsr_tc(p[P_AMP_RELEASE], sr);
}

/* SynthVoice::Process, the restatement (oracle/voice_ref.c voice_tick with the source replaced) */
static float voice_tick(const sref *o, voice_t *v)
{
    float amp = adsr_process(&v->amp_env, v->gate);
    amp *= v->amp_env_amount;
    float src = 0.0f;                               /* the caller's zeroed frame */
    sample_process(o, &v->smp, &src);
    const float fc_in = v->filter_cutoff + ((adsr_process(&v->filt_env, v->gate) * 20000) * v->filter_env_amount);
    const float fc = fclampf(fc_in, 1.0e-6f, v->fc_max);
    const float fq = 2.0f * sinf(3.1415927410125732f * MINF(0.25f, fc / (v->sr * 2.0f)));
    const float damp = MINF(2.0f * (1.0f - powf(v->res, 0.25f)), MINF(2.0f, 2.0f / fq - fq * 0.5f));
    float notch = src - damp * v->band;
    v->low = v->low + fq * v->band;
    float high = notch - v->low;
    v->band = fq * high + v->band - v->drive * v->band * v->band * v->band;
    float out_low = 0.5f * v->low;
    notch = src - damp * v->band;
    v->low = v->low + fq * v->band;
    high = notch - v->low;
    v->band = fq * high + v->band - v->drive * v->band * v->band * v->band;
    out_low += 0.5f * v->low;
    return out_low * amp;
}

static float k_sin_quarter(float x)
{
    const float x2 = x * x;
    float p = fmaf(2.7557319e-6f, x2, -1.9841270e-4f);
    p = fmaf(p, x2, 8.3333333e-3f);
    p = fmaf(p, x2, -1.6666667e-1f);
    return fmaf(x * x2, p, x);
}

/* the kernels' arithmetic (oracle/voice_ref.c voice_tick_k, Svf voice, with the source replaced) */
static float voice_tick_k(const sref *o, voice_t *v)
{
    const float env_a = adsr_process(&v->amp_env, v->gate);
    const float amp = env_a * (0.5f * v->amp_env_amount);
    float src = 0.0f;
    sample_process(o, &v->smp, &src);
    const float fe = adsr_process(&v->filt_env, v->gate);
    const float fc_in = fmaf(fe * 20000.0f, v->filter_env_amount, v->filter_cutoff);
    const float fc = fminf(fmaxf(fc_in, 1.0e-6f), v->fc_max);
    const float inv_2sr = 1.0f / (v->sr * 2.0f);
    const float s = k_sin_quarter(3.1415927410125732f * fminf(fc * inv_2sr, 0.25f));
    const float fq = s + s;
    const float lim = rcp(s) - s;
    const float damp_res = 2.0f * (1.0f - powf(v->res, 0.25f));
    const float ndamp = fmaxf(fmaxf(-damp_res, -2.0f), -lim);
    float notch = src + ndamp * v->band;
    v->low = fmaf(fq, v->band, v->low);
    float high = notch - v->low;
    v->band = fmaf(-((v->drive * v->band) * v->band), v->band, fmaf(fq, high, v->band));
    const float low1 = v->low;
    notch = src + ndamp * v->band;
    v->low = fmaf(fq, v->band, v->low);
    high = notch - v->low;
    v->band = fmaf(-((v->drive * v->band) * v->band), v->band, fmaf(fq, high, v->band));
    return (low1 + v->low) * amp;
}

/* ---- the bank of voices ---- */
sref *sref_create(int n, float sr)
{
    if (n <= 0) return NULL;
    sref *o = (sref *)calloc(1, sizeof(*o));
    if (!o) return NULL;
    o->n = n;
    o->sr = sr;
    o->v = (voice_t *)calloc((size_t)n, sizeof(voice_t));
    if (!o->v) { free(o); return NULL; }
    for (int i = 0; i < n; i++) {
        sample_fresh(&o->v[i].smp, -1);
        voice_init(&o->v[i], sr);
    }
    return o;
}

void sref_destroy(sref *o)
{
    if (!o) return;
    free(o->v); free(o->off); free(o->pcm); free(o);
}

/* olfx_sample_bank: replace the bank; every Sample fresh; assignments kept where still valid */
int sref_bank(sref *o, int n_samples, const uint64_t *offsets, const float *pcm)
{
    if (!o || n_samples < 0) return -1;
    free(o->off); free(o->pcm);
    o->off = NULL; o->pcm = NULL; o->n_samples = 0;
    if (n_samples) {
        const uint64_t total = offsets[n_samples];
        o->off = (uint64_t *)malloc(sizeof(uint64_t) * ((size_t)n_samples + 1));
        o->pcm = (float *)malloc(sizeof(float) * (size_t)(total ? total : 1));
        if (!o->off || !o->pcm) return -1;
        memcpy(o->off, offsets, sizeof(uint64_t) * ((size_t)n_samples + 1));
        if (total) memcpy(o->pcm, pcm, sizeof(float) * (size_t)total);
        o->n_samples = n_samples;
    }
    for (int i = 0; i < o->n; i++) {
        sample_t *s = &o->v[i].smp;
        const sample_t old = *s;
        if (old.sample >= n_samples) {
            sample_fresh(s, -1);
        } else {
            sample_fresh(s, old.sample);
            s->loop = old.loop; s->loop_start = old.loop_start; s->loop_end = old.loop_end;
        }
    }
    return 0;
}

/* olfx_sample_voices, one record: another index constructs a fresh Sample, the same one is
   SetPlayMode / SetLoopStart / SetLoopEnd */
int sref_assign(sref *o, int inst, int sample, int loop, uint64_t loop_start, uint64_t loop_end)
{
    if (!o || inst < 0 || inst >= o->n || sample < -1 || sample >= o->n_samples) return -1;
    sample_t *s = &o->v[inst].smp;
    if (s->sample != sample) sample_fresh(s, sample);
    s->loop = loop;
    s->loop_start = loop_start;
    s->loop_end = loop_end;
    return 0;
}

int sref_config(sref *o, int inst, const float *values)
{
    if (!o || inst < 0 || inst >= o->n || !values) return -1;
    voice_update(&o->v[inst], values, o->sr);
    return 0;
}

/* OLFX_EV_*: 0 NoteOff, 1 NoteOn, 2 GateOn, 3 GateOff, 4 SetFrequency (SynthVoice.h:231-268) */
int sref_event(sref *o, int inst, int type, int note, float value)
{
    if (!o || inst < 0 || inst >= o->n) return -1;
    voice_t *v = &o->v[inst];
    switch (type) {
    case 1:
    case 2:
        v->gate = 1;                                    /* GateOn: gate, sound_source_->GateOn() */
        sample_seek(o, &v->smp, 0);
        v->smp.playing = 1;
        if (type == 1) {
            v->freq = powf(2.f, ((float)note - 69.0f) / 12.0f) * 440.0f;
            v->amp_env.mode = SEG_ATTACK; v->amp_env.x = 0.f;       /* Retrigger(true) */
            v->filt_env.mode = SEG_ATTACK; v->filt_env.x = 0.f;
        }
        return 0;
    case 0:
    case 3:
        v->gate = 0;                                    /* GateOff: gate, sound_source_->GateOff() */
        v->smp.playing = 0;
        return 0;
    case 4: v->freq = value; return 0;
    default: return -1;
    }
}

/* the Sample alone, for the source pins: op 0 Pause(), 1 Play(), 2 Seek(k) */
int sref_sample_ctl(sref *o, int inst, int op, uint64_t k)
{
    if (!o || inst < 0 || inst >= o->n) return -1;
    sample_t *s = &o->v[inst].smp;
    switch (op) {
    case 0: s->playing = 0; return 0;
    case 1: s->playing = 1; return 0;
    case 2: sample_seek(o, s, k); return 0;
    default: return -1;
    }
}

/* the bare source stream of one voice: Sample::Process on a zeroed frame, `frames` ticks */
int sref_source(sref *o, int inst, float *out, int frames)
{
    if (!o || inst < 0 || inst >= o->n) return -1;
    for (int f = 0; f < frames; f++) {
        out[f] = 0.0f;
        sample_process(o, &o->v[inst].smp, &out[f]);
    }
    return 0;
}

/* olfx_reset: every voice as created; the bank and the assignments stay, every Sample is fresh */
int sref_reset(sref *o)
{
    if (!o) return -1;
    for (int i = 0; i < o->n; i++) {
        sample_t *s = &o->v[i].smp;
        const sample_t old = *s;
        sample_fresh(s, old.sample);
        s->loop = old.loop; s->loop_start = old.loop_start; s->loop_end = old.loop_end;
        voice_init(&o->v[i], o->sr);
    }
    return 0;
}

/* out [frames][n]; kernel = 1: the kernels' arithmetic */
int sref_process(sref *o, float *out, int frames, int kernel)
{
    if (!o || frames < 0) return -1;
    const long n = o->n;
    for (long i = 0; i < n; i++)
        for (int f = 0; f < frames; f++)
            out[(long)f * n + i] = kernel ? voice_tick_k(o, &o->v[i]) : voice_tick(o, &o->v[i]);
    return 0;
}
