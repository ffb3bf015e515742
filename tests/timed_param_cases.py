"""olfx_timed_params against the oracle's kernel arithmetic: the cases as data, their reference, and the condition
each reference must meet.  No torch, no GPU.

tests/test_timed_params_ref.py runs every reference alone on the CPU and asserts its condition;
tests/test_gpu_timed_params.py runs the same cases on the engine and compares bit for bit.

A case is a timed_cases.Setup and a list of calls
  (untimed events, timed events, boundary work, timed parameters, n_frames)
as timed_cases.py states the first three.  A timed parameter is (frame, ("params", inst, column[16])): the voice's
whole configuration at that frame -- ref.config at its split point, and on the engine sixteen olfx_timed_params
records, one per field (set_param of every field of a voice is UpdateConfig + Update() of that column).

The reference is timed_cases.split_oracle, extended here and not edited: every call is cut at its parameter times
into calls of timed_cases' kind, a time's columns being the boundary work of the call that starts there -- so they
land ahead of that frame's events, as the header states -- and the events keep their frames through split_oracle's
own carry-over.

The condition: against the same case without its timed parameters, the reference is identical before the first
changed frame, and differs in at least one sample from that frame on for every changed voice that sounds there.  A
case may name voices whose change the kind ignores (MoogFilter::SetDrive is a no-op): those must NOT differ."""
from __future__ import annotations

import numpy as np

import timed_cases as C
from edge_fused_cases import _voice_corners, clean_bank
from helpers import voice_configs
from test_gpu_sampler import assignments
from timed_cases import NOTE_OFF, NOTE_ON, SET_FREQ

KINDS = C.KINDS
N = 70                                   # two workgroups, six live lanes in the last
# engine.py PARAMS[voice]
CUTOFF, RES, DRIVE, ENV_AMT, F_ATTACK = 0, 1, 2, 3, 4
AMP_AMT, A_ATTACK, A_SHAPE, A_DECAY, A_SUSTAIN, A_RELEASE, PORTA = 9, 10, 11, 12, 13, 14, 15


def split_oracle(ref, calls) -> np.ndarray:
    """timed_cases.split_oracle over the calls cut at their parameter times."""
    pending, arrival, t0, sub = [], 0, 0, []
    for untimed, timed, boundary, tparams, n_frames in calls:
        for frame, op in tparams:
            assert frame % 4 == 0 and op[0] == "params"
            pending.append((t0 + frame, arrival, op))
            arrival += 1
        pending.sort(key=lambda p: (p[0], p[1]))
        due = [p for p in pending if p[0] < t0 + n_frames]
        pending = [p for p in pending if p[0] >= t0 + n_frames]
        cuts = sorted({t0} | {p[0] for p in due}) + [t0 + n_frames]
        for k, (a, b) in enumerate(zip(cuts, cuts[1:])):
            work = (list(boundary) if k == 0 else []) + [p[2] for p in due if p[0] == a]
            sub.append((untimed if k == 0 else [], timed if k == 0 else [], work, b - a))
        t0 += n_frames
    return C.split_oracle(ref, sub)


def without_params(calls):
    return [(u, t, b, [], nf) for u, t, b, _, nf in calls]


def setup(kind: str, cfg: np.ndarray, configured=None) -> C.Setup:
    n = cfg.shape[1]
    sample = kind == "voice_sample"
    return C.Setup(kind, n, cfg, list(range(n)) if configured is None else configured,
                   clean_bank() if sample else None, assignments(n) if sample else [])


def base_config(n: int = N, seed: int = 41) -> np.ndarray:
    """Ordinary configurations with audible, stable filters and envelopes of tens of milliseconds, so that a change of
    any one field inside a 64-frame block reaches the output."""
    cfg = voice_configs(np.random.default_rng(seed), n)
    cfg[CUTOFF] = np.float32(900.0) + np.float32(40.0) * np.arange(n, dtype=np.float32)
    cfg[RES] = 0.4
    cfg[DRIVE] = 2.0
    cfg[ENV_AMT] = 0.2
    cfg[AMP_AMT] = 1.0
    cfg[A_ATTACK], cfg[F_ATTACK] = 0.002, 0.002
    cfg[A_SHAPE] = 0.0
    cfg[A_SUSTAIN] = 0.8
    return cfg.astype(np.float32)


def change(cfg, who, frame, fields):
    """Timed columns at `frame` for the voices `who`: cfg's column with `fields` = {index: value or f(i)} applied (cfg is
    updated, so later changes build on it)."""
    out = []
    for i in who:
        for f, v in fields.items():
            cfg[f, i] = np.float32(v(i) if callable(v) else v)
        out.append((frame, ("params", int(i), cfg[:, i].copy())))
    return out


def notes_on(n, frame=None):
    evs = [(i, NOTE_ON, 40 + i % 40, 0.0) for i in range(n)]
    return evs if frame is None else [(frame,) + ev for ev in evs]


def cases(kind: str):
    """name -> (Setup, calls, first changed frame, changed voices, voices whose change the kind ignores)."""
    out = {}
    every = list(range(N))
    moog, sample = kind == "voice_moog", kind == "voice_sample"

    # a cutoff sweep of 16 steps in a 64-frame block: every quad, frame 0 included (set_param now)
    cfg = base_config()
    s = setup(kind, cfg.copy())
    tp = []
    for k in range(16):
        tp += change(cfg, every, 4 * k, {CUTOFF: lambda i, k=k: 500.0 + 450.0 * k + 10.0 * i})
    out["cutoff_sweep"] = (s, [(notes_on(N), [], [], tp, 64), ([], [], [], [], 64)], 0, every, [])

    # an amp-release change in mid-release: NoteOff at 16, the release time from 0.5 s to 5 ms at 32
    cfg = base_config()
    cfg[A_RELEASE] = 0.5
    s = setup(kind, cfg.copy())
    timed = [(16, i, NOTE_OFF, 0, 0.0) for i in every]
    out["release_mid_release"] = (s, [(notes_on(N), timed, [], change(cfg, every[::2], 32, {A_RELEASE: 0.005}), 64),
                                      ([], [], [], [], 64)], 32, every[::2], [])

    # an attack change in mid-attack: a 0.5 s attack, 5 ms from frame 20 on
    cfg = base_config()
    cfg[A_ATTACK] = 0.5
    s = setup(kind, cfg.copy())
    out["attack_mid_attack"] = (s, [(notes_on(N), [], [], change(cfg, every[1::2], 20, {A_ATTACK: 0.005}), 64),
                                    ([], [], [], [], 64)], 20, every[1::2], [])

    # a portamento change during a glide (the sample voice only stores its pitch: SampleSoundSource.h:28-30)
    if not sample:
        cfg = base_config()
        cfg[PORTA] = 0.05
        s = setup(kind, cfg.copy())
        timed = [(8, i, SET_FREQ, 0, 880.0 + i) for i in every]
        out["portamento_in_glide"] = (s, [(notes_on(N), timed, [], change(cfg, every[::3], 24, {PORTA: 0.002}), 64),
                                          ([], [], [], [], 64)], 24, every[::3], [])

    # resonance and drive: the resonance is live on both filters; the drive on the Svf only
    cfg = base_config()
    s = setup(kind, cfg.copy())
    tp = change(cfg, every[::2], 16, {RES: 0.85}) + change(cfg, every[1::2], 16, {DRIVE: 9.0})
    out["resonance_and_drive"] = (s, [(notes_on(N), [], [], tp, 64), ([], [], [], [], 64)], 16,
                                  every[::2] if moog else every, every[1::2] if moog else [])

    # a change and a NoteOn at the same frame, the NoteOn queued first: the parameters still precede it
    cfg = base_config()
    cfg[A_ATTACK] = 0.3
    s = setup(kind, cfg.copy())
    out["change_with_note_on"] = (s, [([], notes_on(N, 24), [], change(cfg, every, 24, {A_ATTACK: 0.001, CUTOFF: 3000.0}), 64),
                                      ([], [], [], [], 64)], 24, every, [])

    # a voice never configured (Init's component defaults) until a timed record configures it
    cfg = base_config()
    cfg[A_RELEASE], cfg[RES] = 0.01, 0.8
    s = setup(kind, cfg.copy(), configured=every[::2])
    out["configured_by_a_timed_record"] = (s, [(notes_on(N), [], [], change(cfg, every[1::2], 16, {}), 64),
                                               ([], [], [], [], 64)], 16, every[1::2], [])

    # the fp32 corner parameters of edge_fused_cases: every field at an end of its range, at frames 4 and 12
    cfg = base_config()
    corners = _voice_corners(np.random.default_rng(33), N)
    s = setup(kind, cfg.copy())
    tp = []
    for frame, who in ((4, every[::2]), (12, every[1::2])):
        for i in who:
            tp.append((frame, ("params", i, corners[:, i].copy())))
    out["fp32_corners"] = (s, [(notes_on(N), [], [], tp, 64), ([], [], [], [], 64)], 4, every, [])
    return out


CASE_NAMES = ["cutoff_sweep", "release_mid_release", "attack_mid_attack", "portamento_in_glide", "resonance_and_drive",
              "change_with_note_on", "configured_by_a_timed_record", "fp32_corners"]


def condition(name, case, yr, y0) -> None:
    """The timed change matters: nothing before its first frame, something after it for every changed voice that
    sounds there (and nothing at all for the voices whose change the kind ignores)."""
    s, calls, first, changed, ignored = case
    assert yr.shape == y0.shape == (1, sum(c[4] for c in calls), s.n)
    same = yr.view(np.uint32) == y0.view(np.uint32)
    assert same[:, :first].all(), f"{name}: differs before frame {first}"
    sounds = np.any(yr[0, first:] != 0, axis=0) | np.any(y0[0, first:] != 0, axis=0)
    who = [i for i in changed if sounds[i]]
    differs = ~same[0, first:].all(axis=0)
    print(f"\n{s.kind} {name}: {len(who)} of {len(changed)} changed voices sound; {int(differs[who].sum())} differ after frame {first}")
    assert len(who) * 3 >= len(changed), f"{name}: too few changed voices sound"
    assert differs[who].all(), f"{name}: the change is inaudible on voices {[i for i in who if not differs[i]][:8]}"
    untouched = [i for i in range(s.n) if i not in changed]
    assert not differs[untouched].any() and not differs[ignored].any()
