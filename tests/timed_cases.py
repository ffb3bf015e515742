"""olfx_timed_events against the oracle's kernel arithmetic: the cases as data, the split-oracle driver
that is their reference, and the condition each reference must meet.  No torch, no GPU.

tests/test_timed_ref.py runs every reference alone on the CPU and asserts its condition and the score's
facts; tests/test_gpu_timed_paths.py runs the same cases on the engine and compares bit for bit.  The
references are O.Voice(kernel_arith=True) and sampler_ref.SamplerVoices(kernel_arith=True) with the
committed v_rcp_f32 table installed (the GPU tests' rcp_table fixture, or synth_ref.install_rcp() /
remove_rcp() on the CPU).

A case is a Setup (the kind, its voices, their configurations and samples) and a list of calls
  (untimed events, timed events, boundary work, n_frames)
in the order a host makes them before one olfx_process(n_frames):
  untimed events   (inst, type, note, value)          olfx_voice_events
  timed events     (frame, inst, type, note, value)   olfx_timed_events, after the untimed ones
  boundary work    ("params", inst, column[16])       olfx_set_params of one voice
                   ("member", inst, field, value, column[16])   olfx_set_member; the column is the voice's
                                                      configuration after it (what the oracle takes)
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

import oracle as O
import sampler_ref as SMP
from edge_fused_cases import clean_bank, voice_config, voice_corner_case
from helpers import voice_configs
from test_gpu_sampler import LENGTHS, assignments

KINDS = ["voice", "voice_moog", "voice_sample"]
NOTE_OFF, NOTE_ON, GATE_ON, GATE_OFF, SET_FREQ = 0, 1, 2, 3, 4
SEG_CAP = 16                     # olfx_layout.h kSegCap: the segments of one launch
VEV_CAP = 4                      # olfx_layout.h kVevCap: a workgroup's fixed event slots per segment
SCORE_N = 130
SCORE_FRAMES = [64, 4, 12, 100, 300, 256, 20, 8]
SCORE_CALLS = 12
SCORE_SEED = {"voice": 5, "voice_moog": 5, "voice_sample": 5}
MEMBER_FIELDS = ((0, 100.0, 8000.0), (3, 0.0, 1.0), (9, 0.2, 1.0))     # test_voice_bit_exact_kernel_arith's
HZ_RANGE = (30.0, 3000.0)                                              # ... and its SetFrequency values


def _say(text: str) -> None:
    print("\n" + text)


@dataclass
class Setup:
    kind: str
    n: int
    cfg: np.ndarray                      # [16][n]
    configured: list                     # the voices that get cfg's column (the rest stay at Init's defaults)
    bank: list = None                    # voice_sample: the samples ...
    recs: list = field(default_factory=list)   # ... and olfx_sample_voices' records


def reference(s: Setup):
    """The kernel-arithmetic oracle of a setup: config(), event() and process()."""
    if s.kind == "voice_sample":
        ref = SMP.SamplerVoices(s.n, kernel_arith=True)
        ref.sample_bank(s.bank)
        ref.sample_voices(s.recs)
    else:
        ref = O.Voice(s.n, moog=s.kind == "voice_moog", kernel_arith=True)
    for i in s.configured:
        ref.config(int(i), s.cfg[:, i])
    return ref


# ------------------------------------------------------------------------------ the split-oracle driver
def split_oracle(ref, calls) -> np.ndarray:
    """The calls on the oracle, as olfx.h states the queue: events apply in order of (frame, arrival);
    untimed events are at frame 0; what a call does not reach stays, its frame reduced by the call's
    length; boundary work lands ahead of frame 0's events.  One ref.process per distinct event frame."""
    waiting, arrival, parts = [], 0, []
    for untimed, timed, boundary, n_frames in calls:
        assert n_frames > 0 and n_frames % 4 == 0
        for op in boundary:
            ref.config(int(op[1]), op[-1])
        for ev in untimed:
            waiting.append([0, arrival, ev])
            arrival += 1
        for ev in timed:
            assert ev[0] % 4 == 0
            waiting.append([ev[0], arrival, ev[1:]])
            arrival += 1
        waiting.sort(key=lambda w: (w[0], w[1]))
        at = 0
        while at < n_frames:
            while waiting and waiting[0][0] == at:
                inst, ty, note, value = waiting.pop(0)[2]
                ref.event(int(inst), int(ty), int(note), float(value) if ty == SET_FREQ else 0.0)
            until = min(n_frames, waiting[0][0]) if waiting else n_frames
            parts.append(ref.process(until - at))
            at = until
        for w in waiting:
            w[0] -= n_frames
    return np.concatenate(parts, 1)


def recut(calls, lengths):
    """The same score in calls of other lengths: the same total, every event at its absolute time and in its
    order of arrival, queued before the last new call that starts at or before the call it was queued
    before, its frame counted from there (an untimed event becomes a timed one where that is no new
    boundary).  Boundary work needs its boundary: a new call must start there."""
    assert sum(lengths) == sum(c[3] for c in calls)
    starts = np.concatenate([[0], np.cumsum(lengths)[:-1]]).tolist()
    out = [([], [], [], int(m)) for m in lengths]
    t0 = 0
    for untimed, timed, boundary, n_frames in calls:
        j = max(k for k, s in enumerate(starts) if s <= t0)
        if boundary:
            assert starts[j] == t0, "no new call starts at this boundary work"
            out[j][2].extend(boundary)
        for ev in untimed:
            out[j][1].append((t0 - starts[j],) + tuple(ev))
        for ev in timed:
            out[j][1].append((t0 + ev[0] - starts[j],) + tuple(ev[1:]))
        t0 += n_frames
    return out


def recut_lengths(calls, piece=None):
    """piece = None: as few calls as the boundary work allows; else: every call in pieces of at most `piece`."""
    if piece is not None:
        return [min(piece, c[3] - f) for c in calls for f in range(0, c[3], piece)]
    lengths = []
    for k, c in enumerate(calls):
        if k == 0 or c[2]:
            lengths.append(c[3])
        else:
            lengths[-1] += c[3]
    return lengths


# ------------------------------------------------------------------------------------------ the score
def score(kind: str, n: int = SCORE_N, seed: int = None):
    """(Setup, calls): SCORE_CALLS calls of 64, 4, 12, 100, 300, 256, 20, 8, ... frames.  Before each, timed
    events of all five types on about 30 % of the voices at multiples of 4 below 2.5 call lengths (some
    carry over); untimed events before calls 0 (NoteOn on every voice), 3, 6 and 9; before call 5 a new
    configuration for a third of the configured voices, before call 8 three olfx_set_member writes on
    40 of them.  voice, voice_moog: the odd voices are never configured.  voice_sample:
    test_gpu_sampler's bank and assignments."""
    rng = np.random.default_rng([SCORE_SEED[kind] if seed is None else seed, KINDS.index(kind), n])
    cfg = voice_configs(rng, n)
    sample = kind == "voice_sample"
    conf = list(range(n)) if sample else list(range(0, n, 2))
    s = Setup(kind, n, cfg.copy(), conf, clean_bank() if sample else None, assignments(n) if sample else [])

    def event(i):
        return (int(i), int(rng.integers(0, 5)), int(rng.integers(30, 100)), float(np.float32(rng.uniform(*HZ_RANGE))))

    calls = []
    for c in range(SCORE_CALLS):
        nf = SCORE_FRAMES[c % len(SCORE_FRAMES)]
        boundary, untimed = [], []
        if c == 5:
            new = voice_configs(rng, n)
            for i in conf:
                if rng.random() < 1 / 3:
                    cfg[:, i] = new[:, i]
                    boundary.append(("params", i, cfg[:, i].copy()))
        if c == 8:
            for i in conf[:40]:
                for f, lo, hi in MEMBER_FIELDS:
                    cfg[f, i] = np.float32(rng.uniform(lo, hi))
                    boundary.append(("member", i, f, float(cfg[f, i]), cfg[:, i].copy()))
        if c == 0:
            untimed = [(i, NOTE_ON, int(rng.integers(30, 100)), 0.0) for i in range(n)]
        elif c % 3 == 0:
            untimed = [event(i) for i in np.flatnonzero(rng.random(n) < 0.2)]
        timed = [(4 * int(rng.integers(0, (5 * nf + 7) // 8)),) + event(i) for i in np.flatnonzero(rng.random(n) < 0.3)]
        calls.append((untimed, timed, boundary, nf))
    return s, calls


def launches(calls):
    """What the engine makes of the calls, by the header's rules alone: per call, its launches; per launch, its
    segments as (start frame, [events in order]) -- segment 0 starts at frame 0 with or without events, and a
    launch ends ahead of the first event time that would be its segment SEG_CAP + 1."""
    waiting, arrival, out = [], 0, []
    for untimed, timed, _, n_frames in calls:
        for ev in untimed:
            waiting.append([0, arrival, tuple(ev), 0])
            arrival += 1
        for ev in timed:
            waiting.append([ev[0], arrival, tuple(ev[1:]), 0])
            arrival += 1
        waiting.sort(key=lambda w: (w[0], w[1]))
        due = [w for w in waiting if w[0] < n_frames]
        waiting = [w for w in waiting if w[0] >= n_frames]
        segs = [(0, [])]
        for w in due:
            if w[0] != segs[-1][0]:
                segs.append((w[0], []))
            segs[-1][1].append((w[2], w[3]))
        out.append([segs[k:k + SEG_CAP] for k in range(0, len(segs), SEG_CAP)])
        for w in waiting:
            w[0] -= n_frames
            w[3] += 1                                # calls carried over
    return out


def score_facts(calls) -> dict:
    """Counts of what the score is meant to contain (tests/test_timed_ref.py asserts each is at least 1)."""
    per_call = launches(calls)
    facts = dict(calls_over_the_cap=0, single_quad_runs=0, carried_two_calls=0, crowded_twice=0, setfreq_after_noteon=0,
                 most_launches=0)
    for (_, _, _, n_frames), ls in zip(calls, per_call):
        times = sum(len(l) for l in ls) - (0 if ls[0][0][1] else 1)          # distinct event frames
        facts["calls_over_the_cap"] += times > SEG_CAP
        facts["most_launches"] = max(facts["most_launches"], len(ls))
        last_on = set()
        starts = [sg[0] for l in ls for sg in l] + [n_frames]
        lens = [b - a for a, b in zip(starts, starts[1:])]                   # every segment's frames, in order
        first = 0
        for l in ls:
            mine = lens[first:first + len(l)]
            first += len(l)
            facts["single_quad_runs"] += any(mine[k:k + 3] == [4, 4, 4] for k in range(len(mine) - 2))
            crowded = {}
            for sg in l:
                voices = {}
                for (inst, ty, _, _), carried in sg[1]:
                    voices.setdefault(inst >> 6, set()).add(inst)
                    facts["carried_two_calls"] += carried >= 2
                    if ty == NOTE_ON:
                        last_on.add(inst)
                    facts["setfreq_after_noteon"] += ty == SET_FREQ and inst in last_on
                for g, v in voices.items():
                    crowded[g] = crowded.get(g, 0) + (len(v) > VEV_CAP)
            facts["crowded_twice"] += any(c >= 2 for c in crowded.values())
    return {k: int(v) for k, v in facts.items()}


def score_condition(kind: str, yr: np.ndarray) -> None:
    """Finite on more than 90 % of the samples (test_voice_bit_exact_kernel_arith's bar) and at least half
    the voices non-silent."""
    fin, sounding = float(np.isfinite(yr).mean()), float(np.mean(np.any(yr[0] != 0, axis=0)))
    _say(f"{kind} score: reference finite on {100 * fin:.1f} % of the samples, {100 * sounding:.0f} % of the voices non-silent")
    assert fin > 0.9 and sounding >= 0.5


# ------------------------------------------------------------------------------------------- corners
CORNER_HZ_SEED = 34


def corner_case(kind: str):
    """(Setup, calls): n = 256, every field at an end of its range, notes from {0, 1, 21, 60, 108, 127}
    (test_voice_corners' draw; the sample voice: edge_fused_cases.voice_corner_case).  One call of 64 frames --
    NoteOn at 12, SetFrequency at 20 on every second voice (in portamento from the NoteOn), NoteOff at 36,
    NoteOn at 40 (a retrigger in mid-release), GateOff at 44, GateOn at 48 -- and one event-free call."""
    if kind == "voice_sample":
        n, cfg, script = voice_corner_case()
        notes = [ev[2] for ev in script[0][1]]
        s = Setup(kind, n, cfg, list(range(n)), clean_bank(), assignments(n))
    else:
        n = 256
        rng = np.random.default_rng(33)
        cfg = rng.integers(0, 2, (16, n)).astype(np.float32)
        cfg[0] *= 20000.0
        notes = [int(v) for v in rng.choice([0, 1, 21, 60, 108, 127], n)]
        s = Setup(kind, n, cfg, list(range(n)))
    assert len(notes) == n and set(notes) == {0, 1, 21, 60, 108, 127}
    hz = np.random.default_rng(CORNER_HZ_SEED).uniform(*HZ_RANGE, n).astype(np.float32)
    every = range(n)
    timed = [(12, i, NOTE_ON, notes[i], 0.0) for i in every]
    timed += [(20, i, SET_FREQ, 0, float(hz[i])) for i in every if i % 2 == 0]
    timed += [(36, i, NOTE_OFF, notes[i], 0.0) for i in every]
    timed += [(40, i, NOTE_ON, notes[i], 0.0) for i in every]
    timed += [(44, i, GATE_OFF, 0, 0.0) for i in every]
    timed += [(48, i, GATE_ON, 0, 0.0) for i in every]
    return s, [([], timed, [], 64), ([], [], [], 64)]


def corner_condition(kind: str, yr: np.ndarray) -> None:
    """Finite throughout, and at least a third of the voices sound (test_voice_corners' bar)."""
    sounding = float(np.mean(np.any(yr[0] != 0, axis=0)))
    _say(f"{kind} timed corners: reference finite on {100 * np.isfinite(yr).mean():.1f} % of the samples, "
         f"{100 * sounding:.0f} % of the voices non-silent")
    assert np.all(np.isfinite(yr)) and sounding >= 1 / 3


# --------------------------------------------------------------------------------------- the sampler case
SAMPLER_N = 130


def sampler_case():
    """(Setup, calls): test_gpu_sampler's bank and assignments at n = 130.  One call of 256 frames: NoteOn on every
    voice at 0; NoteOff on the voices i % 3 == 0 at 8 and their NoteOn at 12, i % 3 == 1 at 12 and 16, i % 3 == 2
    at 16 and 20.  Every sample length and loop mode is paused for one 4-frame segment, sought back to 0 and
    replayed inside single-quad segments, then runs through four 64-frame fetch windows."""
    n = SAMPLER_N
    s = Setup("voice_sample", n, voice_config(n), list(range(n)), clean_bank(), assignments(n))
    note = [40 + i % 50 for i in range(n)]
    timed = [(0, i, NOTE_ON, note[i], 0.0) for i in range(n)]
    for third, f in enumerate((8, 12, 16)):
        who = range(third, n, 3)
        timed += [(f, i, NOTE_OFF, note[i], 0.0) for i in who] + [(f + 4, i, NOTE_ON, note[i], 0.0) for i in who]
    return s, [([], timed, [], 256)]


def sampler_condition(s: Setup, yr: np.ndarray) -> None:
    """Finite, every assigned voice non-silent (and every unassigned one silent)."""
    assigned = [r[0] for r in s.recs if r[1] is not None]
    idle = [r[0] for r in s.recs if r[1] is None]
    sounding = np.any(yr[0] != 0, axis=0)
    _say(f"voice_sample timed bank: reference finite on {100 * np.isfinite(yr).mean():.1f} % of the samples, "
         f"{int(sounding[assigned].sum())} of {len(assigned)} assigned voices non-silent")
    assert {r[1] for r in s.recs} == set(range(len(LENGTHS))) | {None}
    assert np.all(np.isfinite(yr)) and np.all(sounding[assigned]) and not np.any(sounding[idle])
