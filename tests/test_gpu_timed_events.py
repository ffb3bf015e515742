"""olfx_timed_events on the GPU: note events at a frame inside the block, for the three voice kinds.

The contract is the oracle: one process(N) with timed events equals, bit for bit, a fresh twin engine
that is called once per distinct event frame below N with that frame's events queued by voice_events
before the call -- in the output, and in the output of one further event-free 64-frame block, which
exposes the stored state.  `Twin` restates the queue's rules (order by frame then arrival, carry-over)
in Python and drives the twin engine with split calls.

n = 130 voices: three workgroups, two live lanes in the last.  n_frames = 64 unless stated."""
import ctypes

import numpy as np
import pytest

import ol_dsp_amd as ofx
import oracle as O
import sampler_ref as SR
from helpers import first_mismatch_or_nan, rel_err, same_bits_or_nan, voice_configs
from ol_dsp_amd import _lib, workload
from test_gpu_parity import VOICE_TOL

pytestmark = pytest.mark.gpu

N, NF = 130, 64
KINDS = ["voice", "voice_moog", "voice_sample"]
NOTE_OFF, NOTE_ON, GATE_ON, GATE_OFF, SET_FREQ = 0, 1, 2, 3, 4
# sample voices: a 20-frame one-shot on the even voices, 61-frame loops of a 1000-frame sample on the odd
# ones (a turn inside every 64-frame window), voice 7 unassigned
SAMPLE_LENGTHS = [20, 1000]


def sample_recs(n):
    recs = [(i, 0) if i % 2 == 0 else (i, 1, 1, 100 + i, 160 + i) for i in range(n)]
    if n > 7:
        recs[7] = (7, None)
    return recs


def configs(kind, n=N, seed=21):
    return voice_configs(np.random.default_rng(seed), n)


def run(e, frames, cuda, io="device"):
    if io == "host":
        return e.process(None, n_frames=frames)
    import torch
    out = torch.full((e.info.out_channels, frames, e.n), 7.0, device=cuda)        # poisoned: every word is written
    e.process(None, out=out)
    return out.cpu().numpy()


def make(kind, cfg=None, n=N):
    e = ofx.Engine(kind, n)
    e.set_params(0, configs(kind, n) if cfg is None else cfg)
    if kind == "voice_sample":
        e.sample_bank(workload.sample_bank(SAMPLE_LENGTHS, seed=11))
        e.sample_voices(sample_recs(n))
    return e


class Twin:
    """The split-call side of the contract: a pending list ordered by (frame, arrival) and an engine that
    only ever sees voice_events at a block's start."""

    def __init__(self, e):
        self.e, self.pending = e, []

    def queue(self, events):                     # (frame, inst, type[, note[, value]])
        self.pending += [tuple(ev) for ev in events]
        self.pending.sort(key=lambda ev: ev[0])  # stable: ties keep arrival order

    def run(self, frames, cuda, io="device"):
        now = [ev for ev in self.pending if ev[0] < frames]
        self.pending = [(ev[0] - frames,) + ev[1:] for ev in self.pending if ev[0] >= frames]
        cuts = sorted({0} | {ev[0] for ev in now}) + [frames]
        parts = []
        for f0, f1 in zip(cuts, cuts[1:]):
            self.e.voice_events([ev[1:] for ev in now if ev[0] == f0])
            parts.append(run(self.e, f1 - f0, cuda, io))
        return np.concatenate(parts, 1)


def assert_same(got, want, what):
    assert same_bits_or_nan(got, want), (what, first_mismatch_or_nan(got, want))


def check(kind, schedule, cuda, frames=NF, io="device", cfg=None, boundary=None, calls=1):
    """`schedule` through timed_events on one engine and through the twin; `boundary(engine, queue)` does
    the same block-boundary work on both first (queue: untimed events)."""
    a, b = make(kind, cfg), make(kind, cfg)
    t = Twin(b)
    if boundary:
        boundary(a, a.voice_events)
        boundary(b, lambda evs: t.queue([(0,) + tuple(ev) for ev in evs]))
    a.timed_events(schedule)
    t.queue(schedule)
    for c in range(calls):
        ya, yb = run(a, frames, cuda, io), t.run(frames, cuda, io)
        assert np.isfinite(yb).all()
        assert_same(ya, yb, f"call {c}")
    assert not t.pending
    assert ya.any()                                              # some voice sounded
    assert_same(run(a, 64, cuda, io), run(b, 64, cuda, io), "the stored state (a further event-free block)")
    return ya


def all_on(frame, n=N):
    return [(frame, i, NOTE_ON, 40 + i % 50) for i in range(n)]


def quads(frames, n=N):
    """One event time per listed frame, on disjoint voice subsets, the types cycling."""
    types = [NOTE_ON, NOTE_OFF, SET_FREQ, GATE_ON]
    evs = []
    for k, f in enumerate(frames):
        ty = types[k % 4]
        evs += [(f, i, ty, 36 + (i * 7) % 60, 55.0 * (1 + i % 9)) for i in range(k, n, len(frames))]
    return evs


@pytest.mark.parametrize("kind", KINDS)
def test_one_mid_chunk_time(cuda, kind):
    """NoteOn on all voices at frame 12: a segment of one full and one half chunk, then the rest."""
    check(kind, all_on(12), cuda)


@pytest.mark.parametrize("io", ["device", "host"])
@pytest.mark.parametrize("kind", KINDS)
def test_consecutive_single_quad_segments(cuda, kind, io):
    """Frames 4, 8, 12, 16: segments of one 4-frame chunk, so ENV is two segments ahead of FILT (v5) when
    it reaches the third; sounding voices first, so NoteOff and SetFrequency act on them.  Both I/O paths."""
    check(kind, all_on(0) + quads([4, 8, 12, 16]), cuda, io=io)


@pytest.mark.parametrize("kind", KINDS)
def test_last_quad(cuda, kind):
    check(kind, all_on(0)[::3] + quads([NF - 4]), cuda)


@pytest.mark.parametrize("kind", KINDS)
def test_empty_segment_0_then_crowded_groups(cuda, kind):
    """Nothing at frame 0; at frame 20 group 0 has 9 voices with events (the overflow list), group 1
    exactly 4 (the fixed slots full), group 2 none."""
    evs = [(20, i, NOTE_ON, 50 + i) for i in (0, 5, 9, 17, 18, 33, 40, 62, 63)]
    evs += [(20, 64 + i, NOTE_ON, 60 + i) for i in (0, 1, 31, 63)]
    ya = check(kind, evs, cuda)
    assert not ya[0, :20].any() and not ya[0, :, 128:].any()


@pytest.mark.parametrize("kind", KINDS)
def test_one_voice_over_time(cuda, kind):
    """NoteOn and NoteOff both at frame 8 (they fold: retriggered, gate off), NoteOn again at 24: a
    retrigger in mid-release.  Every third voice, and the last one (the dead lanes' mirror)."""
    who = sorted(set(range(0, N, 3)) | {N - 1})
    evs = [(8, i, NOTE_ON, 60) for i in who] + [(8, i, NOTE_OFF, 60) for i in who] + [(24, i, NOTE_ON, 67) for i in who]
    check(kind, evs, cuda)


@pytest.mark.parametrize("kind", KINDS)
def test_envelope_redo_path(cuda, kind):
    """Both attacks at 0 s, the shortest the kinds accept: the attack ends on the first sample after the
    NoteOn at frame 12, so the speculative full chunk that starts that segment is redone."""
    cfg = configs(kind)
    cfg[4] = 0.0
    cfg[10] = 0.0
    check(kind, all_on(12), cuda, cfg=cfg)


@pytest.mark.parametrize("kind", KINDS)
def test_every_quad(cuda, kind):
    """16 times in 64 frames: as many segments as one launch takes."""
    check(kind, quads(list(range(0, NF, 4))), cuda)


@pytest.mark.parametrize("kind", KINDS)
def test_over_the_cap(cuda, kind):
    """64 distinct times in 256 frames: more than a launch's segments, so the call runs as several."""
    check(kind, all_on(0)[::2] + quads(list(range(0, 256, 4))), cuda, frames=256)


@pytest.mark.parametrize("kind", KINDS)
def test_long_segments(cuda, kind):
    """256 frames cut at 12, 100 and 236: segments of 88 and 136 frames, so the sample voice's 64-frame fetch
    windows end inside a segment, its ring wraps, and its rows are off the frame numbers by the short chunks."""
    check(kind, all_on(12) + quads([100, 236]), cuda, frames=256)


@pytest.mark.parametrize("kind", KINDS)
def test_carry_over(cuda, kind):
    """Frames n_frames + 8 and 2 n_frames queued before call 1: call 1 has no event, call 2 one at frame 8,
    call 3 one at its frame 0."""
    evs = [(NF + 8, i, NOTE_ON, 40 + i % 40) for i in range(N)] + [(2 * NF, i, NOTE_OFF, 0) for i in range(0, N, 2)]
    check(kind, evs, cuda, calls=3)


@pytest.mark.parametrize("kind", KINDS)
def test_mixed_with_boundary_work(cuda, kind):
    """Untimed events, set_params and (sample voices) sample_voices queued before the same call as timed
    events: they land at the block boundary, ahead of frame 0's timed events."""
    cfg2 = configs(kind, seed=22)

    def boundary(e, queue):
        queue([(i, NOTE_ON, 45 + i % 30) for i in range(0, N, 2)])
        e.set_params(0, cfg2[:, 10:90], first=10)
        if kind == "voice_sample":
            e.sample_voices([(i, 1, 1, 10, 40) for i in range(0, N, 5)])
        queue([(i, SET_FREQ, 0, 330.0) for i in range(1, N, 4)])

    check(kind, [(0, i, GATE_OFF) for i in range(0, N, 4)] + quads([0, 12, 40]), cuda, boundary=boundary)


def test_sample_exhaustion_pause_and_reseek(cuda):
    """NoteOn at 12, NoteOff at 36, NoteOn at 40: the 20-frame one-shot runs out at frame 32, the loops are
    paused mid-turn, and both are sought back to 0 inside the block."""
    evs = all_on(12) + [(36, i, NOTE_OFF) for i in range(N)] + all_on(40)
    ya = check("voice_sample", evs, cuda)
    assert not ya[0, :12].any() and not ya[0, :, 7].any()


@pytest.mark.parametrize("sched", ["one_time", "single_quads"])
@pytest.mark.parametrize("kind", KINDS)
def test_against_the_cpu_reference(cuda, kind, sched):
    """Schedules 1 and 2 against the CPU reference of the kind's parity suite, called in split blocks, at
    that suite's tolerance (test_gpu_parity.py VOICE_TOL)."""
    evs = all_on(12) if sched == "one_time" else all_on(0) + quads([4, 8, 12, 16])
    e = make(kind)
    cfg = configs(kind)
    if kind == "voice_sample":
        ref = SR.SamplerVoices(N)
        ref.sample_bank(workload.sample_bank(SAMPLE_LENGTHS, seed=11))
        ref.sample_voices(sample_recs(N))
    else:
        ref = O.Voice(N, moog=kind == "voice_moog")
    for i in range(N):
        ref.config(i, cfg[:, i])
    e.timed_events(evs)
    y = np.concatenate([run(e, NF, cuda), run(e, 64, cuda)], 1)
    cuts = sorted({0} | {ev[0] for ev in evs}) + [NF]
    parts = []
    for f0, f1 in zip(cuts, cuts[1:]):
        for ev in evs:
            if ev[0] == f0:
                ref.event(ev[1], ev[2], ev[3] if len(ev) > 3 else 0, ev[4] if len(ev) > 4 else 0.0)
        parts.append(ref.process(f1 - f0))
    yr = np.concatenate(parts + [ref.process(64)], 1)
    assert np.isfinite(yr).all() and yr.any()
    err = rel_err(y[0].T, yr[0].T)
    print(f"{kind} {sched}: rel err vs the CPU reference {err:.3e}")
    assert err <= VOICE_TOL


REFUSED = [("synth", _lib.OLFX_E_KIND), ("synth_svf", _lib.OLFX_E_KIND), ("drumkit", _lib.OLFX_E_KIND),
           ("fxrack", _lib.OLFX_E_STATE), ("chorus", _lib.OLFX_E_STATE), ("meter", _lib.OLFX_E_STATE)]


@pytest.mark.parametrize("kind,code", REFUSED)
def test_other_kinds_refuse(cuda, kind, code):
    """The instrument kinds: OLFX_E_KIND; effects and meters: OLFX_E_STATE -- and the next block is what a
    twin that never made the call computes."""
    import torch
    n = 70
    a, b = ofx.Engine(kind, n), ofx.Engine(kind, n)
    arr = (_lib.TimedEvent * 1)()
    arr[0].frame, arr[0].ev.inst, arr[0].ev.type, arr[0].ev.note = 8, 1, NOTE_ON, 60
    assert a.lib.olfx_timed_events(a.handle, arr, 1) == code
    ich = a.info.in_channels
    x = torch.from_numpy(workload.noise_np(0, n, NF, ich)).to(cuda) if ich else None
    for e in (a, b):
        if a.info.in_channels == 0:
            e.note_events([(i, NOTE_ON, 36 + i % 12) for i in range(n)])
    ya = a.process(x, n_frames=NF) if x is not None else run(a, NF, cuda)
    yb = b.process(x, n_frames=NF) if x is not None else run(b, NF, cuda)
    ya, yb = (v.cpu().numpy() if hasattr(v, "cpu") else v for v in (ya, yb))
    assert_same(ya, yb, kind)


def test_bad_records_change_nothing(cuda):
    """OLFX_E_ARG for a frame that is no multiple of 4, a frame at 2^31, a voice out of range or a
    non-finite SetFrequency anywhere in the call; the good records of that call are not queued."""
    a, b = make("voice"), make("voice")
    for frame, inst, ty, val in ((6, 0, NOTE_ON, 0.0), (1 << 31, 0, NOTE_ON, 0.0), (8, N, NOTE_ON, 0.0),
                                 (8, 0, SET_FREQ, float("inf")), (8, 0, 5, 0.0)):
        arr = (_lib.TimedEvent * 2)()
        arr[0].frame, arr[0].ev.inst, arr[0].ev.type, arr[0].ev.note = 8, 3, NOTE_ON, 60
        arr[1].frame, arr[1].ev.inst, arr[1].ev.type, arr[1].ev.value = frame, inst, ty, val
        assert a.lib.olfx_timed_events(a.handle, arr, 2) == _lib.OLFX_E_ARG
    assert a.lib.olfx_timed_events(a.handle, ctypes.cast(None, ctypes.POINTER(_lib.TimedEvent)), 1) == _lib.OLFX_E_ARG
    for e in (a, b):
        e.note_events([(i, NOTE_ON, 50) for i in range(0, N, 2)])
    assert_same(run(a, NF, cuda), run(b, NF, cuda), "after refused calls")


def test_reset_drops_pending_events(cuda):
    a, b = make("voice"), make("voice")
    a.timed_events(all_on(8) + all_on(NF + 8))
    a.reset()
    b.reset()
    for e in (a, b):
        e.set_params(0, configs("voice"))
        e.note_events([(i, NOTE_ON, 50) for i in range(0, N, 2)])
    assert_same(np.concatenate([run(a, NF, cuda), run(a, NF, cuda)], 1),
                np.concatenate([run(b, NF, cuda), run(b, NF, cuda)], 1), "after reset")
