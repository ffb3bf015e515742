"""olfx_timed_events on the GPU beyond tests/test_gpu_timed_events.py's corner: the segmented kernels
against the oracle's kernel arithmetic (tests/timed_cases.py: a seeded score with carry-over, boundary
work, unconfigured voices and member writes; corner configurations; the sampler suite's bank inside
4-frame segments), the copied packets' big slots and the zero-copy slot ring wrapping inside one
olfx_process, ragged and large voice counts, stream switches with events pending, a refused
olfx_process, and the containment of the segmented kernels' stores.  Every comparison is bit for bit:
against the oracle with voice_bits_equal, against the twin engine driven by split calls (Twin) with
same_bits_or_nan, there also in one further event-free block, which exposes the stored state."""
import ctypes

import numpy as np
import pytest

import ol_dsp_amd as ofx
import timed_cases as C
from helpers import first_mismatch
from ol_dsp_amd import _lib, workload
from test_gpu_edges import _assert_contained, _guarded_numpy, _guarded_torch
from test_gpu_parity import voice_bits_equal
from test_gpu_timed_events import (KINDS, N, SAMPLE_LENGTHS, Twin, all_on, assert_same, configs, make, quads, run,
                                   sample_recs)

pytestmark = pytest.mark.gpu

NOTE_OFF, NOTE_ON = C.NOTE_OFF, C.NOTE_ON
KSLOTS = 16                       # olfx_engine::kSlots: the zero-copy control slots


# ------------------------------------------------------------------------------------ the engine side
def engine_for(s: C.Setup):
    e = ofx.Engine(s.kind, s.n)
    if len(s.configured) == s.n:
        e.set_params(0, s.cfg)
    else:
        for i in s.configured:
            e.set_params(0, s.cfg[:, i:i + 1], first=int(i))
    if s.kind == "voice_sample":
        e.sample_bank(s.bank)
        e.sample_voices(s.recs)
    return e


def drive(e, calls, cuda):
    """The calls of a case (timed_cases.py) on the engine: device I/O into a poisoned `out`."""
    parts = []
    for untimed, timed, boundary, n_frames in calls:
        for op in boundary:
            if op[0] == "params":
                e.set_params(0, np.asarray(op[2], np.float32)[:, None], first=int(op[1]))
            else:
                assert e.lib.olfx_set_member(e.handle, int(op[1]), int(op[2]), float(op[3])) == 0
        e.voice_events(untimed)
        e.timed_events(timed)
        parts.append(run(e, n_frames, cuda))
    return np.concatenate(parts, 1)


def against_oracle(s, calls, cuda, yr=None):
    yr = C.split_oracle(C.reference(s), calls) if yr is None else yr
    y = drive(engine_for(s), calls, cuda)
    assert voice_bits_equal(y, yr), first_mismatch(y, yr)
    return y


def five(evs):
    """(frame, inst, type[, note[, value]]) -> timed_cases' five-tuples."""
    return [(tuple(ev) + (0, 0.0))[:5] for ev in evs]


def the_suites_setup(kind, n=N):
    """What test_gpu_timed_events.make(kind) configures, as a timed_cases.Setup."""
    sample = kind == "voice_sample"
    return C.Setup(kind, n, configs(kind, n), list(range(n)),
                   workload.sample_bank(SAMPLE_LENGTHS, seed=11) if sample else None, sample_recs(n) if sample else [])


def against_twin(a, t, calls, cuda, io="device"):
    """calls = [(schedule, n_frames)]: each schedule queued on both sides before its call; then one
    event-free block of 64 frames on both engines."""
    sounded = False
    for c, (sched, frames) in enumerate(calls):
        a.timed_events(sched)
        t.queue(sched)
        ya, yb = run(a, frames, cuda, io), t.run(frames, cuda, io)
        assert_same(ya, yb, f"call {c} of {frames} frames")
        sounded = sounded or bool(ya.any())
    assert not t.pending and sounded
    assert_same(run(a, 64, cuda, io), run(t.e, 64, cuda, io), "the stored state (a further event-free block)")


# ---------------------------------------------------------- against the kernel-arithmetic oracle, bit for bit
@pytest.mark.parametrize("kind", KINDS)
def test_score_vs_oracle(cuda, rcp_table, kind):
    """The score at n = 130 (three workgroups): 12 calls of 4 to 300 frames, events of all five types carried
    over up to two calls, four calls that run as two launches, a new configuration and member writes at two
    boundaries, and (voice, voice_moog) the odd voices at Init's defaults throughout."""
    s, calls = C.score(kind)
    yr = C.split_oracle(C.reference(s), calls)
    C.score_condition(kind, yr)
    against_oracle(s, calls, cuda, yr)


@pytest.mark.parametrize("kind", KINDS)
def test_corners_vs_oracle(cuda, rcp_table, kind):
    """n = 256, every field at an end of its range, notes 0 to 127: NoteOn at 12, SetFrequency in portamento at
    20, NoteOff at 36, a retrigger in mid-release at 40, GateOff at 44, GateOn at 48; then an event-free call."""
    s, calls = C.corner_case(kind)
    yr = C.split_oracle(C.reference(s), calls)
    C.corner_condition(kind, yr)
    against_oracle(s, calls, cuda, yr)


def test_sampler_bank_vs_oracle(cuda, rcp_table):
    """The sampler suite's bank (samples of 1 to 1000 frames, the nine loop modes, loops of 1, 2, 7, 8 and 9
    frames): every voice paused, sought to 0 and replayed inside single-quad segments, then through four fetch
    windows.  Against the oracle, and against the twin."""
    s, calls = C.sampler_case()
    yr = C.split_oracle(C.reference(s), calls)
    C.sampler_condition(s, yr)
    y = against_oracle(s, calls, cuda, yr)
    a, t = engine_for(s), Twin(engine_for(s))
    a.timed_events(calls[0][1])
    t.queue(calls[0][1])
    ya, yb = run(a, 256, cuda), t.run(256, cuda)
    assert_same(ya, yb, "the twin")
    assert_same(ya, y, "a second engine")
    assert_same(run(a, 64, cuda), run(t.e, 64, cuda), "the stored state")


def ring_schedule(n, times, first_frame=0, step=4):
    """One event time every `step` frames: time k on the voices k and k + n / 2 (mod n), so that any number of times
    finds voices at any n; the types cycling as quads'."""
    types = [NOTE_ON, NOTE_OFF, C.SET_FREQ, C.GATE_ON]
    evs = []
    for k in range(times):
        for i in sorted({k % n, (k + n // 2) % n}):
            evs.append((first_frame + step * k, i, types[k % 4], 36 + (i * 7) % 60, 55.0 * (1 + i % 9)))
    return evs


@pytest.mark.parametrize("kind", KINDS)
def test_slot_ring_wraps_in_one_call(cuda, rcp_table, kind):
    """272 event times in one call of 1088 frames: 17 launches, each with a packet of its own, one more than
    the engine has zero-copy slots -- the last launch's packet waits for the first one's readers.  A second such
    call is queued up front as carry-over and made without any synchronisation after the first."""
    import torch
    frames, times = 1088, 272
    assert times == frames // 4 and -(-times // C.SEG_CAP) == KSLOTS + 1
    sched = five(all_on(0)) + ring_schedule(N, times) + ring_schedule(N, times, frames)
    calls = [([], sched, [], frames), ([], [], [], frames)]
    assert [len(ls) for ls in C.launches(calls)] == [KSLOTS + 1, KSLOTS + 1]
    yr = C.split_oracle(C.reference(the_suites_setup(kind)), calls)
    assert yr.any()
    e = make(kind)
    e.timed_events(sched)
    outs = [torch.full((1, frames, N), 7.0, device=cuda) for _ in calls]
    torch.cuda.synchronize()
    for out in outs:
        e.process(None, out=out)
    torch.cuda.synchronize()
    y = np.concatenate([o.cpu().numpy() for o in outs], 1)
    assert voice_bits_equal(y, yr), first_mismatch(y, yr)
    assert e.frames_processed == 2 * frames


# ------------------------------------------------------------------------------- against the twin, bit for bit
@pytest.mark.parametrize("n", [1, 63, 64, 65])
@pytest.mark.parametrize("kind", KINDS)
def test_ragged_voice_counts(cuda, kind, n):
    """One voice, a wave short of one lane, a full workgroup, one voice past it: consecutive single-quad
    segments; and calls of 4, 12 and 20 frames, of which the first has nothing to do and carries everything."""
    against_twin(make(kind, n=n), Twin(make(kind, n=n)), [(all_on(0, n) + quads([4, 8, 12, 16], n), 64)], cuda)
    against_twin(make(kind, n=n), Twin(make(kind, n=n)), [(all_on(12, n), 4), ([], 12), ([], 20)], cuda)


@pytest.mark.parametrize("kind", KINDS)
def test_copied_packets(cuda, monkeypatch, kind):
    """OLFX_COPY_BYTES=0 on the engine under test: every packet, segment tables included, is copied through one of
    the two big slots and read from its device half.  An over-the-cap call is four launches, so the third
    packet waits for the first one's readers; then 16 segments in one launch."""
    t = Twin(make(kind))
    monkeypatch.setenv("OLFX_COPY_BYTES", "0")
    a = make(kind)
    monkeypatch.delenv("OLFX_COPY_BYTES")
    over_the_cap = all_on(0)[::2] + quads(list(range(0, 256, 4)))
    assert [len(ls) for ls in C.launches([([], five(over_the_cap), [], 256)])] == [4]
    against_twin(a, t, [(over_the_cap, 256), (quads(list(range(0, 64, 4))), 64)], cuda)


@pytest.mark.parametrize("n", [8230, 32838])
@pytest.mark.parametrize("kind", KINDS)
def test_large_packets_by_size(cuda, kind, n):
    """128 full workgroups and 38 voices, and 513 workgroups and 6 voices: a segment with a record for every voice
    is past the 64 KiB from which a packet is copied, without any override; six segments in the launch."""
    assert 8 * n >= 65536                                        # one all-voices segment's overflow records, bytes
    sched = all_on(12, n) + [(24, i, NOTE_OFF) for i in range(n)] + quads([4, 40, 60], n)
    assert [[len(l) for l in ls] for ls in C.launches([([], five(sched), [], 64)])] == [[6]]
    against_twin(make(kind, n=n), Twin(make(kind, n=n)), [(sched, 64)], cuda)


@pytest.mark.parametrize("kind", KINDS)
def test_stream_switches_with_events_pending(cuda, kind):
    """Six calls on the engine's own stream, a second torch stream and the null stream in turn, no ordering and
    no wait from the caller, the whole score queued before the first: events stay pending across every
    switch, and the third call (256 frames, an event time on every quad) runs as several launches on its
    stream.  The twin makes its split calls on one stream."""
    import torch
    lengths = [64, 20, 256, 12, 64, 64]
    starts = np.concatenate([[0], np.cumsum(lengths)]).tolist()
    sched = all_on(0) + quads(list(range(starts[2], starts[3], 4)) + [8, 40, 72, 344, 348, 360, 400, 472])
    per_call = C.launches([([], five(sched), [], lengths[0])] + [([], [], [], m) for m in lengths[1:]])
    assert [len(ls) for ls in per_call] == [1, 1, 4, 1, 1, 1]
    a, t = make(kind), Twin(make(kind))
    side = torch.cuda.Stream(cuda)
    streams = [a.lib.olfx_stream(a.handle) or 0, side.cuda_stream, 0]
    assert len(set(streams)) == 3
    outs = [torch.full((1, m, N), 7.0, device=cuda) for m in lengths]
    torch.cuda.synchronize()
    a.timed_events(sched)
    for c, out in enumerate(outs):
        a.process(None, out=out, stream=streams[c % 3])
    torch.cuda.synchronize()
    t.queue(sched)
    for c, m in enumerate(lengths):
        assert_same(outs[c].cpu().numpy(), t.run(m, cuda), f"call {c} of {m} frames")
    assert not t.pending and a.frames_processed == starts[-1]
    assert_same(run(a, 64, cuda), run(t.e, 64, cuda), "the stored state")


def test_refused_process_keeps_the_queue(cuda):
    """olfx_process with n_frames = 6 and with out = NULL is OLFX_E_ARG and leaves the pending list alone: the next
    valid calls equal the twin that never made the refused ones."""
    import torch
    a, t = make("voice"), Twin(make("voice"))
    sched = all_on(0)[::2] + quads([8, 20, 64, 72])
    a.timed_events(sched)
    t.queue(sched)
    out = torch.full((1, 64, N), 7.0, device=cuda)
    s0 = ctypes.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)
    assert a.lib.olfx_process(a.handle, None, ctypes.c_void_p(out.data_ptr()), 6, _lib.IO_DEVICE, s0) == _lib.OLFX_E_ARG
    assert a.lib.olfx_process(a.handle, None, None, 64, _lib.IO_DEVICE, s0) == _lib.OLFX_E_ARG
    assert a.lib.olfx_process(a.handle, None, None, 64, _lib.IO_HOST, s0) == _lib.OLFX_E_ARG
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and a.frames_processed == 0
    against_twin(a, t, [([], 64), ([], 64)], cuda)


# ------------------------------------------------------------------------------------------------ containment
CONTAIN_CALLS = [4, 20, 260]


@pytest.mark.parametrize("io", ["device", "host"])
@pytest.mark.parametrize("n", [1, 63, 70, 72])
@pytest.mark.parametrize("kind", KINDS)
def test_segmented_stores_contained(cuda, kind, n, io):
    """`out` is a view into a larger buffer with 64 sentinel floats on each side, at offset 0 and at offset 1 (off
    16-byte alignment): calls of 4, 20 and 260 frames with an event time on every third quad (the last call
    runs as two launches, the second writing from row 192 on).  The guards keep their bits, every float of `out`
    is written, and the output is the twin's."""
    import torch
    cfg = configs(kind, n)
    cfg[2] *= 0.25                       # moderate Svf drive: finite, so the sentinel NaN is unmistakable
    for offset in (0, 1):
        a, t = make(kind, cfg, n), Twin(make(kind, cfg, n))
        for c, b in enumerate(CONTAIN_CALLS):
            sched = (all_on(0, n) if c == 0 else []) + ring_schedule(n, -(-b // 12), step=12)
            a.timed_events(sched)
            t.queue(sched)
            if io == "device":
                buf, view = _guarded_torch(b * n, offset, cuda)
                a.process(None, out=view.view(1, b, n))
                torch.cuda.synchronize()
                ya = view.view(1, b, n).cpu().numpy()
            else:
                buf, view = _guarded_numpy(b * n, offset)
                out = view.reshape(1, b, n)
                assert a.process(None, out=out) is out and np.shares_memory(out, buf)
                ya = out.copy()
            _assert_contained(buf, offset, b * n)
            yb = t.run(b, cuda, io)
            assert np.isfinite(yb).all() and yb.any()
            assert_same(ya, yb, f"offset {offset}, call of {b} frames")
        assert not t.pending
