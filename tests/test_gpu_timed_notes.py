"""olfx_timed_notes on the GPU: notes at a frame inside the block for OLFX_KIND_SYNTH, OLFX_KIND_SYNTH_SVF and
OLFX_KIND_DRUMKIT (synth_block_v1_seg, synth_svf_block_v1_seg, drumkit_block_v1_seg).

The contract is the oracle: a timed script on one engine equals, bit for bit, a twin engine driven by the split
calls tests/timed_note_cases.py resolve() makes of it -- one process call per distinct event frame with that
frame's notes handed to olfx_note_events before it -- in the output, in one further event-free 64-frame call (the
stored state) and in Engine.playing after every call.  The cases are that module's; n = 130 unless stated: three
groups, two live lanes in the last, whose second delay wave exits.  The same cases at n = 65 are compared with the
composed CPU references as well."""
import ctypes

import numpy as np
import pytest

import ol_dsp_amd as ofx
import timed_note_cases as C
from helpers import first_mismatch
from ol_dsp_amd import _lib
from synth_ref import bits_equal
from test_gpu_drumkit import apply as kit_apply
from test_gpu_edges import _assert_contained, _guarded_numpy, _guarded_torch

pytestmark = pytest.mark.gpu

N = 130
ON, OFF = C.NOTE_ON, C.NOTE_OFF


def make(kind, n, voices):
    return ofx.Engine(kind, n, voices=voices)


def block(e, frames, cuda, io="device", stream=None):
    if io == "host":
        return e.process(None, out=np.full((2, frames, e.n), 7.0, np.float32)).copy()
    import torch
    out = torch.full((2, frames, e.n), 7.0, device=cuda)        # poisoned: every word is written
    e.process(None, out=out, stream=stream)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def run_engine(kind, script, n, voices, cuda, timed=True, io="device", e=None):
    """The timed script on an engine (timed = False: the split calls it resolves into):
    ([2][frames][n], [Playing() [n][voices] at each check_playing step], the engine)."""
    e = make(kind, n, voices) if e is None else e
    out, tables = [], []
    for step in (script if timed else C.resolve(script)):
        op = step[0]
        if op == "timed":
            e.timed_notes(step[1])
        elif op == "block":
            out.append(block(e, step[1], cuda, io))
        elif op == "check_playing":
            tables.append(np.array([e.playing(i) for i in range(n)]))
        elif kind == "drumkit":
            kit_apply(e, step, voices)
        elif op == "params":
            e.set_params(0, step[1])
        elif op == "events":
            e.note_events(step[1])
        elif op == "set":
            e.set_param(step[1], step[2], step[3])
        elif op == "control":
            e.control(step[1])
        else:
            raise ValueError(op)
    return (np.concatenate(out, 1) if out else None), tables, e


def against_twin(kind, script, n, voices, cuda, io="device"):
    ya, pa, a = run_engine(kind, script, n, voices, cuda, True, io)
    yb, pb, b = run_engine(kind, script, n, voices, cuda, False, io)
    assert np.isfinite(yb).all() and yb[0].any(axis=0).all()     # every instrument sounded
    assert np.array_equal(ya.view(np.uint32), yb.view(np.uint32)), first_mismatch(ya, yb)
    assert len(pa) == len(pb) >= 1
    for k, (ta, tb) in enumerate(zip(pa, pb)):
        assert np.array_equal(ta, tb), (k, np.argwhere(ta != tb)[:4])
    assert a.frames_processed == b.frames_processed
    return ya, pa


# ------------------------------------------------------------------------------ against the split-call twin
@pytest.mark.parametrize("case", ["sparse", "all_on"])
@pytest.mark.parametrize("voices", [1, 4, 5, 8])
@pytest.mark.parametrize("kind", C.KINDS)
def test_event_frames_by_voices(cuda, kind, voices, case):
    """Event frames 4, 12, 16, 20, 36 and 60 (sparse: records in the fixed slots) and NoteOns on every voice at one
    frame (all_on: the overflow list) at P = 1, 4, 5 (V wave 0 runs two voices) and 8."""
    build = C.case_sparse if case == "sparse" else C.case_all_on
    against_twin(kind, build(kind, N, voices), N, voices, cuda)


@pytest.mark.parametrize("n", [1, 33, 64, 65])
@pytest.mark.parametrize("kind", C.KINDS)
def test_event_frames_by_instruments(cuda, kind, n):
    """One lane, the second delay wave just on, one full group, a group of one."""
    against_twin(kind, C.case_sparse(kind, n, 4), n, 4, cuda)
    against_twin(kind, C.case_all_on(kind, n, 4), n, 4, cuda)


@pytest.mark.parametrize("kind", ["synth", "synth_svf"])
def test_voice_allocation_over_time(cuda, kind):
    """A NoteOn with no free voice at its frame is dropped; one that follows a NoteOff takes the freed voice."""
    _, tables = against_twin(kind, C.case_allocation(kind, N), N, 2, cuda)
    for t, want in zip(tables, C.ALLOCATION_PLAYING):
        assert np.array_equal(t, np.tile(want, (N, 1)))


@pytest.mark.parametrize("kind", C.KINDS)
def test_carry_over_three_calls(cuda, kind):
    """Notes at frame == N and 2 N + 8, an untimed note between the calls: Playing() after every call."""
    _, tables = against_twin(kind, C.case_carry(kind, N, 4), N, 4, cuda)
    if kind != "drumkit":
        assert not tables[0][:, 0].any() and np.all(tables[1][:, 0] == 82) and np.all(tables[3][:, 3] == 81)


@pytest.mark.parametrize("io", ["device", "host"])
@pytest.mark.parametrize("kind", C.KINDS)
def test_seventeen_times_in_one_call(cuda, kind, io):
    """Two launches in one 128-frame call: the second writes rows 64 .. 127 of both planes, and channel 1's lie a
    128-frame plane from channel 0's, with device and with host I/O."""
    script = C.case_seventeen(kind, N, 4)
    ya, _ = against_twin(kind, script, N, 4, cuda, io)
    assert ya[0, 64:128].any() and ya[1, 64:128, 1::2].any()     # (odd instruments: topology 1 in every kind)


@pytest.mark.parametrize("kind", C.KINDS)
def test_stream_switch_with_notes_pending(cuda, kind):
    """The carry-over case with its calls on the engine's own stream, a second torch stream and the null stream in
    turn, no ordering and no wait from the caller: the pending notes cross every switch."""
    import torch
    script = C.case_carry(kind, N, 4)
    a = make(kind, N, 4)
    side = torch.cuda.Stream(cuda)
    streams = [a.lib.olfx_stream(a.handle) or 0, side.cuda_stream, 0]
    assert len(set(streams)) == 3
    outs = [torch.full((2, s[1], N), 7.0, device=cuda) for s in script if s[0] == "block"]
    torch.cuda.synchronize()
    c = 0
    for step in script:
        if step[0] == "timed":
            a.timed_notes(step[1])
        elif step[0] == "block":
            a.process(None, out=outs[c], stream=streams[c % 3])
            c += 1
        elif step[0] == "events":
            a.note_events(step[1])
        elif step[0] != "check_playing":
            kit_apply(a, step, 4) if kind == "drumkit" else a.set_params(0, step[1])
    torch.cuda.synchronize()
    ya = np.concatenate([o.cpu().numpy() for o in outs], 1)
    yb, _, _ = run_engine(kind, script, N, 4, cuda, timed=False)
    assert np.array_equal(ya.view(np.uint32), yb.view(np.uint32)), first_mismatch(ya, yb)


@pytest.mark.parametrize("kind", C.KINDS)
def test_copied_packets(cuda, kind, monkeypatch):
    """OLFX_COPY_BYTES=0: every packet goes through the two big slots and is copied to the device, so the segment
    table and the records are read from device memory; the 17-times call is two launches, two packets."""
    script = C.case_seventeen(kind, N, 4)
    yb, pb, _ = run_engine(kind, script, N, 4, cuda, timed=False)
    monkeypatch.setenv("OLFX_COPY_BYTES", "0")
    a = make(kind, N, 4)
    monkeypatch.delenv("OLFX_COPY_BYTES")
    ya, pa, _ = run_engine(kind, script, N, 4, cuda, e=a)
    assert np.array_equal(ya.view(np.uint32), yb.view(np.uint32)), first_mismatch(ya, yb)
    assert all(np.array_equal(ta, tb) for ta, tb in zip(pa, pb))


def test_kit_map_change_with_notes_pending(cuda):
    _, tables = against_twin("drumkit", C.case_kit_map_change(N), N, 4, cuda)
    assert np.array_equal(tables[1][1::2], tables[0][1::2])
    assert all(tables[1][i, 1] == C.DK.snote(i, 0) for i in range(0, N, 2))


def test_kit_pads_retriggered_inside_a_chunk(cuda):
    """Frames 4 and 12 on the 20-frame one-shots and on the 61-frame loops, which turn inside that chunk."""
    against_twin("drumkit", C.case_kit_retrigger(N), N, 4, cuda)


@pytest.mark.parametrize("kind", ["synth_svf", "drumkit"])
def test_topologies_mixed_in_one_engine(cuda, kind):
    script = C.case_sparse(kind, 70, 4)
    ya, _ = against_twin(kind, script, 70, 4, cuda)
    assert not ya[1, :, 0::2].any() and ya[1, :, 1::2].any(axis=0).all()     # 0.0f x master | the reverb's channel


def test_reset_drops_pending_notes(cuda):
    a, b = make("synth", N, 4), make("synth", N, 4)
    a.timed_notes([(8, i, ON, 60) for i in range(N)] + [(72, i, ON, 64) for i in range(N)])
    a.reset()
    b.reset()
    for e in (a, b):
        e.note_events([(i, ON, 50) for i in range(N)])
    ya = np.concatenate([block(a, 64, cuda), block(a, 64, cuda)], 1)
    yb = np.concatenate([block(b, 64, cuda), block(b, 64, cuda)], 1)
    assert yb.any() and np.array_equal(ya.view(np.uint32), yb.view(np.uint32))
    assert a.playing(0) == b.playing(0) == [50, 0, 0, 0]


def test_return_codes_and_refused_calls(cuda):
    """The voice kinds: OLFX_E_KIND; effects and meters: OLFX_E_STATE; a bad record anywhere in a call: OLFX_E_ARG,
    nothing queued, Playing() untouched -- the next block is the twin's that never made the call."""
    arr = (_lib.TimedNote * 2)()
    arr[0].frame, arr[0].ev.inst, arr[0].ev.type, arr[0].ev.note = 8, 0, ON, 60
    for kind, code in (("voice", _lib.OLFX_E_KIND), ("voice_moog", _lib.OLFX_E_KIND), ("voice_sample", _lib.OLFX_E_KIND),
                       ("fxrack", _lib.OLFX_E_STATE), ("meter", _lib.OLFX_E_STATE)):
        e = ofx.Engine(kind, 8)
        assert e.lib.olfx_timed_notes(e.handle, arr, 1) == code
    for kind in C.KINDS:
        a, b = make(kind, 70, 4), make(kind, 70, 4)
        bad = [(6, 0, ON, 60), (1 << 31, 0, ON, 60), (8, 70, ON, 60), (8, 0, ON, 128), (8, 0, 4, 60)]
        bad += [(8, 0, C.GATE_ON, 60)] if kind == "drumkit" else []
        for frame, inst, ty, note in bad:
            arr[0].frame, arr[0].ev.inst, arr[0].ev.type, arr[0].ev.note = 0, 1, ON, 61
            arr[1].frame, arr[1].ev.inst, arr[1].ev.type, arr[1].ev.note = frame, inst, ty, note
            assert a.lib.olfx_timed_notes(a.handle, arr, 2) == _lib.OLFX_E_ARG
            assert a.playing(1) == [0, 0, 0, 0]
        assert a.lib.olfx_timed_notes(a.handle, ctypes.cast(None, ctypes.POINTER(_lib.TimedNote)), 1) == _lib.OLFX_E_ARG
        setup = C.setup(kind, 70, 4) + [("events", C.notes_on(kind, 70, 4)), ("block", 64), ("block", 64)]
        ya, _, _ = run_engine(kind, setup, 70, 4, cuda, e=a)
        yb, _, _ = run_engine(kind, setup, 70, 4, cuda, e=b)
        assert yb.any() and np.array_equal(ya.view(np.uint32), yb.view(np.uint32))


# ------------------------------------------------------------------- against the CPU references, composed
CASES = C.cases(65)


@pytest.mark.parametrize("name", sorted(CASES))
def test_against_the_cpu_references(cuda, rcp_table, name):
    """Every case at n = 65 against synth_ref / synth_svf_ref / drumkit_ref run on the resolved script, bit for bit,
    with Playing() against the references' tables."""
    kind, script, n, voices = CASES[name]
    yr, ref = C.run_reference(kind, script, n, voices, threads=8)
    C.condition(kind, yr, ref)
    y, tables, _ = run_engine(kind, script, n, voices, cuda)
    assert bits_equal(y, yr), first_mismatch(y, yr)
    assert len(tables) == len(ref.trace)
    for k, (t, want) in enumerate(zip(tables, ref.trace)):
        assert np.array_equal(t, want), (k, np.argwhere(t != want)[:4])


# ------------------------------------------------------------------------------------------- containment
@pytest.mark.parametrize("io", ["device", "host"])
@pytest.mark.parametrize("kind", C.KINDS)
def test_segmented_stores_contained(cuda, kind, io):
    """n = 65.  `out` is a view into a larger buffer with 64 sentinel floats on each side, at offset 0 and at offset
    1 (off 16-byte alignment): the 128-frame call of 17 times (two launches, the second writing from row 64 of both
    planes) and a 64-frame call of six.  The guards keep their bits, every float of `out` is written, and the output
    is the split-call twin's."""
    import torch
    n, voices = 65, 4
    for offset in (0, 1):
        for script in (C.case_seventeen(kind, n, voices), C.case_sparse(kind, n, voices)):
            yb, _, _ = run_engine(kind, script, n, voices, cuda, timed=False)
            assert np.isfinite(yb).all()                         # so that the sentinel NaN is unmistakable
            a, at = make(kind, n, voices), 0
            for step in script:
                if step[0] == "block":
                    b = step[1]
                    if io == "device":
                        buf, view = _guarded_torch(2 * b * n, offset, cuda)
                        a.process(None, out=view.view(2, b, n))
                        torch.cuda.synchronize()
                        ya = view.view(2, b, n).cpu().numpy()
                    else:
                        buf, view = _guarded_numpy(2 * b * n, offset)
                        out = view.reshape(2, b, n)
                        assert a.process(None, out=out) is out and np.shares_memory(out, buf)
                        ya = out.copy()
                    _assert_contained(buf, offset, 2 * b * n)
                    want = yb[:, at:at + b]
                    assert np.array_equal(ya.view(np.uint32), want.view(np.uint32)), (offset, at, first_mismatch(ya, want))
                    at += b
                elif step[0] != "check_playing":
                    run_engine(kind, [step], n, voices, cuda, e=a)
