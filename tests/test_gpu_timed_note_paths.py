"""olfx_timed_notes on the GPU beyond tests/test_gpu_timed_notes.py's 64-frame calls: the cases of
tests/timed_note_paths.py on synth_block_v1_seg, synth_svf_block_v1_seg and drumkit_block_v1_seg -- a seeded score
over calls of 4 to 300 frames (partial last chunks with a segment start in them, launches that start off the chunk
grid, many pieces per V wave, notes carried over two calls) and the same notes in other cuts, exactly 4 and 5 records
in a voice-slot group, the kit's retriggers inside a chunk against the sampler suite's bank, the edge suites' corner
parameters with the envelopes restarted in mid-chunk, 17 launches in one call, a set and a control with notes
pending, n = 8230 and 32838, a refused olfx_process with notes pending, 44.1 and 96 kHz.

Every comparison is bit for bit, the output and Engine.playing: against the twin engine driven by the split calls
(test_gpu_timed_notes.against_twin, which also makes every case end in an event-free call: the stored state), and
against the composed CPU references, each held to its condition first (tests/test_timed_notes_ref.py does that
alone on the CPU)."""
import ctypes

import numpy as np
import pytest

import ol_dsp_amd as ofx
import timed_note_cases as C
import timed_note_paths as T
from helpers import first_mismatch
from ol_dsp_amd import _lib
from synth_ref import bits_equal
from test_gpu_edges import _assert_contained, _guarded_numpy, _guarded_torch
from test_gpu_timed_notes import against_twin, make, run_engine

pytestmark = pytest.mark.gpu

N = 130


def same(y, yr, what=""):
    assert y.shape == yr.shape and np.array_equal(y.view(np.uint32), yr.view(np.uint32)), (what, first_mismatch(y, yr))


def against_reference(kind, script, n, voices, cuda, y=None, tables=None, io="device", sample_rate=48000.0):
    """The reference meets timed_note_cases.condition; then the engine's output (y, or a run of the script with this
    I/O at this sample rate) and every Playing() table equal the reference's."""
    yr, ref = T.run_reference(kind, script, n, voices, threads=8, sample_rate=sample_rate)
    C.condition(kind, yr, ref)
    if y is None:
        e = ofx.Engine(kind, n, voices=voices, sample_rate=sample_rate)
        y, tables, _ = run_engine(kind, script, n, voices, cuda, io=io, e=e)
    assert bits_equal(y, yr), first_mismatch(y, yr)
    assert len(tables) == len(ref.trace)
    for k, (t, want) in enumerate(zip(tables, ref.trace)):
        assert np.array_equal(t, want), (k, np.argwhere(t != want)[:4])
    return yr, ref


# ------------------------------------------------------------------------------------------------ the score
@pytest.mark.parametrize("n,voices", T.SCORE_SHAPES)
@pytest.mark.parametrize("kind", C.KINDS)
def test_score_against_reference_and_twin(cuda, rcp_table, kind, n, voices):
    """Calls of 64, 4, 12, 100, 300, 256, 20, 8 and 64 frames at (130, 4), (65, 5) and (65, 8): segment starts inside
    partial last chunks and on a call's last quad, a launch of 16 segments followed by one that starts at frame 68,
    dense and sparse times beyond chunk 4, notes carried over one and two calls, Playing() after every call."""
    s = T.score(kind, n, voices)
    y, tables = against_twin(kind, s, n, voices, cuda)
    against_reference(kind, s, n, voices, cuda, y, tables)


@pytest.mark.parametrize("kind", C.KINDS)
def test_score_with_host_io(cuda, rcp_table, kind):
    """The score at (65, 4) through host buffers: a later launch of a call writes from an unaligned row on."""
    s = T.score(kind, 65, 4)
    against_reference(kind, s, 65, 4, cuda, io="host")


@pytest.mark.parametrize("kind", C.KINDS)
def test_score_recut(cuda, rcp_table, kind):
    """The score's notes queued up front at their absolute times, in one call of 828 frames (four launches or more,
    the later ones from unaligned rows) and in calls of 36, 300 and 492: the reference's bits of the original cut."""
    n, voices = 65, 4
    s = T.score(kind, n, voices)
    yr, ref = T.run_reference(kind, s, n, voices, threads=8)
    C.condition(kind, yr, ref)
    for lengths in T.RECUTS:
        again = T.recut(s, lengths)
        assert len(C.launches(again)[0]) >= (4 if len(lengths) == 1 else 1)
        y, tables, e = run_engine(kind, again, n, voices, cuda)
        assert bits_equal(y, yr), (lengths, first_mismatch(y, yr))
        assert len(tables) == 1 and np.array_equal(tables[0], ref.trace[-1])
        assert e.frames_processed == T.SCORE_TOTAL


@pytest.mark.parametrize("io", ["device", "host"])
@pytest.mark.parametrize("kind", C.KINDS)
def test_score_stores_contained(cuda, kind, io):
    """n = 65.  Every call of the score writes into a view of a larger buffer with 64 sentinel floats on each side,
    at offset 0 and at offset 1 (off 16-byte alignment): the 4-frame call, the partial last chunks and the launches
    that start at an unaligned row leave the guards alone, write every float of `out`, and give the twin's bits."""
    import torch
    n, voices = 65, 4
    s = T.score(kind, n, voices)
    yb, _, _ = run_engine(kind, s, n, voices, cuda, timed=False)
    assert np.isfinite(yb).all()                                 # so that the sentinel NaN is unmistakable
    for offset in (0, 1):
        a, at = make(kind, n, voices), 0
        for step in s:
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
                same(ya, yb[:, at:at + b], (offset, at, b))
                at += b
            elif step[0] != "check_playing":
                run_engine(kind, [step], n, voices, cuda, e=a)
        assert at == T.SCORE_TOTAL


# ------------------------------------------------------------------------------------- fixed-slot capacity
@pytest.mark.parametrize("kind", C.KINDS)
def test_exactly_four_and_five_records(cuda, rcp_table, kind):
    """n = 70, P = 4: 4 records in a voice-slot group (the fixed slots, full), 5 (the first overflow run), 4, 5 and
    6 in the ragged last group, whose spare lanes mirror instrument 69, and 63 in a full one."""
    s = T.case_capacity(kind)
    assert T.capacity_counts(kind, s) == T.CAPACITY_COUNTS
    y, tables = against_twin(kind, s, T.CAPACITY_N, T.CAPACITY_P, cuda)
    against_reference(kind, s, T.CAPACITY_N, T.CAPACITY_P, cuda, y, tables)
    assert np.array_equal(tables[1], tables[0]) and np.all(tables[0] != 0)


# ------------------------------------------------------------------------- the kit against the sampler bank
@pytest.mark.parametrize("n,voices", T.KIT_BANK_SHAPES)
def test_kit_bank_retriggered_inside_a_chunk(cuda, rcp_table, n, voices):
    """Samples of 1 to 1000 frames, the nine loop configurations and loops of 1 to 17 frames, every pad sought back
    to 0 at frames 4, 8 and 12 of a 16-frame call and at 20, 40 and 60 of a 64-frame one: pieces of 4, 8 and 12
    frames with plain and frame-by-frame lanes in one wave."""
    s = T.case_kit_bank(n, voices)
    made, got, forced, ended, looping = T.kit_bank_coverage(s, n, voices)
    assert got == made and forced == set(T.DK.FORCED) and ended and looping
    y, tables = against_twin("drumkit", s, n, voices, cuda)
    against_reference("drumkit", s, n, voices, cuda, y, tables)


# ------------------------------------------------------------------------------------------------- corners
@pytest.mark.parametrize("kind", C.KINDS)
def test_corner_parameters_with_timed_notes(cuda, rcp_table, kind):
    """(70, 8), each field at its corner with probability 1/2: the NoteOns at frames 4 and 12 of a 256-frame call,
    the NoteOffs at frame 8 and on the last quad of the 100-frame call, queued a call ahead -- the envelopes are
    restarted from live registers in mid-chunk with attack, decay and release at their corners."""
    s = T.case_corners(kind)
    yr, ref = T.run_reference(kind, s, T.CORNER_N, T.CORNER_P, threads=8)
    T.corner_condition(kind, s, yr)
    y, tables, _ = run_engine(kind, s, T.CORNER_N, T.CORNER_P, cuda)
    assert bits_equal(y, yr), first_mismatch(y, yr)
    assert len(tables) == len(ref.trace) == 2 and all(np.array_equal(t, w) for t, w in zip(tables, ref.trace))
    yb, pb, _ = run_engine(kind, s, T.CORNER_N, T.CORNER_P, cuda, timed=False)
    same(y, yb, "the twin")
    assert all(np.array_equal(t, w) for t, w in zip(tables, pb))


# -------------------------------------------------------------------------------------------- engine paths
@pytest.mark.parametrize("kind", C.KINDS)
def test_seventeen_launches_in_one_call(cuda, kind):
    """272 event times in one call of 1088 frames: 17 launches with a packet each, one more than the engine has
    zero-copy slots -- the last one's packet waits for the first one's readers."""
    s = T.case_ring(kind, N, 4)
    assert len(C.launches(s)[0]) == T.KSLOTS + 1
    against_twin(kind, s, N, 4, cuda)


@pytest.mark.parametrize("kind", C.KINDS)
def test_set_and_control_with_notes_pending(cuda, rcp_table, kind):
    """A set of a voice field and a rack field and a control between calls 2 and 3, the notes of calls 3 and 4
    pending: coefficient records and a three-segment event table in one packet.  Against the twin; at n = 65 against
    the references as well."""
    against_twin(kind, T.case_coefs(kind, N, 4), N, 4, cuda)
    s = T.case_coefs(kind, 65, 4)
    against_reference(kind, s, 65, 4, cuda)


@pytest.mark.parametrize("n,voices", T.SCALE_SHAPES)
@pytest.mark.parametrize("kind", C.KINDS)
def test_large_packets(cuda, kind, n, voices):
    """128 groups and 38 instruments at P = 8, 513 groups and 6 instruments at P = 4: a sparse time at 4, a dense one
    at 12 (its records past the 64 KiB from which a packet is copied) and a sparse one at 60.  Playing() on 64
    instruments or so, the first and the last among them."""
    s = T.case_scale(kind, n, voices)
    assert C.launches(s) == [[4], [1]]
    ya, _, a = run_engine(kind, s, n, voices, cuda)
    yb, _, b = run_engine(kind, s, n, voices, cuda, timed=False)
    assert np.isfinite(yb).all() and yb[0].any(axis=0).all()
    same(ya, yb)
    note = C.note_of(kind, n, voices)
    for i in T.sampled(n):
        assert a.playing(i) == b.playing(i), i
        assert a.playing(i)[voices - 1] == 0 and a.playing(i)[0] == note(i, 0)
    a.close()
    b.close()


@pytest.mark.parametrize("kind", C.KINDS)
def test_refused_process_keeps_pending_notes(cuda, kind):
    """olfx_process with n_frames = 6 and with out = NULL is OLFX_E_ARG and leaves the pending notes and Playing()
    alone: the next valid calls equal the twin's, which never made the refused ones."""
    import torch
    s = C.case_carry(kind, N, 4)
    at = next(k for k, st in enumerate(s) if st[0] == "block")
    a = make(kind, N, 4)
    run_engine(kind, s[:at], N, 4, cuda, e=a)                    # the set-up, the notes, the timed notes
    before = [a.playing(i) for i in range(N)]
    out = torch.full((2, 64, N), 7.0, device=cuda)
    s0 = ctypes.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)
    assert a.lib.olfx_process(a.handle, None, ctypes.c_void_p(out.data_ptr()), 6, _lib.IO_DEVICE, s0) == _lib.OLFX_E_ARG
    assert a.lib.olfx_process(a.handle, None, None, 64, _lib.IO_DEVICE, s0) == _lib.OLFX_E_ARG
    assert a.lib.olfx_process(a.handle, None, None, 64, _lib.IO_HOST, s0) == _lib.OLFX_E_ARG
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and a.frames_processed == 0
    assert [a.playing(i) for i in range(N)] == before
    ya, pa, _ = run_engine(kind, s[at:], N, 4, cuda, e=a)
    yb, pb, _ = run_engine(kind, s, N, 4, cuda, timed=False)
    assert yb[0].any(axis=0).all()
    same(ya, yb)
    assert len(pa) == len(pb) and all(np.array_equal(t, w) for t, w in zip(pa, pb))


@pytest.mark.parametrize("sr", [44100.0, 96000.0])
@pytest.mark.parametrize("kind", C.KINDS)
def test_at_other_sample_rates(cuda, rcp_table, kind, sr):
    """case_sparse at n = 33 and 44.1 and 96 kHz: the reference at that rate is not the 48 kHz one; bit for bit."""
    s = C.case_sparse(kind, 33, 4)
    yr, _ = against_reference(kind, s, 33, 4, cuda, sample_rate=sr)
    yr48, _ = T.run_reference(kind, s, 33, 4, threads=8)
    assert np.any(yr.view(np.uint32) != yr48.view(np.uint32))
