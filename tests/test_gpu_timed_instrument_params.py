"""olfx_timed_instrument_params / olfx_timed_instrument_control on the GPU: parameter and control changes at a frame
inside the block for OLFX_KIND_SYNTH, OLFX_KIND_SYNTH_SVF and OLFX_KIND_DRUMKIT (synth_block_v1_seg,
synth_svf_block_v1_seg, drumkit_block_v1_seg: the V role's loop-carried voice coefficients, the F role's rack
coefficients switched at a quad inside a chunk, a launch ended at a delay-field or topology change).

The contract is the oracle: a timed script on one engine equals, bit for bit, a twin engine driven by the split
calls tests/timed_instrument_param_cases.py resolve() makes of it -- one process call per distinct time, with that
time's records applied by set_param / control in queueing order and its notes handed to note_events before it -- in
the output, in the event-free 64-frame call every case ends with (the stored state), in Engine.playing, in get_param
and in frames_processed.  The cases are that module's; n = 130 unless stated: three groups, two live lanes in the
last, whose second delay wave exits.  The same cases at n = 65 are compared with the composed CPU references as well,
and tests/test_timed_instrument_params_ref.py shows on the CPU that every timed change in them is audible."""
import ctypes

import numpy as np
import pytest

import ol_dsp_amd as ofx
import timed_instrument_param_cases as T
import timed_note_cases as C
from helpers import first_mismatch
from ol_dsp_amd import _lib
from synth_ref import bits_equal
from test_gpu_drumkit import apply as kit_apply
from test_gpu_edges import _assert_contained, _guarded_numpy, _guarded_torch

pytestmark = pytest.mark.gpu

N = 130


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


def step_on(e, kind, step, voices):
    """One step of a timed or resolved script that is no block."""
    op = step[0]
    if op == "timed":
        e.timed_notes(step[1])
    elif op == "tparams":
        e.timed_instrument_params(step[1])
    elif op == "tcontrol":
        e.timed_instrument_control(step[1])
    elif op == "set":
        e.set_param(step[1], step[2], step[3])
    elif op == "control":
        e.control(step[1])
    elif kind == "drumkit":
        kit_apply(e, step, voices)
    elif op == "params":
        e.set_params(0, step[1])
    elif op == "events":
        e.note_events(step[1])
    else:
        raise ValueError(op)


def params_of(e, insts):
    return np.array([[e.get_param(i, f) for f in range(len(ofx.engine.PARAMS[e.kind]))] for i in insts], np.float32)


def run_engine(kind, script, n, voices, cuda, timed=True, io="device", e=None):
    """The timed script on an engine (timed = False: the split calls it resolves into): ([2][frames][n], [Playing()
    [n][voices] and few(n)'s parameters at each check_playing step and at the end], the engine)."""
    e = make(kind, n, voices) if e is None else e
    out, tables = [], []
    look = lambda: tables.append((np.array([e.playing(i) for i in range(n)]), params_of(e, C.few(n))))
    for step in (script if timed else T.resolve(script)):
        if step[0] == "block":
            out.append(block(e, step[1], cuda, io))
        elif step[0] == "check_playing":
            look()
        else:
            step_on(e, kind, step, voices)
    look()
    return (np.concatenate(out, 1) if out else None), tables, e


def against_twin(kind, script, n, voices, cuda, io="device"):
    ya, pa, a = run_engine(kind, script, n, voices, cuda, True, io)
    yb, pb, b = run_engine(kind, script, n, voices, cuda, False, io)
    assert np.isfinite(yb).all() and yb[0].any(axis=0).all()     # every instrument sounded
    assert np.array_equal(ya.view(np.uint32), yb.view(np.uint32)), first_mismatch(ya, yb)
    assert len(pa) == len(pb) >= 1
    for k, ((ta, qa), (tb, qb)) in enumerate(zip(pa, pb)):
        assert np.array_equal(ta, tb), (k, np.argwhere(ta != tb)[:4])
        assert np.array_equal(qa.view(np.uint32), qb.view(np.uint32)), (k, np.argwhere(qa != qb)[:4])
    every = range(n) if n <= 130 else C.few(n)
    qa, qb = params_of(a, every), params_of(b, every)
    assert np.array_equal(qa.view(np.uint32), qb.view(np.uint32)), np.argwhere(qa != qb)[:4]
    assert a.frames_processed == b.frames_processed
    return ya, a


# ------------------------------------------------------------------------------ against the split-call twin
@pytest.mark.parametrize("voices", [1, 4, 5, 8])
@pytest.mark.parametrize("kind", T.KINDS)
def test_record_frames_by_voices(cuda, kind, voices):
    """Records at frames 4, 12, 16, 20, 36 and 60 -- a voice field, a rack field, a control -- at P = 1, 4, 5 (V wave 0
    runs two voices) and 8."""
    against_twin(kind, T.case_frames(kind, N, voices), N, voices, cuda)


@pytest.mark.parametrize("n", [1, 33, 64, 65])
@pytest.mark.parametrize("kind", T.KINDS)
def test_record_frames_by_instruments(cuda, kind, n):
    """One lane (a launch takes one record there: the call runs as several), the second delay wave just on, one full
    group, a group of one."""
    against_twin(kind, T.case_frames(kind, n, 4), n, 4, cuda)


@pytest.mark.parametrize("case", ["voice_fields", "rack_fields", "controls", "update_only", "with_notes"])
@pytest.mark.parametrize("kind", T.KINDS)
def test_fields_controls_and_notes(cuda, kind, case):
    """Voice fields alone (cutoff, resonance, the envelope times, portamento, the Svf voice's drive); F-role fields alone
    (FILTER_TYPE through all five values, MASTER_VOLUME at topology 0, REVERB_BALANCE); controls (CC 41-44 on both
    filters, CC 45-48 and 7 at topology 0, a kit's channel and rack, update-only on never-configured voices, ignored
    ones); records with notes at their frame, a NoteOn retriggering envelopes whose times change at that frame."""
    build = getattr(T, "case_" + case)
    against_twin(kind, build(kind, N, 4), N, 4, cuda)


@pytest.mark.parametrize("kind", T.KINDS)
def test_boundary_fields_end_the_launch(cuda, kind):
    """DELAY_TIME at 20 (small, and large on every third instrument) and at 36 (0), the topology flipped at 12 on every
    other instrument: four launches, the later ones starting off the 16-frame grid, with voice records and notes at
    those frames and between them."""
    script = T.case_boundary(kind, N, 4)
    ya, a = against_twin(kind, script, N, 4, cuda)
    if kind != "synth":
        topo = np.array([a.get_param(i, T.rf(kind, "topology")) for i in range(N)])
        assert np.array_equal(topo[0::2], np.ones(N // 2)) and np.array_equal(topo[1::2], np.ones(N // 2))
        assert not ya[1, :12, 0::2].any() and ya[1, 12:64, 0::2].any(axis=0).all()      # channel 1 wakes at frame 12


@pytest.mark.parametrize("kind", T.KINDS)
def test_call_sizes(cuda, kind):
    """Calls of 4, 12, 100 and 300 frames: a start in a partial last chunk, on a call's last quad, records carried over."""
    against_twin(kind, T.case_sizes(kind, N, 4), N, 4, cuda)


# ------------------------------------------------------------------------------------------- engine limits
@pytest.mark.parametrize("io", ["device", "host"])
@pytest.mark.parametrize("kind", T.KINDS)
def test_seventeen_times_in_one_call(cuda, kind, io):
    """Note times and record times together make 17: two launches in one 128-frame call, with device and host I/O."""
    ya, _ = against_twin(kind, T.case_seventeen(kind, N, 4), N, 4, cuda, io)
    assert ya[0, 64:128].any() and ya[1, 64:128, 1::2].any()


@pytest.mark.parametrize("kind", T.KINDS)
def test_record_cap_exceeded_in_one_call(cuda, kind):
    against_twin(kind, T.case_record_cap(kind, N, 4), N, 4, cuda)


@pytest.mark.parametrize("kind", T.KINDS)
def test_carry_over_three_calls_with_untimed_changes(cuda, kind):
    """Records at frame == 64, 64 + 36 and 2 x 64 + 4 / + 60 queued up front; an untimed set_param and a control between
    the calls land behind the record that reached frame 0 and ahead of the pending ones."""
    against_twin(kind, T.case_carry(kind, N, 4), N, 4, cuda)


@pytest.mark.parametrize("kind", T.KINDS)
def test_stream_switch_with_records_pending(cuda, kind):
    """The carry-over case with its calls on the engine's own stream, a second torch stream and the null stream in turn,
    no ordering and no wait from the caller."""
    import torch
    script = T.case_carry(kind, N, 4)
    a = make(kind, N, 4)
    side = torch.cuda.Stream(cuda)
    streams = [a.lib.olfx_stream(a.handle) or 0, side.cuda_stream, 0]
    assert len(set(streams)) == 3
    outs = [torch.full((2, s[1], N), 7.0, device=cuda) for s in script if s[0] == "block"]
    torch.cuda.synchronize()
    c = 0
    for step in script:
        if step[0] == "block":
            a.process(None, out=outs[c], stream=streams[c % 3])
            c += 1
        else:
            step_on(a, kind, step, 4)
    torch.cuda.synchronize()
    ya = np.concatenate([o.cpu().numpy() for o in outs], 1)
    yb, _, _ = run_engine(kind, script, N, 4, cuda, timed=False)
    assert np.array_equal(ya.view(np.uint32), yb.view(np.uint32)), first_mismatch(ya, yb)


@pytest.mark.parametrize("kind", T.KINDS)
def test_copied_packets(cuda, kind, monkeypatch):
    """OLFX_COPY_BYTES=0: every packet is copied to the device, so both tables and the records are read from device
    memory; the boundary case is four launches, four packets."""
    script = T.case_boundary(kind, N, 4)
    yb, _, _ = run_engine(kind, script, N, 4, cuda, timed=False)
    monkeypatch.setenv("OLFX_COPY_BYTES", "0")
    a = make(kind, N, 4)
    monkeypatch.delenv("OLFX_COPY_BYTES")
    ya, _, _ = run_engine(kind, script, N, 4, cuda, e=a)
    assert np.array_equal(ya.view(np.uint32), yb.view(np.uint32)), first_mismatch(ya, yb)


@pytest.mark.parametrize("kind", T.KINDS)
def test_reset_drops_pending_records(cuda, kind):
    a, b = make(kind, N, 4), make(kind, N, 4)
    a.timed_instrument_params([(8, i, T.vf(kind, "filter_cutoff"), 300.0) for i in range(N)] +
                              [(72, i, T.rf(kind, "filter_cutoff"), 500.0) for i in range(N)])
    a.timed_instrument_control([T.ctl(12, i, T.CC_RESONANCE, 100.0, kind) for i in range(N)])
    a.reset()
    b.reset()
    script = C.setup(kind, N, 4) + [("events", C.notes_on(kind, N, 4)), ("block", 64), ("block", 64)]
    ya, _, _ = run_engine(kind, script, N, 4, cuda, e=a)
    yb, _, _ = run_engine(kind, script, N, 4, cuda, e=b)
    assert yb.any() and np.array_equal(ya.view(np.uint32), yb.view(np.uint32))


@pytest.mark.parametrize("kind", T.KINDS)
def test_at_scale(cuda, kind):
    """n = 8230: 129 groups, a last group of 38."""
    against_twin(kind, T.case_frames(kind, 8230, 4), 8230, 4, cuda)


def test_return_codes_and_refused_calls(cuda):
    """The voice kinds: OLFX_E_KIND; effects and meters: OLFX_E_STATE; a bad record anywhere in a call: OLFX_E_ARG,
    nothing queued, the parameters untouched -- the next blocks are the twin's that never made the call."""
    par = (_lib.TimedParam * 2)()
    con = (_lib.TimedControl * 2)()
    par[0].frame, par[0].inst, par[0].field, par[0].value = 8, 0, 0, 100.0
    con[0].frame, con[0].ev.inst, con[0].ev.control, con[0].ev.value = 8, 0, 41, 64.0
    for kind, code in (("voice", _lib.OLFX_E_KIND), ("voice_moog", _lib.OLFX_E_KIND), ("voice_sample", _lib.OLFX_E_KIND),
                       ("fxrack", _lib.OLFX_E_STATE), ("meter", _lib.OLFX_E_STATE)):
        e = ofx.Engine(kind, 8)
        assert e.lib.olfx_timed_instrument_params(e.handle, par, 1) == code
        assert e.lib.olfx_timed_instrument_control(e.handle, con, 1) == code
    for kind in T.KINDS:
        e = make(kind, 8, 4)
        assert e.lib.olfx_timed_params(e.handle, par, 1) == _lib.OLFX_E_KIND
        a, b = make(kind, 70, 4), make(kind, 70, 4)
        f, topo = T.vf(kind, "filter_cutoff"), T.rf(kind, "topology")
        before = params_of(a, range(70))
        bad = [(6, 0, f, 1.0), (1 << 31, 0, f, 1.0), (8, 70, f, 1.0), (8, 0, len(ofx.engine.PARAMS[a.kind]), 1.0),
               (8, 0, f, float("nan")), (8, 0, topo, 2.0), (8, 0, topo, 0.0 if kind == "synth" else 0.5)]
        for frame, inst, field, value in bad:
            par[0].frame, par[0].inst, par[0].field, par[0].value = 0, 1, f, 321.0
            par[1].frame, par[1].inst, par[1].field, par[1].value = frame, inst, field, value
            assert a.lib.olfx_timed_instrument_params(a.handle, par, 2) == _lib.OLFX_E_ARG
        for frame, inst, source, value in [(6, 0, 0, 64.0), (1 << 31, 0, 0, 64.0), (8, 70, 0, 64.0), (8, 0, 2, 64.0),
                                           (8, 0, 0, float("nan"))]:
            con[0].frame, con[0].ev.inst, con[0].ev.control, con[0].ev.value, con[0].ev.source = 0, 1, 41, 64.0, 0
            con[1].frame, con[1].ev.inst, con[1].ev.control, con[1].ev.value, con[1].ev.source = frame, inst, 41, value, source
            con[0].ev.pad = con[1].ev.pad = T.CH_RACK if kind == "drumkit" else 0
            assert a.lib.olfx_timed_instrument_control(a.handle, con, 2) == _lib.OLFX_E_ARG
        null = ctypes.cast(None, ctypes.POINTER(_lib.TimedParam))
        assert a.lib.olfx_timed_instrument_params(a.handle, null, 1) == _lib.OLFX_E_ARG
        assert np.array_equal(params_of(a, range(70)).view(np.uint32), before.view(np.uint32))
        script = C.setup(kind, 70, 4) + [("events", C.notes_on(kind, 70, 4)), ("block", 64), ("block", 64)]
        ya, _, _ = run_engine(kind, script, 70, 4, cuda, e=a)
        yb, _, _ = run_engine(kind, script, 70, 4, cuda, e=b)
        assert yb.any() and np.array_equal(ya.view(np.uint32), yb.view(np.uint32))


# ------------------------------------------------------------------- against the CPU references, composed
CASES = T.cases(65)


@pytest.mark.parametrize("name", sorted(CASES))
def test_against_the_cpu_references(cuda, rcp_table, name):
    """Every case at n = 65 against synth_ref / synth_svf_ref / drumkit_ref run on the resolved script, bit for bit,
    with Playing() against the references' tables."""
    kind, script, n, voices = CASES[name]
    yr, ref = T.run_reference(kind, script, n, voices, threads=8)
    C.condition(kind, yr, ref)
    y, tables, _ = run_engine(kind, script, n, voices, cuda)
    assert bits_equal(y, yr), first_mismatch(y, yr)
    assert len(tables) == len(ref.trace) + 1
    for k, ((t, _), want) in enumerate(zip(tables, ref.trace)):
        assert np.array_equal(t, want), (k, np.argwhere(t != want)[:4])


# ------------------------------------------------------------------------------------------- containment
@pytest.mark.parametrize("io", ["device", "host"])
@pytest.mark.parametrize("kind", T.KINDS)
def test_segmented_stores_contained(cuda, kind, io):
    """n = 65.  `out` is a view into a larger buffer with 64 sentinel floats on each side, at offset 0 and at offset 1
    (off 16-byte alignment): the boundary case (four launches in a call, three of them starting off the chunk grid)
    and the 128-frame call of 17 times.  The guards keep their bits, every float of `out` is written, and the output
    is the split-call twin's."""
    import torch
    n, voices = 65, 4
    for offset in (0, 1):
        for script in (T.case_boundary(kind, n, voices), T.case_seventeen(kind, n, voices)):
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
                    step_on(a, kind, step, voices)
