"""olfx_timed_params / olfx_timed_control on the GPU: parameter and control changes at a frame inside the block,
for the three voice kinds.

The contract is the oracle: one process(N) with timed records equals, bit for bit, a fresh twin engine that is
called once per distinct time below N -- a time being a timed event's or a timed parameter record's frame -- with
that time's parameter records applied by set_param / control in queueing order, and that time's events then queued
by voice_events, before the call.  Compared: the output, and the output of one further event-free 64-frame block,
which exposes the stored state.  `PTwin` restates the queue's rules in Python and drives the twin with split calls.

n = 130 voices unless stated: three workgroups, two live lanes in the last.

The CPU-reference cases (tests/timed_param_cases.py) run on the engine in test_cases_against_the_cpu_reference."""
import ctypes

import numpy as np
import pytest

import ol_dsp_amd as ofx
from helpers import first_mismatch_or_nan, same_bits_or_nan
from ol_dsp_amd import _lib
from test_gpu_edges import _assert_contained, _guarded_numpy, _guarded_torch
from test_gpu_timed_events import KINDS, N, NOTE_OFF, NOTE_ON, all_on, configs, make, quads, run

pytestmark = pytest.mark.gpu

CUTOFF, ENV_AMT, RES, DRIVE = "filter_cutoff", "filter_env_amount", "filter_resonance", "filter_drive"
CC_CUTOFF, CC_RES, CC_AMP_R, CC_OSC_1_VOLUME, CC_NOBODY = 41, 42, 111, 114, 3


def fname(e, name):
    """A field by the name engine.py gives it, whatever the spelling of the table: resolved through field()."""
    return e.field(name)


class PTwin:
    """The split-call side of the contract: pending events and pending parameter records, each ordered by (frame,
    arrival), and an engine that only ever sees set_param / control / voice_events at a block's start."""

    def __init__(self, e):
        self.e, self.events, self.params = e, [], []

    def queue_events(self, events):              # (frame, inst, type[, note[, value]])
        self.events += [tuple(ev) for ev in events]
        self.events.sort(key=lambda ev: ev[0])   # stable: ties keep arrival order

    def queue_params(self, records):             # (frame, inst, field, value)
        self.params += [("p",) + tuple(r) for r in records]
        self.params.sort(key=lambda r: r[1])

    def queue_control(self, records):            # (frame, inst, cc, value[, source])
        self.params += [("c",) + tuple(r) for r in records]
        self.params.sort(key=lambda r: r[1])

    def run(self, frames, cuda, io="device"):
        ev = [x for x in self.events if x[0] < frames]
        pr = [x for x in self.params if x[1] < frames]
        self.events = [(x[0] - frames,) + x[1:] for x in self.events if x[0] >= frames]
        self.params = [(x[0], x[1] - frames) + x[2:] for x in self.params if x[1] >= frames]
        cuts = sorted({0} | {x[0] for x in ev} | {x[1] for x in pr}) + [frames]
        parts = []
        for f0, f1 in zip(cuts, cuts[1:]):
            for r in pr:
                if r[1] == f0 and r[0] == "p":
                    self.e.set_param(r[2], r[3], r[4])
                elif r[1] == f0:
                    self.e.control([r[2:]])
            self.e.voice_events([x[1:] for x in ev if x[0] == f0])
            parts.append(run(self.e, f1 - f0, cuda, io))
        return np.concatenate(parts, 1)

    @property
    def pending(self):
        return self.events or self.params


def assert_same(got, want, what):
    assert same_bits_or_nan(got, want), (what, first_mismatch_or_nan(got, want))


def check(kind, cuda, params=(), events=(), control=(), frames=64, calls=1, io="device", n=N, cfg=None, a=None, sounding=True):
    """The records through timed_params / timed_control / timed_events on one engine and through the twin."""
    a = make(kind, cfg, n) if a is None else a
    t = PTwin(make(kind, cfg, n))
    a.timed_events(list(events))
    a.timed_params(list(params))
    a.timed_control(list(control))
    t.queue_events(events)
    t.queue_params(params)
    t.queue_control(control)
    lengths = [frames] * calls if isinstance(frames, int) else list(frames)
    for c, m in enumerate(lengths):
        ya, yb = run(a, m, cuda, io), t.run(m, cuda, io)
        assert np.isfinite(yb).all()
        assert_same(ya, yb, f"call {c} of {m} frames")
        assert not sounding or c or ya.any() or m < 16
    assert not t.pending
    assert_same(run(a, 64, cuda, io), run(t.e, 64, cuda, io), "the stored state (a further event-free block)")
    return a, t


def sweep(e, who, frames, field=CUTOFF, lo=300.0, hi=9000.0):
    """One record per (listed frame, listed voice): the field stepping from lo to hi over the frames."""
    f = e if isinstance(e, int) else fname(e, field)
    return [(fr, i, f, float(np.float32(lo + (hi - lo) * ((k + 1) / len(frames) + 1e-3 * (i % 97)))))
            for k, fr in enumerate(frames) for i in who]


FIELDS = [CUTOFF, "amp_release", "amp_attack", "portamento", RES, DRIVE, ENV_AMT, "amp_env_amount", "filter_attack",
          "filter_decay", "amp_sustain"]


def varied(e, frames, groups, rng):
    """Records on the voices of `groups[k]` at frames[k], the field cycling through every role's words."""
    ranges = {CUTOFF: (100.0, 12000.0), "portamento": (0.001, 0.3)}
    recs = []
    for k, (fr, who) in enumerate(zip(frames, groups)):
        name = FIELDS[k % len(FIELDS)]
        lo, hi = ranges.get(name, (0.05, 0.95))
        recs += [(fr, int(i), fname(e, name), float(np.float32(rng.uniform(lo, hi)))) for i in who]
    return recs


TIMES = [4, 12, 16, 20, 36, 60]


@pytest.mark.parametrize("kind", KINDS)
def test_sparse_groups_and_every_voice_at_one_frame(cuda, kind):
    """n = 130, times 4, 12, 16, 20, 36, 60.  Sparse: a few voices per time, group 1 untouched at 12, the last group's
    two voices at 36 (the dead lanes' mirror, voice 129, among them).  Then every voice at frame 20, with notes
    sounding from frame 0 and events of their own at 12 and 36."""
    a = make(kind)
    rng = np.random.default_rng(3)
    groups = [[0, 5, 63, 64, 129], [1, 2, 128], [7, 70], [3, 64, 65, 66, 67, 68], [128, 129], [0, 63, 64, 127, 129]]
    check(kind, cuda, params=varied(a, TIMES, groups, rng), events=all_on(0) + quads([12, 36]), a=a)
    b = make(kind)
    check(kind, cuda, params=sweep(b, range(N), [20]) + sweep(b, range(N), [20], field=RES, lo=0.1, hi=0.9),
          events=all_on(0), a=b)


@pytest.mark.parametrize("n", [1, 63, 64, 65])
@pytest.mark.parametrize("kind", KINDS)
def test_sizes(cuda, kind, n):
    a = make(kind, n=n)
    rng = np.random.default_rng(n)
    groups = [sorted(set(rng.integers(0, n, 5).tolist()) | {n - 1}) for _ in TIMES]
    check(kind, cuda, params=varied(a, TIMES, groups, rng), events=all_on(0, n) + quads([16, 40], n), n=n, a=a)


@pytest.mark.parametrize("kind", KINDS)
def test_changed_voice_counts_and_ragged_group(cuda, kind):
    """n = 70: exactly one changed voice in group 0 (its last lane) at frame 8, all 64 at frame 16, the ragged
    group's six voices at 24, its last voice alone at 28, and voice 3 again at 40 only (it keeps frame 16's
    registers through the segments at 24 and 28)."""
    n = 70
    a = make(kind, n=n)
    recs = sweep(a, [63], [8]) + sweep(a, range(64), [16], lo=500.0, hi=4000.0) + sweep(a, range(64, 70), [24])
    recs += sweep(a, [69], [28], field=RES, lo=0.2, hi=0.8) + sweep(a, [3], [40], lo=50.0, hi=200.0)
    check(kind, cuda, params=recs, events=all_on(0, n) + [(28, i, NOTE_OFF) for i in range(0, n, 2)], n=n, a=a)


@pytest.mark.parametrize("kind", KINDS)
def test_17_mixed_times_two_launches(cuda, kind):
    """128 frames, 17 times past frame 0 alternating between events and parameter records (both at 60): two
    launches, the second starting at the time that did not fit."""
    a = make(kind)
    times = list(range(4, 72, 4))
    assert len(times) == 17
    ev_t = [t for k, t in enumerate(times) if k % 2 == 0 or t == 60]
    pr_t = [t for k, t in enumerate(times) if k % 2 == 1 or t == 60]
    recs = sweep(a, range(0, N, 3), pr_t) + sweep(a, [129], pr_t[:2], field=ENV_AMT, lo=0.1, hi=0.9)
    check(kind, cuda, params=recs, events=all_on(0) + quads(ev_t), frames=128, a=a)


@pytest.mark.parametrize("kind", KINDS)
def test_ragged_calls_and_carry_over(cuda, kind):
    """Calls of 64, 4, 12, 100 and 300 frames, everything queued before the first: records land in every call, one
    at a call's frame 0 (carried there), one carried over two calls, launches that start off the chunk grid."""
    a = make(kind)
    lengths = [64, 4, 12, 100, 300]
    times = [8, 64, 68, 72, 76, 84, 132, 180, 184, 300, 476]            # 64, 68 and 180 are call starts
    recs = sweep(a, range(0, N, 2), times) + sweep(a, range(1, N, 2), times[::3], field=RES, lo=0.1, hi=0.9)
    check(kind, cuda, params=recs, events=all_on(0) + quads([20, 72, 200, 304]), frames=lengths, a=a)


@pytest.mark.parametrize("kind", KINDS)
def test_launch_cut_by_the_record_bound(cuda, kind):
    """n = 65: all 65 voices change at frame 8 and one more at 16 -- 66 records, one past the launch's n: the launch
    ends at 16 and the change there is the next launch's frame-0 scatter."""
    n = 65
    a = make(kind, n=n)
    recs = sweep(a, range(n), [8]) + sweep(a, [7], [16], lo=40.0, hi=90.0) + sweep(a, range(0, n, 2), [24], field=RES, lo=0.1, hi=0.9)
    check(kind, cuda, params=recs, events=all_on(0, n), n=n, a=a)


@pytest.mark.parametrize("kind", KINDS)
def test_host_io(cuda, kind):
    a = make(kind)
    check(kind, cuda, params=sweep(a, range(0, N, 2), TIMES), events=all_on(0) + quads([12]), io="host", a=a)


@pytest.mark.parametrize("kind", KINDS)
def test_copied_packets(cuda, monkeypatch, kind):
    """OLFX_COPY_BYTES=0 on the engine under test: every packet, the timed coefficient section included, is read from
    its device copy."""
    monkeypatch.setenv("OLFX_COPY_BYTES", "0")
    a = make(kind)
    monkeypatch.delenv("OLFX_COPY_BYTES")
    check(kind, cuda, params=sweep(a, range(N), TIMES), events=all_on(0) + quads([12, 40]), frames=[64, 64], a=a)


@pytest.mark.parametrize("kind", KINDS)
def test_at_scale(cuda, kind):
    """n = 8230, once: 129 workgroups; a third of the voices change at each of three times."""
    n = 8230
    a = make(kind, n=n)
    recs = sweep(a, range(0, n, 3), [12]) + sweep(a, range(1, n, 3), [24], field=RES, lo=0.1, hi=0.9) + sweep(a, range(2, n, 3), [44])
    check(kind, cuda, params=recs, events=all_on(0, n), n=n, a=a)


@pytest.mark.parametrize("kind", KINDS)
def test_stream_switch_with_records_pending(cuda, kind):
    import torch
    a, t = make(kind), PTwin(make(kind))
    lengths = [64, 20, 64]
    recs = sweep(a, range(0, N, 2), [8, 40, 64, 72, 84, 100, 140])
    side = torch.cuda.Stream(cuda)
    streams = [a.lib.olfx_stream(a.handle) or 0, side.cuda_stream, 0]
    outs = [torch.full((1, m, N), 7.0, device=cuda) for m in lengths]
    torch.cuda.synchronize()
    a.timed_events(all_on(0))
    a.timed_params(recs)
    for c, out in enumerate(outs):
        a.process(None, out=out, stream=streams[c % 3])
    torch.cuda.synchronize()
    t.queue_events(all_on(0))
    t.queue_params(recs)
    for c, m in enumerate(lengths):
        assert_same(outs[c].cpu().numpy(), t.run(m, cuda), f"call {c} of {m} frames")
    assert not t.pending
    assert_same(run(a, 64, cuda), run(t.e, 64, cuda), "the stored state")


@pytest.mark.parametrize("kind", KINDS)
def test_control_equals_its_mapped_field(cuda, kind):
    """timed_control against timed_params of the field and value olfx_control_map gives, the update-only control
    against the twin's control(), and a control the reference ignores against nothing."""
    a, b = make(kind), make(kind)
    ctl, par = [], []
    for k, (fr, cc) in enumerate([(8, CC_CUTOFF), (20, CC_RES), (36, CC_AMP_R)]):
        for i in range(k, N, 3):
            val = float(10 + (7 * i) % 110)
            name, mapped = ofx.control_map(kind, cc, val)
            ctl.append((fr, i, cc, val))
            par.append((fr, i, b.field(name), mapped))
    ctl += [(12, i, CC_NOBODY, 64.0) for i in range(N)]
    assert ofx.control_map(kind, CC_NOBODY, 64.0) is None and ofx.control_map(kind, CC_OSC_1_VOLUME, 64.0)[0] == "update_only"
    for e in (a, b):
        e.timed_events(all_on(0))
    a.timed_control(ctl)
    b.timed_params(par)
    ya, yb = run(a, 64, cuda), run(b, 64, cuda)
    assert_same(ya, yb, "control against its mapped field")
    assert ya.any()
    assert_same(run(a, 64, cuda), run(b, 64, cuda), "the stored state")
    # update-only: voices that were never configured become configured at frame 24
    c = ofx.Engine(kind, N)
    if kind == "voice_sample":
        c = make(kind)
        c.reset()
    tc = PTwin(ofx.Engine(kind, N) if kind != "voice_sample" else make(kind))
    if kind == "voice_sample":
        tc.e.reset()
    for e in (c, tc.e):
        for i in range(N):
            for name in ("amp_release", "filter_resonance"):
                assert e.lib.olfx_set_member(e.handle, i, e.field(name), 0.9) == 0
    upd = [(24, i, CC_OSC_1_VOLUME, 64.0) for i in range(0, N, 2)]
    c.timed_events(all_on(0))
    c.timed_control(upd)
    tc.queue_events(all_on(0))
    tc.queue_control(upd)
    assert_same(run(c, 64, cuda), tc.run(64, cuda), "update-only at frame 24")
    assert_same(run(c, 64, cuda), run(tc.e, 64, cuda), "the stored state")


@pytest.mark.parametrize("kind", KINDS)
def test_untimed_write_after_a_timed_launch(cuda, kind):
    """A launch changes voices at frames 8 and 24; at the next boundary set_param rewrites some of them, then come two
    calls with nothing queued: the device arrays get each voice's last record -- the timed one where nothing was
    written since, the untimed one where it was -- once, and keep it."""
    a, t = make(kind), PTwin(make(kind))
    recs = sweep(a, range(0, N, 2), [8, 24]) + sweep(a, range(0, N, 4), [24], field=RES, lo=0.1, hi=0.9)
    for q in (a.timed_events, t.queue_events):
        q(all_on(0))
    a.timed_params(recs)
    t.queue_params(recs)
    assert_same(run(a, 64, cuda), t.run(64, cuda), "the timed call")
    for e in (a, t.e):
        for i in range(0, N, 8):
            e.set_param(i, CUTOFF, 150.0 + i)
    for c in range(3):
        assert_same(run(a, 64, cuda), t.run(64, cuda), f"event-free call {c}")


@pytest.mark.parametrize("kind", KINDS)
def test_refused_process_keeps_the_records(cuda, kind):
    import torch
    a = make(kind)
    recs = sweep(a, range(0, N, 2), [8, 20, 64, 72])
    a.timed_events(all_on(0))
    a.timed_params(recs)
    out = torch.full((1, 64, N), 7.0, device=cuda)
    s0 = ctypes.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)
    assert a.lib.olfx_process(a.handle, None, ctypes.c_void_p(out.data_ptr()), 6, _lib.IO_DEVICE, s0) == _lib.OLFX_E_ARG
    assert a.lib.olfx_process(a.handle, None, None, 64, _lib.IO_DEVICE, s0) == _lib.OLFX_E_ARG
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and a.frames_processed == 0
    t = PTwin(make(kind))
    t.queue_events(all_on(0))
    t.queue_params(recs)
    for c in range(2):
        assert_same(run(a, 64, cuda), t.run(64, cuda), f"call {c}")
    assert not t.pending


@pytest.mark.parametrize("kind", KINDS)
def test_shadow_reads_and_refusals(cuda, kind):
    """get_param over time; OLFX_E_ARG leaves the queue and the shadow alone; OLFX_E_KIND for another kind."""
    a, b = make(kind), make(kind)
    f = a.field(CUTOFF)
    before = a.get_param(5, CUTOFF)
    a.timed_params([(0, 4, f, 1234.0), (8, 5, f, 2345.0), (64, 5, f, 3456.0), (100, 5, f, 4567.0)])
    assert a.get_param(4, CUTOFF) == 1234.0 and a.get_param(5, CUTOFF) == before
    for bad in ((6, 0, f, 1.0), (1 << 31, 0, f, 1.0), (8, N, f, 1.0), (8, 0, 16, 1.0), (8, 0, f, float("nan"))):
        arr = (_lib.TimedParam * 2)()
        arr[0].frame, arr[0].inst, arr[0].field, arr[0].value = 0, 9, f, 77.0
        arr[1].frame, arr[1].inst, arr[1].field, arr[1].value = bad
        assert a.lib.olfx_timed_params(a.handle, arr, 2) == _lib.OLFX_E_ARG
    assert a.lib.olfx_timed_params(a.handle, ctypes.cast(None, ctypes.POINTER(_lib.TimedParam)), 1) == _lib.OLFX_E_ARG
    carr = (_lib.TimedControl * 1)()
    carr[0].frame, carr[0].ev.inst, carr[0].ev.control, carr[0].ev.value = 8, N, CC_CUTOFF, 64.0
    assert a.lib.olfx_timed_control(a.handle, carr, 1) == _lib.OLFX_E_ARG
    assert a.get_param(9, CUTOFF) == b.get_param(9, CUTOFF)
    for e in (a, b):
        e.note_events([(i, NOTE_ON, 50) for i in range(N)])
    t = PTwin(b)
    t.queue_params([(0, 4, f, 1234.0), (8, 5, f, 2345.0), (64, 5, f, 3456.0), (100, 5, f, 4567.0)])
    assert_same(run(a, 64, cuda), t.run(64, cuda), "call 0")
    assert a.get_param(5, CUTOFF) == 3456.0          # frame 64 reached frame 0 as the call returned
    assert_same(run(a, 64, cuda), t.run(64, cuda), "call 1")
    assert a.get_param(5, CUTOFF) == 4567.0
    a.timed_params([(8, 5, f, 9999.0)])
    a.reset()
    b.reset()
    assert_same(run(a, 64, cuda), run(b, 64, cuda), "reset drops the pending records")
    for other in ("synth", "drumkit", "fxrack", "chorus", "meter"):
        e = ofx.Engine(other, 3)
        arr = (_lib.TimedParam * 1)()
        arr[0].frame, arr[0].value = 8, 0.5
        assert e.lib.olfx_timed_params(e.handle, arr, 1) == _lib.OLFX_E_KIND
        carr = (_lib.TimedControl * 1)()
        carr[0].frame, carr[0].ev.control, carr[0].ev.value = 8, CC_CUTOFF, 64.0
        assert e.lib.olfx_timed_control(e.handle, carr, 1) == _lib.OLFX_E_KIND


def test_sampler_bank_cutoff_change_while_a_loop_turns(cuda):
    """The sample voice: 61-frame loops on the odd voices turn inside every 64-frame fetch window; their cutoff and
    resonance change at frames 100 and 200 of a 256-frame call, and the one-shots' at 12 (as they run out)."""
    a = make("voice_sample")
    recs = sweep(a, range(1, N, 2), [100, 200]) + sweep(a, range(1, N, 2), [200], field=RES, lo=0.1, hi=0.9)
    recs += sweep(a, range(0, N, 2), [12])
    check("voice_sample", cuda, params=recs, events=all_on(0), frames=256, a=a)


@pytest.mark.parametrize("io", ["device", "host"])
@pytest.mark.parametrize("n", [1, 70])
@pytest.mark.parametrize("kind", KINDS)
def test_stores_contained(cuda, kind, n, io):
    """`out` is a view into a larger buffer with sentinel guards on each side, at offsets 0 and 1: the guards keep
    their bits and the output is the twin's."""
    import torch
    cfg = configs(kind, n)
    cfg[2] *= 0.25                       # moderate Svf drive: finite, so the sentinel NaN is unmistakable
    for offset in (0, 1):
        a, t = make(kind, cfg, n), PTwin(make(kind, cfg, n))
        for c, b in enumerate([4, 20, 68]):
            recs = sweep(a, range(n), list(range(4, b, 12)))
            evs = all_on(0, n) if c == 0 else []
            a.timed_events(evs)
            a.timed_params(recs)
            t.queue_events(evs)
            t.queue_params(recs)
            if io == "device":
                buf, view = _guarded_torch(b * n, offset, cuda)
                a.process(None, out=view.view(1, b, n))
                torch.cuda.synchronize()
                ya = view.view(1, b, n).cpu().numpy()
            else:
                buf, view = _guarded_numpy(b * n, offset)
                out = view.reshape(1, b, n)
                assert a.process(None, out=out) is out
                ya = out.copy()
            _assert_contained(buf, offset, b * n)
            yb = t.run(b, cuda, io)
            assert np.isfinite(yb).all()
            assert_same(ya, yb, f"offset {offset}, call of {b} frames")


# ------------------------------------------------- the cases of timed_param_cases.py against the CPU reference
import timed_cases as C          # noqa: E402
import timed_param_cases as P    # noqa: E402
from helpers import first_mismatch                        # noqa: E402
from test_gpu_parity import voice_bits_equal              # noqa: E402
from test_gpu_timed_paths import engine_for               # noqa: E402


def drive_case(e, calls, cuda):
    """A case's calls on the engine: a timed column is one timed_params record per field."""
    parts = []
    for untimed, timed, boundary, tparams, n_frames in calls:
        assert not boundary
        e.voice_events(untimed)
        e.timed_events(timed)
        e.timed_params([(frame, op[1], f, float(op[2][f])) for frame, op in tparams for f in range(16)])
        parts.append(run(e, n_frames, cuda))
    return np.concatenate(parts, 1)


@pytest.mark.parametrize("kind", KINDS)
def test_cases_against_the_cpu_reference(cuda, rcp_table, kind):
    """Every case of tests/timed_param_cases.py, bit for bit against the kernel-arithmetic oracle called in split
    blocks; each reference meets its condition first (the timed change matters)."""
    for name, case in P.cases(kind).items():
        s, calls = case[0], case[1]
        yr = P.split_oracle(C.reference(s), calls)
        P.condition(name, case, yr, P.split_oracle(C.reference(s), P.without_params(calls)))
        y = drive_case(engine_for(s), calls, cuda)
        assert voice_bits_equal(y, yr), (name, first_mismatch(y, yr))
