"""OLFX_KIND_METER / OLFX_KIND_METER_MONO (meter_block_v1) on the GPU, bit for bit against tests/meter_ref.py --
the numpy restatement that tests/test_meter_ref.py holds to recordings of the reference's own ol::core::Rms.
The envelope of every frame and all five state rows after every call are compared under
helpers.same_bits_or_nan.  Small ragged shapes: instance counts that are no multiple of four (one signal per
lane) and multiples of four (four per lane) with partial last waves, buffers one float off the 16-byte
boundary, calls whose last chunk has 4 or 12 frames, a one-chunk call."""
import numpy as np
import pytest
import torch

import meter_cases as C
import meter_ref as M
import ol_dsp_amd as ofx
from helpers import same_bits_or_nan
from ol_dsp_amd import _lib

pytestmark = pytest.mark.gpu

KINDS = {"meter": 2, "meter_mono": 1}
GUARD = 64
SENTINEL = np.array([0xDEADBEEF], np.uint32).view(np.float32)[0]       # a finite float no meter produces here


def engine(kind, n, sample_rate=48000.0, window=None, hold=None):
    e = ofx.Engine(kind, n, sample_rate=sample_rate)
    assert e.kernel_name == "meter_block_v1" and e.info.in_channels == KINDS[kind] == e.info.out_channels
    if window is not None:
        e.set_params("window", np.broadcast_to(np.asarray(window, np.float32), (n,)))
    if hold is not None:
        e.set_params("peak_hold", np.broadcast_to(np.asarray(hold, np.float32), (n,)))
    return e


def guarded(cuda, shape, offset):
    """A [shape] view `offset` floats past a 16-byte boundary with GUARD sentinel floats on either side."""
    size = int(np.prod(shape))
    buf = torch.full((GUARD + offset + size + GUARD,), float(SENTINEL), dtype=torch.float32, device=cuda)
    assert buf.data_ptr() % 16 == 0
    view = buf[GUARD + offset:GUARD + offset + size].view(*shape)
    assert view.is_contiguous() and view.data_ptr() % 16 == (4 * offset) % 16
    return buf, view


def guards_intact(buf, offset, size):
    b = buf.cpu().numpy().view(np.uint32)
    s = SENTINEL.view(np.uint32)
    return bool(np.all(b[:GUARD + offset] == s) and np.all(b[GUARD + offset + size:] == s))


def run(e, x, cuda, calls=C.CALLS, modes=(True,), changes=None, offset=0, stream_of=None):
    """The call schedule on the device: each call's input and output in guarded buffers of their own.  Returns the
    envelope (zeros where a summary call wrote nothing) and the levels after every call."""
    ch, _, n = x.shape
    env = np.zeros(x.shape, np.float32)
    levels, f0 = [], 0
    for k, m in enumerate(calls):
        for field, values, first in (changes or {}).get(k, ()):
            e.set_params(field, np.atleast_1d(np.asarray(values, np.float32)), first=first)
        ibuf, xin = guarded(cuda, (ch, m, n), offset)
        xin.copy_(torch.from_numpy(np.array(x[:, f0:f0 + m])))
        stream = stream_of(k) if stream_of else None
        if stream is not None:
            torch.cuda.current_stream(cuda).synchronize()       # the input copy, ahead of a launch on another stream
        if modes[k % len(modes)]:
            obuf, out = guarded(cuda, (ch, m, n), offset)
            e.process(xin, out=out, stream=stream)
            levels.append(e.levels())
            env[:, f0:f0 + m] = out.cpu().numpy()
            assert guards_intact(obuf, offset, ch * m * n), ("out guards", k)
        else:
            e.meter(xin, stream=stream)
            levels.append(e.levels())
        assert guards_intact(ibuf, offset, ch * m * n), ("in guards", k)
        assert same_bits_or_nan(xin.cpu().numpy(), x[:, f0:f0 + m]), ("input changed", k)
        f0 += m
    return env, levels


def assert_same(env, levels, renv, rlevels, what=""):
    assert same_bits_or_nan(env, renv), (what, "envelope", np.argwhere(env.view(np.uint32) != renv.view(np.uint32))[:4])
    assert len(levels) == len(rlevels)
    for k, (a, b) in enumerate(zip(levels, rlevels)):
        for f in M.FIELDS:
            assert same_bits_or_nan(a[f], b[f]), (what, "call", k, f)


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("n,offset", [(1, 0), (63, 0), (70, 0), (72, 0), (260, 0), (300, 0), (72, 1)])
def test_shapes_windows_and_holds(cuda, kind, n, offset):
    """Every window and hold of the mix within one wave, over the ragged call schedule."""
    ch = KINDS[kind]
    C.check_hold_expiries()
    x = C.noise(n, ch)
    w, h = C.mixed_windows(n), C.mixed_holds(n)
    renv, rlevels = C.reference(n, ch, x, window=w, hold=h)
    with engine(kind, n, window=w, hold=h) as e:
        env, levels = run(e, x, cuda, offset=offset)
        assert e.frames_processed == C.FRAMES
        assert e.algorithmic_bytes_per_frame == 8 * ch and e.algorithmic_read_bytes_per_frame == 4 * ch
    assert_same(env, levels, renv, rlevels, (kind, n, offset))
    assert np.any(env != 0) and not np.any(env.view(np.uint32) == SENTINEL.view(np.uint32))     # every float written


@pytest.mark.parametrize("n", [70, 72])
def test_modes_leave_the_same_state(cuda, n):
    x = C.noise(n)
    w, h = C.mixed_windows(n), C.mixed_holds(n)
    renv, rlevels = C.reference(n, 2, x, window=w, hold=h)
    got = {}
    for name, modes in (("envelope", (True,)), ("summary", (False,)), ("alternating", (True, False)),
                        ("alternating2", (False, True))):
        with engine("meter", n, window=w, hold=h) as e:
            got[name] = run(e, x, cuda, modes=modes)            # (summary calls: guards around `in` only)
        _, rl = C.reference(n, 2, x, modes=modes, window=w, hold=h)
        for k, (a, b) in enumerate(zip(got[name][1], rl)):
            for f in M.FIELDS:
                assert same_bits_or_nan(a[f], b[f]), (name, k, f)
    for name in ("summary", "alternating", "alternating2"):
        for f in M.FIELDS:
            assert same_bits_or_nan(got[name][1][-1][f], got["envelope"][1][-1][f]), (name, f)
            assert same_bits_or_nan(got[name][1][-1][f], rlevels[-1][f]), (name, f)
    assert same_bits_or_nan(got["envelope"][0], renv)
    assert not np.any(got["summary"][0])
    for k in range(len(C.CALLS)):                               # the alternations' envelope calls
        s = slice(C.STARTS[k], C.STARTS[k + 1])
        assert same_bits_or_nan(got["alternating" if k % 2 == 0 else "alternating2"][0][:, s], renv[:, s])


@pytest.mark.parametrize("n", [70, 72])
def test_window_changes_between_calls(cuda, n):
    w, changes, up, down = C.window_changes(n)
    x = C.noise(n)
    renv, rlevels = C.reference(n, 2, x, window=w, changes=changes)
    C.check_window_changes(rlevels, up, down)                   # on the reference first: no later reset
    with engine("meter", n, window=w) as e:
        env, levels = run(e, x, cuda, changes=changes)
        assert e.get_param(int(down[0]), "window") == 100 and e.get_param(int(up[0]), "window") == 128
    assert_same(env, levels, renv, rlevels)


@pytest.mark.parametrize("sample_rate,count", [(44100.0, C.FRAMES), (96000.0, 256)])
def test_default_window_at_other_rates(cuda, sample_rate, count):
    n = 70
    x = C.noise(n)
    renv, rlevels = C.reference(n, 2, x, sample_rate=sample_rate)
    assert np.all(rlevels[-1]["count"] == count)
    with engine("meter", n, sample_rate=sample_rate) as e:
        env, levels = run(e, x, cuda)
    assert_same(env, levels, renv, rlevels, sample_rate)


def test_long_run_past_the_default_hold(cuda):
    """100,352 frames at 44.1 kHz in calls of 4,096, alternating the modes: the default hold (96,000) expires inside
    call 23, and the sum that never resets (window 117.6) runs past 70,000 frames."""
    n, frames, call = 70, 100352, 4096
    calls = [call] * (frames // call) + [frames % call]
    assert len(calls) == 25 and sum(calls) == frames
    x = C.noise(n, 1, frames, first=1000)
    renv, rlevels = C.reference(n, 1, x, calls=calls, modes=(True, False), sample_rate=44100.0)
    assert np.all(rlevels[22]["peak_count"] == 23 * call) and np.all(rlevels[23]["peak_count"] == 24 * call - 96000)
    assert np.all(rlevels[-1]["count"] == frames) and np.all(rlevels[-1]["peak_count"] == frames - 96000)
    xd = torch.from_numpy(np.array(x)).to(cuda)
    env = np.zeros_like(x)
    levels = []
    with engine("meter_mono", n, sample_rate=44100.0) as e:
        for k in range(len(calls)):
            xin = xd[:, k * call:k * call + calls[k]].contiguous()
            if k % 2 == 0:
                env[:, k * call:k * call + calls[k]] = e.process(xin).cpu().numpy()
            else:
                e.meter(xin)
            if k in (22, 23, len(calls) - 1):
                levels.append(e.levels())
    assert_same(env, levels, renv, [rlevels[22], rlevels[23], rlevels[-1]])


@pytest.mark.parametrize("n", [70, 72])
@pytest.mark.parametrize("name", C.EDGES)
def test_edges(cuda, name, n):
    x, hold = C.edge(name, n)                                   # its condition asserted on the reference
    renv, rlevels = C.reference(n, 2, x, window=np.float32(128), hold=hold)
    with engine("meter", n, window=np.float32(128), hold=hold) as e:
        env, levels = run(e, x, cuda)
    assert_same(env, levels, renv, rlevels, (name, n))
    if name in ("one_nan", "inf"):
        # everything but the poisoned signals: bit-identical to a GPU run on the clean input
        with engine("meter", n, window=np.float32(128), hold=hold) as e:
            clean, clevels = run(e, C.noise(n), cuda)
        p = C.POISONED(n)
        others = np.setdiff1d(np.arange(n), p)
        assert np.array_equal(env[0][:, others].view(np.uint32), clean[0][:, others].view(np.uint32))
        assert np.array_equal(env[1].view(np.uint32), clean[1].view(np.uint32))
        for a, b in zip(levels, clevels):
            for f in M.FIELDS:
                assert np.array_equal(a[f][others].view(np.uint32), b[f][others].view(np.uint32))
                assert np.array_equal(a[f][:, 1].view(np.uint32), b[f][:, 1].view(np.uint32))


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", [1, 63, 70, 72])
def test_containment_device(cuda, n, offset):
    """64 sentinel floats around `in` and `out` keep their bits and every output float is written (run checks the
    guards after every call), aligned and one float off."""
    for kind, ch in KINDS.items():
        x = C.noise(n, ch, 280)
        renv, rlevels = C.reference(n, ch, x, calls=[256, 4, 20])
        with engine(kind, n) as e:
            env, levels = run(e, x, cuda, calls=[256, 4, 20], offset=offset)
        assert_same(env, levels, renv, rlevels, (kind, n, offset))
        assert not np.any(env.view(np.uint32) == SENTINEL.view(np.uint32))


def test_containment_host():
    n, calls = 70, [256, 4, 20]
    for kind, ch in KINDS.items():
        x = C.noise(n, ch, 280)
        renv, rlevels = C.reference(n, ch, x, calls=calls, modes=(True, False))
        with engine(kind, n) as e:
            f0 = 0
            for k, m in enumerate(calls):
                size = ch * m * n
                ibuf = np.full(2 * GUARD + 1 + size, SENTINEL, np.float32)
                obuf = ibuf.copy()
                xin = ibuf[GUARD + 1:GUARD + 1 + size].reshape(ch, m, n)
                out = obuf[GUARD + 1:GUARD + 1 + size].reshape(ch, m, n)
                xin[:] = x[:, f0:f0 + m]
                if k % 2 == 0:
                    assert e.process(xin, out=out) is out
                    assert same_bits_or_nan(out, renv[:, f0:f0 + m])
                else:
                    e.meter(xin)
                    assert np.all(out.view(np.uint32) == SENTINEL.view(np.uint32))
                lv = e.levels()
                for f in M.FIELDS:
                    assert same_bits_or_nan(lv[f], rlevels[k][f]), (kind, k, f)
                for buf in (ibuf, obuf):
                    b = buf.view(np.uint32)
                    assert np.all(b[:GUARD + 1] == SENTINEL.view(np.uint32)) and np.all(b[GUARD + 1 + size:] == SENTINEL.view(np.uint32))
                f0 += m


def test_reset_gives_fresh_state_and_keeps_the_parameters(cuda):
    n = 72
    x = C.noise(n)
    w, h = C.mixed_windows(n), C.mixed_holds(n)
    renv, rlevels = C.reference(n, 2, x, window=w, hold=h)
    with engine("meter", n, window=w, hold=h) as e:
        run(e, x[:, :280], cuda, calls=[256, 4, 20])
        e.reset()
        lv = e.levels()
        assert all(not np.any(lv[f]) for f in M.FIELDS) and e.frames_processed == 0
        assert e.get_param(3, "window") == w[3] and e.get_param(3, "peak_hold") == h[3]
        env, levels = run(e, x, cuda)
        assert_same(env, levels, renv, rlevels)


def test_stream_switch_and_asynchronous_levels(cuda):
    """Calls alternate between two streams with no event from the caller; levels() right after an asynchronous
    device call returns that call's state."""
    n = 300
    x = C.noise(n)
    w, h = C.mixed_windows(n), C.mixed_holds(n)
    renv, rlevels = C.reference(n, 2, x, window=w, hold=h)
    s1, s2 = torch.cuda.Stream(cuda), torch.cuda.Stream(cuda)
    torch.cuda.synchronize()
    with engine("meter", n, window=w, hold=h) as e:
        env, levels = run(e, x, cuda, stream_of=lambda k: (s1, s2)[k % 2].cuda_stream)
        e.sync()
    assert_same(env, levels, renv, rlevels)


def test_fed_from_another_engines_device_output(cuda):
    """fxrack -> meter on the device: the levels of the rack's output, never copied to the host in between."""
    n, frames = 70, 512
    x = torch.from_numpy(np.array(C.noise(n)[:, :frames])).to(cuda)
    with ofx.Engine("fxrack", n) as rack, engine("meter", n) as e:
        y = rack.process(x)
        env = e.process(y)
        lv = e.levels()
        yh = y.cpu().numpy()
    renv, rlevels = C.reference(n, 2, yh, calls=[frames])
    assert np.any(yh != 0)
    assert_same(env.cpu().numpy(), [lv], renv, rlevels)


def test_refusals(cuda):
    lib = ofx.load()
    with engine("meter_mono", 8) as e, ofx.Engine("fxrack", 8) as rack:
        with pytest.raises(ofx.OlfxError) as err:
            e.set_param(0, "window", float("nan"))
        assert err.value.code == _lib.OLFX_E_ARG
        with pytest.raises(ofx.OlfxError) as err:
            e.control([(0, 7, 64)])
        assert err.value.code == _lib.OLFX_E_KIND
        with pytest.raises(ofx.OlfxError) as err:
            rack.levels()
        assert err.value.code == _lib.OLFX_E_STATE
        # summary mode is the meters' alone
        xr = torch.zeros((2, 4, 8), device=cuda)
        assert lib.olfx_process(rack.handle, xr.data_ptr(), None, 4, 0, None) == _lib.OLFX_E_ARG
        assert lib.olfx_process(e.handle, None, None, 4, 0, None) == _lib.OLFX_E_ARG
        assert e.levels(2, 3)["rms"].shape == (3, 1)


QUAD_CHILD = """
import sys
sys.path[:0] = [{root!r}, {root!r} + "/oracle", {root!r} + "/tests"]
import torch
import meter_cases as C
import test_gpu_meter as T
cuda = torch.device("cuda:0")
for kind, ch in T.KINDS.items():
    for n, offset in ((72, 0), (260, 0), (300, 0), (72, 1), (70, 0)):
        x = C.noise(n, ch)
        w, h = C.mixed_windows(n), C.mixed_holds(n)
        for modes in ((True,), (False, True)):
            renv, rlevels = C.reference(n, ch, x, modes=modes, window=w, hold=h)
            with T.engine(kind, n, window=w, hold=h) as e:
                env, levels = T.run(e, x, cuda, modes=modes, offset=offset)
            T.assert_same(env, levels, renv, rlevels, (kind, n, offset, modes))
print("quad ok")
"""


def test_quad_layout_in_a_process_of_its_own(cuda):
    """OLFX_MT_QUAD is read once per process: a child with it set runs the four-instances-per-lane layout wherever
    n % 4 == 0 and the buffers are aligned (72, 260, 300; not 70, not one float off), the same checks as above."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, OLFX_MT_QUAD="1")
    r = subprocess.run([sys.executable, "-c", QUAD_CHILD.format(root=root)], env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and "quad ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
