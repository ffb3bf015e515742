"""GPU parity: the HIP kernels (through the C-ABI) against the CPU oracle and the golden fixtures.

Bars: dattorro, chorus, pitch-shift and the chain are BIT-EXACT (integer-exact fp32 sequence,
-ffp-contract=off on both sides); the voice is within rel 1e-5 of max(|ref|, rms(ref)) because
Svf::SetFreq calls sinf every sample (device ocml vs host glibc may differ by an ulp).
"""
import numpy as np
import pytest

import oracle as O
from helpers import (bits_equal, chorus_params, dt_params, fast_noise, first_mismatch, fxrack_params,
                     noise_block, rel_err, voice_configs)

pytestmark = pytest.mark.gpu

VOICE_TOL = 1e-5


def engine(kind, n, **kw):
    import ol_dsp_amd as ofx
    return ofx.Engine(kind, n, **kw)


def run_gpu(eng, x: np.ndarray, blocks, cuda):
    """Feed x [ch][frames][n] block by block through device buffers; return host array."""
    import torch
    outs = []
    f0 = 0
    for b in blocks:
        xb = torch.from_numpy(np.ascontiguousarray(x[:, f0:f0 + b])).to(cuda)
        outs.append(eng.process(xb).cpu().numpy())
        f0 += b
    torch.cuda.synchronize()
    return np.concatenate(outs, axis=1)


# ------------------------------------------------------------------------------------ dattorro
def test_dattorro_impulse_golden(cuda, golden):
    e = engine("dattorro", 1)
    x = np.zeros((2, 48000, 1), np.float32)
    x[:, 0, 0] = 1.0                               # (1+1)/2 = 1: the mono C-API impulse
    y = run_gpu(e, x, [256] * 187 + [128], cuda)
    import os
    first = np.load(os.path.join(os.path.dirname(__file__), "golden", "dattorro_impulse_4096.npy"))
    assert bits_equal(y[:, :4096, 0], first), first_mismatch(y[:, :4096, 0], first)
    g = golden["dattorro_impulse"]
    assert f"{O.fnv1a64_lr(y[0, :, 0], y[1, :, 0]):016x}" == g["fnv1a64"]


def test_dattorro_noise_10s_kat(cuda, golden):
    g = golden["dattorro_noise_10s"]
    x1 = O.xorshift_noise(g["seed"], g["frames"])
    x = np.stack([x1, x1])[:, :, None]
    e = engine("dattorro", 1)
    y = run_gpu(e, x, [4096] * 117 + [768], cuda)
    assert f"{O.fnv1a64_lr(y[0, :, 0], y[1, :, 0]):016x}" == g["fnv1a64"]


def test_dattorro_reference_sweeps(cuda, golden):
    """Hashes produced by the REAL reference (oracle/_ref) for random params, 4 pre-delays."""
    for g in golden["dattorro_sweep"]:
        p = np.asarray(g["params"], np.float32)
        e = engine("dattorro", g["n"])
        e.set_params(0, p)
        x = noise_block(g["n"], g["frames"], g["input_base"])
        frames = g["frames"]
        blocks = [256] * (frames // 256) + ([frames % 256] if frames % 256 else [])
        y = run_gpu(e, x, blocks, cuda)
        got = [f"{O.fnv1a64_lr(y[0, :, i], y[1, :, i]):016x}" for i in range(g["n"])]
        assert got == g["fnv1a64"], g["pre_delay"]


@pytest.mark.parametrize("n", [1, 63, 300])
def test_dattorro_ragged_vs_oracle(cuda, n):
    rng = np.random.default_rng(n)
    p = dt_params(rng, n, 0.1)
    x = fast_noise(n, 1536, seed=n)
    e = engine("dattorro", n)
    e.set_params(0, p)
    y = run_gpu(e, x, [256, 512, 4, 764], cuda)
    ref = O.Dattorro(n)
    for i in range(n):
        for f in range(7):
            ref.set(i, f, float(p[f, i]))
    yr = ref.process(x, threads=8)
    assert bits_equal(y, yr), first_mismatch(y, yr)


def test_dattorro_per_instance_predelay(cuda):
    """DattorroVerb_setPreDelay per instance (verb.cpp:137-139): every lane has its own pre-delay
    tap, including the in-chunk delays 0..3, the chunk edges 4..8, the block edges 255..257 and
    the maximum 4800; a wave that shares one pre-delay and a wave that mixes them."""
    edge = np.array([0, 1, 2, 3, 4, 5, 7, 8, 255, 256, 257, 4799, 4800], np.float32) / 4800
    n = 200
    rng = np.random.default_rng(77)
    p = dt_params(rng, n, 0.0)
    p[0, :64] = 0.3                                               # one uniform wave
    p[0, 64:64 + len(edge)] = edge
    p[0, 64 + len(edge):] = rng.uniform(0, 1, n - 64 - len(edge))
    x = fast_noise(n, 6400, seed=77)
    e = engine("dattorro", n)
    e.set_params(0, p)
    y = run_gpu(e, x, [256] * 20 + [4, 1276], cuda)
    ref = O.Dattorro(n)
    for i in range(n):
        for f in range(7):
            ref.set(i, f, float(p[f, i]))
    yr = ref.process(x, threads=8)
    assert bits_equal(y, yr), first_mismatch(y, yr)


def test_dattorro_predelay_gather_mode_switches(cuda):
    """Per-instance pre-delays switched on and off mid-run (verb.cpp:137-139): uniform -> per
    instance (edges 0..8, 255..257, 4800, past the max) -> uniform -> per instance, calls of 256, 4,
    1028 and 60 frames, bit-exact against the oracle throughout; reset() starts over.  At this size
    both kinds run dattorro_block_v5 with the pre-delay ring in rows, as does every reverb test of
    this file and of test_gpu_edges.py below 2 x 64 x CUs instances.  dattorro_block_v4 and the layout
    conversions between the two: test_gpu_dattorro_v4.py at small ragged n (v4 forced in a child
    process), test_gpu_fullsize.py at the sizes where uniform pre-delays run v4 by themselves."""
    n = 96
    rng = np.random.default_rng(81)
    p = dt_params(rng, n, 0.2)
    e = engine("dattorro", n)
    e.set_params(0, p)
    ref = O.Dattorro(n)
    for i in range(n):
        for f in range(7):
            ref.set(i, f, float(p[f, i]))
    edge = np.array([0, 1, 2, 3, 4, 7, 8, 255, 256, 257, 4800, 8191, 8193], np.float64) / 4800
    ys, yrs = [], []
    for step in range(6):
        if step in (1, 4):                                  # per instance: gather mode
            pd = rng.uniform(0, 1, n).astype(np.float32)
            pd[:len(edge)] = edge.astype(np.float32)
        elif step == 2:                                     # one value for all: the position-major tap
            pd = np.full(n, 0.05, np.float32)
        else:
            pd = None
        if pd is not None:
            e.set_params("pre_delay", pd[None, :])
            for i in range(n):
                ref.set(i, 0, float(pd[i]))
        x = fast_noise(n, 1348, seed=81 + step)
        ys.append(run_gpu(e, x, [256, 4, 1028, 60], cuda))
        yrs.append(ref.process(x, threads=8))
    y, yr = np.concatenate(ys, 1), np.concatenate(yrs, 1)
    assert bits_equal(y, yr), first_mismatch(y, yr)
    e.reset()
    ref2 = O.Dattorro(n)
    e.set_params(0, p)
    for i in range(n):
        for f in range(7):
            ref2.set(i, f, float(p[f, i]))
    x = fast_noise(n, 512, seed=99)
    y2, yr2 = run_gpu(e, x, [512], cuda), ref2.process(x)
    assert bits_equal(y2, yr2), first_mismatch(y2, yr2)


@pytest.mark.parametrize("n", [70, 72, 136])
def test_dattorro_gather_mode_long_run_wraps(cuda, n):
    """Per-instance pre-delays over 70,000 frames: the uint16 wrap of t at 65536 and calls that start
    off the 16-position rows and the 4,096-frame launches off the 2,048-frame pieces (60, 3900, 504
    frames); pre-delays on row and window edges 0, 1, 31..37, 63..68, 96, 4800 and 8150..8191 (reads
    of ring slots the launch has not overwritten yet).  Partial 64-instance groups (70, 72, 136)
    whose dead lanes mirror the last instance.  dattorro_block_v5, bit-exact against the oracle."""
    kernel = "dattorro_block_v5"
    rng = np.random.default_rng(85)
    p = dt_params(rng, n, 0.0)
    edge = np.array([0, 1, 31, 32, 33, 35, 36, 37, 63, 64, 65, 67, 68, 96, 4800, 8150, 8160, 8190, 8191],
                    np.float64) / 4800
    p[0, :] = rng.uniform(0, 1, n).astype(np.float32)
    p[0, :len(edge)] = edge.astype(np.float32)
    x = fast_noise(n, 70000, seed=85)
    e = engine("dattorro", n)
    e.set_params(0, p)
    y = run_gpu(e, x, [60] + [4096] * 16 + [3900, 504], cuda)
    assert e.kernel_name == kernel
    ref = O.Dattorro(n)
    for i in range(n):
        for f in range(7):
            ref.set(i, f, float(p[f, i]))
    yr = ref.process(x, threads=8)
    assert bits_equal(y, yr), first_mismatch(y, yr)


def test_dattorro_predelay_beyond_max(cuda):
    """Pre-delays past MAX_PREDELAY: the reference accepts any value whose product with 4800 fits
    uint16 (verb.cpp:137-139); DelayBuffer_setDelay's offset mask + 1 - delay (verb.cpp:59-61) on
    the 8192-sample ring makes the effective delay that product mod 8192 (8192 acts as 0, 8193 as
    1).  Values outside [0, 65536/4800) are rejected, not clamped."""
    ks = np.array([4801, 6000, 8190, 8191, 8192, 8193, 8196, 8200, 12000, 16384, 16389, 65535], np.float64)
    n = 64
    rng = np.random.default_rng(78)
    p = dt_params(rng, n, 0.0)
    p[0, :] = (rng.integers(4801, 65536, n) / 4800).astype(np.float32)
    p[0, :len(ks)] = (ks / 4800).astype(np.float32)
    x = fast_noise(n, 12800, seed=78)
    e = engine("dattorro", n)
    e.set_params(0, p)
    y = run_gpu(e, x, [256] * 40 + [2560], cuda)
    ref = O.Dattorro(n)
    for i in range(n):
        for f in range(7):
            ref.set(i, f, float(p[f, i]))
    yr = ref.process(x, threads=8)
    assert bits_equal(y, yr), first_mismatch(y, yr)
    for bad in (-0.01, 65536 / 4800, 20.0):
        q = p.copy()
        q[0, 3] = bad
        with pytest.raises(Exception):
            e.set_params(0, q)


def test_dattorro_long_run_wraps(cuda):
    """70,000 frames: the modulation turn at t = 32768 and the uint16 wrap of t at 65536."""
    n = 64
    rng = np.random.default_rng(3)
    p = dt_params(rng, n, 0.25)
    x = fast_noise(n, 70000, seed=9)
    e = engine("dattorro", n)
    e.set_params(0, p)
    y = run_gpu(e, x, [4096] * 17 + [368], cuda)
    ref = O.Dattorro(n)
    for i in range(n):
        for f in range(7):
            ref.set(i, f, float(p[f, i]))
    yr = ref.process(x, threads=8)
    assert bits_equal(y, yr), first_mismatch(y, yr)


def test_dattorro_param_change_between_blocks(cuda):
    n = 40
    x = fast_noise(n, 1024, seed=4)
    rng = np.random.default_rng(4)
    p1, p2 = dt_params(rng, n, 0.0), dt_params(rng, n, 0.0)
    e = engine("dattorro", n)
    ref = O.Dattorro(n)
    e.set_params(0, p1)
    for i in range(n):
        for f in range(7):
            ref.set(i, f, float(p1[f, i]))
    ya = run_gpu(e, x[:, :512], [512], cuda)
    yra = ref.process(x[:, :512])
    e.set_params(1, p2[1:])           # fields 1..6, keep pre-delay
    for i in range(n):
        for f in range(1, 7):
            ref.set(i, f, float(p2[f, i]))
    yb = run_gpu(e, x[:, 512:], [512], cuda)
    yrb = ref.process(x[:, 512:])
    assert bits_equal(np.concatenate([ya, yb], 1), np.concatenate([yra, yrb], 1))


def test_dattorro_host_io_equals_device_io(cuda):
    n = 100
    x = fast_noise(n, 512, seed=5)
    e1, e2 = engine("dattorro", n), engine("dattorro", n)
    yd = run_gpu(e1, x, [512], cuda)
    yh = e2.process(x)                      # numpy in/out: pinned staging inside libolfx
    assert bits_equal(yd, yh)


@pytest.mark.parametrize("kind", ["chain", "chorus", "fxrack"])
def test_host_io_streams_and_interleaved_engines(cuda, kind):
    """The same job three ways: device buffers on torch's stream; host (numpy) buffers staged by
    libolfx; and device buffers on a side stream, with a second engine of the same kind processing
    different inputs in between on another stream.  All bit-identical."""
    import torch
    n = 50
    rng = np.random.default_rng(12)
    if kind == "chain":
        p = np.concatenate([chorus_params(rng, n), chorus_params(rng, n)[[0, 7]], dt_params(rng, n, 0.02)], 0)
    elif kind == "chorus":
        p = chorus_params(rng, n)
    else:
        p = fxrack_params(rng, n)
    x = fast_noise(n, 1024, seed=12)
    other = fast_noise(n, 1024, seed=13)
    ea, eb, ec, ed = (engine(kind, n) for _ in range(4))
    for e in (ea, eb, ec, ed):
        e.set_params(0, p)
    ya = run_gpu(ea, x, [256] * 4, cuda)
    yb = np.concatenate([eb.process(np.ascontiguousarray(x[:, f:f + 256])) for f in range(0, 1024, 256)], 1)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    # every input made before the loop and kept alive: a freed tensor's memory would be reused
    # by the caching allocator while the other stream still reads it
    xcs = [torch.from_numpy(np.ascontiguousarray(x[:, f:f + 256])).to(cuda) for f in range(0, 1024, 256)]
    xds = [torch.from_numpy(np.ascontiguousarray(other[:, f:f + 256])).to(cuda) for f in range(0, 1024, 256)]
    torch.cuda.synchronize()
    outs = []
    for xc, xd in zip(xcs, xds):
        with torch.cuda.stream(s1):
            outs.append(ec.process(xc, stream=s1.cuda_stream))
        with torch.cuda.stream(s2):
            ed.process(xd, stream=s2.cuda_stream)
    torch.cuda.synchronize()
    yc = np.concatenate([o.cpu().numpy() for o in outs], 1)
    assert bits_equal(ya, yb), first_mismatch(ya, yb)
    assert bits_equal(ya, yc), first_mismatch(ya, yc)


@pytest.mark.parametrize("kind", ["chain", "chorus", "pitchshift", "fxrack", "dattorro"])
def test_cooperative_and_per_lane_io_agree(cuda, kind):
    """The kernels move audio as cooperative 16-B rows when n, the plane distance and both buffers
    allow it (16-B aligned), and per lane otherwise.  n = 64 with 16-B aligned tensors takes the
    rows; the same tensors offset by one float (4-B aligned) take the per-lane path: bit-identical,
    with ragged and short blocks."""
    import torch
    n = 64
    rng = np.random.default_rng(21)
    if kind == "chain":
        p = np.concatenate([chorus_params(rng, n), chorus_params(rng, n)[[0, 7]], dt_params(rng, n, 0.02)], 0)
    elif kind == "chorus":
        p = chorus_params(rng, n)
    elif kind == "fxrack":
        p = fxrack_params(rng, n)
    elif kind == "dattorro":
        p = dt_params(rng, n, 0.02)
    else:
        p = None                                   # pitch-shift defaults
    blocks = [256, 20, 4, 236, 512]
    x = fast_noise(n, sum(blocks), seed=21)
    ea, eb = engine(kind, n), engine(kind, n)
    if p is not None:
        ea.set_params(0, p)
        eb.set_params(0, p)
    ya = run_gpu(ea, x, blocks, cuda)
    och = ea.info.out_channels
    outs, f0 = [], 0
    for b in blocks:
        xs = torch.empty(x.shape[0] * b * n + 1, dtype=torch.float32, device=cuda)
        xo = xs[1:].view(x.shape[0], b, n)
        xo.copy_(torch.from_numpy(np.ascontiguousarray(x[:, f0:f0 + b])))
        ys = torch.empty(och * b * n + 1, dtype=torch.float32, device=cuda)
        yo = ys[1:].view(och, b, n)
        assert xo.data_ptr() % 16 and yo.data_ptr() % 16
        eb.process(xo, out=yo)
        outs.append(yo.cpu().numpy())
        f0 += b
    torch.cuda.synchronize()
    yb = np.concatenate(outs, 1)
    assert bits_equal(ya, yb), first_mismatch(ya, yb)


def test_dattorro_reset(cuda):
    n = 8
    x = fast_noise(n, 512, seed=6)
    e = engine("dattorro", n)
    a = run_gpu(e, x, [512], cuda)
    e.reset()
    b = run_gpu(e, x, [512], cuda)
    assert bits_equal(a, b) and e.frames_processed == 512


@pytest.mark.parametrize("kind", ["chain", "chorus", "pitchshift", "fxrack", "voice", "voice_moog"])
def test_reset_every_kind(cuda, kind):
    """olfx_reset is destroy + create without reallocating (include/olfx.h): every instance back
    to its freshly created state (rings, recursive state, phasors, envelopes, stream time, default
    parameters).  Run, reset, set the same parameters, run again: the same bits as the first run
    and as a fresh engine."""
    n = 40
    rng = np.random.default_rng(3)
    if kind in ("voice", "voice_moog"):
        cfg = voice_configs(rng, n)

        def run(e):
            e.set_params(0, cfg)
            e.note_events([(i, 1, 40 + i) for i in range(n)])
            return np.concatenate([_voice_run(e, 256, cuda), _voice_run(e, 100, cuda)], 1)
    else:
        if kind == "chain":
            p = np.concatenate([chorus_params(rng, n), chorus_params(rng, n)[[0, 7]], dt_params(rng, n, 0.05)], 0)
        elif kind == "chorus":
            p = chorus_params(rng, n)
        elif kind == "pitchshift":
            p = chorus_params(rng, n)[[0, 7]]
        else:
            p = fxrack_params(rng, n)
        x = fast_noise(n, 1000, seed=3)

        def run(e):
            e.set_params(0, p)
            return run_gpu(e, x, [256, 744], cuda)
    e = engine(kind, n)
    a = run(e)
    e.reset()
    assert e.frames_processed == 0
    b = run(e)
    c = run(engine(kind, n))
    assert np.any(a != 0)
    assert bits_equal(a, b), first_mismatch(a, b)
    assert bits_equal(a, c), first_mismatch(a, c)


def test_dattorro_full_size_properties(cuda):
    """65,536 instances (BASELINE config 3): sampled instances match the oracle exactly, and
    instances sharing params and input produce identical output (checksum of checksums)."""
    import torch
    n, frames = 65536, 512
    rng = np.random.default_rng(11)
    p = dt_params(rng, n, 0.1)
    p[:, 1::2] = p[:, 0:1]                        # odd instances clone instance 0's params
    g = torch.Generator(device=cuda).manual_seed(0)
    x = torch.rand((2, frames, n), generator=g, device=cuda) - 0.5
    x[:, :, 1::2] = x[:, :, 0:1]                  # ... and its input
    e = engine("dattorro", n)
    e.set_params(0, p)
    y = torch.cat([e.process(x[:, :256].contiguous()), e.process(x[:, 256:].contiguous())], 1)
    torch.cuda.synchronize()
    assert torch.isfinite(y).all()
    assert torch.equal(y[:, :, 1::2], y[:, :, 0:1].expand(-1, -1, n // 2))
    idx = np.array([0, 2, 4097, 30000, 65534], np.int64)
    xs = x[:, :, idx].cpu().numpy()
    ref = O.Dattorro(len(idx))
    for k, i in enumerate(idx):
        for f in range(7):
            ref.set(k, f, float(p[f, i]))
    yr = ref.process(np.ascontiguousarray(xs))
    assert bits_equal(y[:, :, idx].cpu().numpy(), yr)


# ------------------------------------------------------------------------------- chorus / pitch
@pytest.mark.parametrize("kind,mode", [("chorus", 0), ("pitchshift", 1)])
def test_chorus_golden(cuda, golden, kind, mode):
    g = golden[kind]
    p = np.asarray(g["params"], np.float32)
    e = engine(kind, g["n"])
    if kind == "chorus":
        e.set_params(0, p)
    else:
        e.set_params(0, p[[0, 7]])          # shift = pitch, window
    x = noise_block(g["n"], g["frames"], g["input_base"])
    y = run_gpu(e, x, [256] * (g["frames"] // 256) + [g["frames"] % 256], cuda)
    got = [f"{O.fnv1a64_lr(y[0, :, i], y[1, :, i]):016x}" for i in range(g["n"])]
    assert got == g["fnv1a64"]


@pytest.mark.parametrize("n", [1, 200])
def test_chorus_vs_oracle(cuda, n):
    """The chorus kind from a pitch set before the first frame: chorus_block_rf1 (the ring-free stage)
    from frame 0 to the end.  chorus_block_v11<FULL> after a pitch or window change is
    test_gpu_chorus_ringfree.py's and test_gpu_chorus_modes.py's."""
    rng = np.random.default_rng(100 + n)
    p = chorus_params(rng, n)
    x = fast_noise(n, 4096, seed=n + 1)
    e = engine("chorus", n)
    e.set_params(0, p)
    y = run_gpu(e, x, [256] * 7 + [4, 12, 240, 2048], cuda)   # tails: partial chunks, the generic path
    ref = O.Chorus(n)
    for i in range(n):
        for f in range(8):
            ref.set(i, f, float(p[f, i]))
    yr = ref.process(x, threads=8)
    assert bits_equal(y, yr), first_mismatch(y, yr)


@pytest.mark.parametrize("kind", ["chorus", "pitchshift"])
def test_chorus_line_carry_stress(cuda, kind):
    """Extreme depth/rate/pitch/window corners over 64 blocks: every tap window mode (carried
    line, fresh reload, chorus straggler, pitch-phasor wrap) occurs many times; bit-exact.  The
    pitch-shift kind runs chorus_block_v11; the chorus kind, its pitch set before the first frame, runs
    chorus_block_rf1 throughout (the same draw on chorus_block_v11<FULL>:
    test_gpu_chorus_modes.test_ring_mode_held_blocks_with_tails)."""
    n, frames = 96, 256 * 64
    rng = np.random.default_rng(77)
    p = np.empty((8, n), np.float32)
    p[0] = rng.choice([0.0, 0.01, 1.0, 2.5, 3.0], n)      # pitch (phasor Hz)
    p[1] = rng.uniform(0, 1, n)                            # mix
    p[2] = rng.uniform(0, 0.95, n)                         # q
    p[3] = rng.uniform(0, 1, n)                            # cutoff
    p[4] = rng.uniform(0, 1, n)                            # phase
    p[5] = rng.choice([0.08, 0.2, 1.0], n)                 # depth
    p[6] = rng.choice([0.01, 0.5, 1.0], n)                 # rate
    p[7] = rng.choice([4.0, 7.3, 10.0], n)                 # window ms
    x = fast_noise(n, frames, seed=9)
    e = engine(kind, n)
    ref = O.Chorus(n, mode=0 if kind == "chorus" else 1)
    if kind == "chorus":
        e.set_params(0, p)
        for i in range(n):
            for f in range(8):
                ref.set(i, f, float(p[f, i]))
    else:
        e.set_params(0, p[[0, 7]])
        for i in range(n):
            ref.set(i, "pitch", float(p[0, i]))
            ref.set(i, "window", float(p[7, i]))
    y = run_gpu(e, x, [256] * 64, cuda)
    yr = ref.process(x, threads=8)
    assert bits_equal(y, yr), first_mismatch(y, yr)


@pytest.mark.parametrize("kind,n", [("chorus", 70), ("pitchshift", 70), ("chorus", 72), ("pitchshift", 72)])
def test_chorus_long_run_many_wraps(cuda, kind, n):
    """100,000 frames at the fastest pitch phasors (every instance's two pitch taps wrap 12 times,
    each wrap a generic chunk with direct ring reads), ragged blocks with partial chunks:
    bit-exact against the oracle.  n = 70 runs the per-lane I/O (rows need n % 4 == 0), n = 72 the
    row I/O: of chorus_block_v11 for the pitch-shift kind, of chorus_block_rf1 for the chorus kind (its
    pitch is set before the first frame, so it stays ring-free; chorus_block_v11<FULL> through phasor
    wraps and 4,096-frame launches: test_gpu_chorus_modes.test_ring_mode_held_long_run)."""
    frames = 100000
    rng = np.random.default_rng(93)
    p = chorus_params(rng, n)
    p[0] = rng.uniform(2.5, 3.0, n)                      # pitch phasor Hz
    x = fast_noise(n, frames, seed=93)
    e = engine(kind, n)
    ref = O.Chorus(n, mode=0 if kind == "chorus" else 1)
    if kind == "chorus":
        e.set_params(0, p)
        for i in range(n):
            for f in range(8):
                ref.set(i, f, float(p[f, i]))
    else:
        e.set_params(0, p[[0, 7]])
        for i in range(n):
            ref.set(i, "pitch", float(p[0, i]))
            ref.set(i, "window", float(p[7, i]))
    y = run_gpu(e, x, [4096] * 24 + [1408, 4, 12, 272], cuda)
    yr = ref.process(x, threads=8)
    assert bits_equal(y, yr), first_mismatch(y, yr)


@pytest.mark.parametrize("kind", ["chorus", "pitchshift"])
@pytest.mark.parametrize("n", [4, 36, 1028])
def test_chorus_block_kernel_edges(cuda, kind, n):
    """Row I/O (n % 4 == 0) at a single partial wave (4), a partial last wave (36, 1028), calls of
    252, 4, 8, 260, 1000 and 2048 frames (partial 16-frame chunks), extreme depth / rate corners
    (the chorus window bound): bit-exact against the oracle.  kernel_name is the kind's ring kernel;
    the chorus kind runs chorus_block_rf1 here from frame 0 to the end (Engine.chorus_ring_free)."""
    rng = np.random.default_rng(500 + n)
    p = chorus_params(rng, n)
    p[5, ::3] = 1.0                                        # depth max
    p[6, ::2] = 1.0                                        # rate max
    blocks = [252, 4, 8, 260, 1000, 2048]
    x = fast_noise(n, sum(blocks), seed=n)
    e = engine(kind, n)
    ref = O.Chorus(n, mode=0 if kind == "chorus" else 1)
    if kind == "chorus":
        e.set_params(0, p)
        for i in range(n):
            for f in range(8):
                ref.set(i, f, float(p[f, i]))
    else:
        e.set_params(0, p[[0, 7]])
        for i in range(n):
            ref.set(i, "pitch", float(p[0, i]))
            ref.set(i, "window", float(p[7, i]))
    assert e.kernel_name == "chorus_block_v11"
    y = run_gpu(e, x, blocks, cuda)
    yr = ref.process(x, threads=8)
    assert bits_equal(y, yr), first_mismatch(y, yr)


def test_chorus_defaults_and_edges(cuda):
    """RNBO defaults, params clamped to @min/@max (out-of-range values), mix 0 == dry."""
    n = 5
    e = engine("chorus", n)
    ref = O.Chorus(n)
    edits = [(1, "rate", 5.0), (2, "depth", 0.0), (3, "mix", 0.0), (4, "pitch", -2.0), (4, "q", 1.0)]
    for i, f, v in edits:
        e.set_param(i, f, v)
        ref.set(i, f, v)
    x = fast_noise(n, 2048, seed=3)
    y = run_gpu(e, x, [1024, 1024], cuda)
    assert bits_equal(y, ref.process(x))
    assert bits_equal(y[:, :, 3], x[:, :, 3])


def test_chorus_full_size_properties(cuda):
    """65,536 chorus instances (BASELINE config 2): sampled instances exact vs oracle."""
    import torch
    n, frames = 65536, 512
    rng = np.random.default_rng(12)
    p = chorus_params(rng, n)
    g = torch.Generator(device=cuda).manual_seed(1)
    x = torch.rand((2, frames, n), generator=g, device=cuda) - 0.5
    e = engine("chorus", n)
    e.set_params(0, p)
    y = torch.cat([e.process(x[:, :256].contiguous()), e.process(x[:, 256:].contiguous())], 1)
    torch.cuda.synchronize()
    assert torch.isfinite(y).all()
    idx = np.array([0, 1, 63, 64, 40000, 65535], np.int64)
    ref = O.Chorus(len(idx))
    for k, i in enumerate(idx):
        for f in range(8):
            ref.set(k, f, float(p[f, i]))
    yr = ref.process(np.ascontiguousarray(x[:, :, idx].cpu().numpy()))
    assert bits_equal(y[:, :, idx].cpu().numpy(), yr)


# ------------------------------------------------------------------------------------- voice
def _voice_pair(n, cfg, notes, on=True, kind="voice"):
    e = engine(kind, n)
    ref = O.Voice(n, moog=kind == "voice_moog")
    if cfg is not None:
        e.set_params(0, cfg)
        for i in range(n):
            ref.config(i, cfg[:, i])
    if on:
        e.note_events([(i, 1, notes[i]) for i in range(n)])
        for i in range(n):
            ref.note(i, True, notes[i])
    return e, ref


def _voice_run(e, frames, cuda):
    import torch
    out = torch.empty((1, frames, e.n), device=cuda)
    e.process(None, out=out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("kind", ["voice", "voice_moog"])
def test_voice_vs_oracle(cuda, kind):
    """SvfFilter voice and MoogFilter (daisysp::LadderFilter) voice against the oracle, through a
    NoteOn and a NoteOff."""
    n = 256
    rng = np.random.default_rng(21)
    cfg = voice_configs(rng, n)
    notes = [int(v) for v in rng.integers(36, 97, n)]
    e, ref = _voice_pair(n, cfg, notes, kind=kind)
    ya = np.concatenate([_voice_run(e, 256, cuda) for _ in range(8)], 1)
    yra = ref.process(2048)
    e.note_events([(i, 0, notes[i]) for i in range(n)])
    for i in range(n):
        ref.note(i, False, notes[i])
    yb = np.concatenate([_voice_run(e, 256, cuda) for _ in range(8)], 1)
    yrb = ref.process(2048)
    y, yr = np.concatenate([ya, yb], 1), np.concatenate([yra, yrb], 1)
    assert np.all(np.isfinite(y))
    assert rel_err(y[0].T, yr[0].T) <= VOICE_TOL
    # pointwise view: |d| / |ref| where |ref| is above 1e-3 of the voice's rms
    # (near zero crossings the ratio is meaningless), the share of bit-identical samples, and the
    # largest absolute error relative to the voice's peak
    d = np.abs(y[0].astype(np.float64) - yr[0])
    ref = np.abs(yr[0].astype(np.float64))
    rms = np.sqrt(np.mean(yr[0].astype(np.float64) ** 2, axis=0, keepdims=True))
    big = ref > 1e-3 * rms
    pw = d[big] / ref[big]
    exact = float(np.mean(y[0] == yr[0]))
    print(f"{kind}: pointwise rel err p50 {np.median(pw):.2e} p99 {np.quantile(pw, 0.99):.2e} "
          f"max {pw.max():.2e}; bit-identical samples {100 * exact:.1f} %; "
          f"max |d| / peak {np.max(d / np.maximum(ref.max(axis=0, keepdims=True), 1e-30)):.2e}")
    # measured (MI355X, round 4: contracted kernels against the unfused oracle): Svf voice p99
    # 2.3e-6, max 4.5e-4, 59.0 % bit-identical; Moog p99 2.1e-6, max 5.1e-4, 44.4 % bit-identical;
    # max |d| / peak 4.2e-7 / 5.8e-7
    assert np.quantile(pw, 0.99) <= 1e-5
    # explicit pointwise bound: p99 and max of |d| / |ref| where |ref| is above
    # 1e-3 of the voice's rms, at the values DESIGN.md section 2 states (with margin: 2.3e-6 / 4.5e-4
    # for the Svf voice, 2.1e-6 / 5.1e-4 for the Moog voice)
    assert np.quantile(pw, 0.99) <= 5e-6 and pw.max() <= 1e-3


def voice_bits_equal(y, yr):
    """Bit-exact where the oracle is finite, the same non-finite pattern elsewhere (a diverging Svf
    produces inf/NaN in the reference arithmetic too; NaN payloads are not compared)."""
    fin = np.isfinite(yr)
    if not np.array_equal(fin, np.isfinite(y)):
        return False
    return np.array_equal(y[fin].view(np.uint32), yr[fin].view(np.uint32))


@pytest.mark.parametrize("kind", ["voice", "voice_moog"])
def test_voice_bit_exact_kernel_arith(cuda, rcp_table, kind):
    """the GPU voices BIT-EXACT against the oracle's kernel-arithmetic mode
    (oracle/voice_ref.c: the same contractions, sine polynomial and v_rcp model), so that an
    indexing or event-timing bug of any size shows.  Half the voices configured, half at Init's
    defaults; NoteOn / NoteOff / GateOn / GateOff / SetFrequency storms at block boundaries; ragged
    blocks (4..300 frames: partial chunks); a config change and Process-read member writes
    (olfx_set_member of filter_cutoff, filter_env_amount, amp_env_amount after Update()) mid-run."""
    from ol_dsp_amd import _lib
    n = 200
    rng = np.random.default_rng(2024)
    e = engine(kind, n)
    ref = O.Voice(n, moog=kind == "voice_moog", kernel_arith=True)
    cfg = voice_configs(rng, n)
    conf = np.arange(n) % 2 == 0
    for i in np.flatnonzero(conf):
        e.set_params(0, cfg[:, i:i + 1], first=int(i))
        ref.config(int(i), cfg[:, i])
    ys, yrs, total, b = [], [], 0, 0
    while total < 6000:
        if b == 9:                                   # a new config for a third of the voices
            who = np.flatnonzero(rng.random(n) < 1 / 3)
            new = voice_configs(rng, n)
            for i in who:
                e.set_params(0, new[:, i:i + 1], first=int(i))
                ref.config(int(i), new[:, i])
                cfg[:, i] = new[:, i]
                conf[i] = True
        if b == 14:                                  # members Process reads, written after Update()
            for i in np.flatnonzero(conf)[:40]:
                for f, lo, hi in ((0, 100.0, 8000.0), (3, 0.0, 1.0), (9, 0.2, 1.0)):
                    v = np.float32(rng.uniform(lo, hi))
                    assert e.lib.olfx_set_member(e.handle, int(i), f, float(v)) == 0
                    cfg[f, i] = v
                ref.config(int(i), cfg[:, i])        # the same members, the rest unchanged
        evs = []
        for i in np.flatnonzero(rng.random(n) < (1.0 if b == 0 else 0.3)):
            t = 1 if b == 0 else int(rng.integers(0, 5))
            evs.append((int(i), t, int(rng.integers(30, 100)), float(rng.uniform(30.0, 3000.0))))
        e.voice_events(evs)
        for i, t, note, hz in evs:
            ref.event(i, t, note, hz if t == _lib.EV_SET_FREQUENCY else 0.0)
        fr = int(rng.choice([256, 256, 4, 12, 100, 300, 37 * 4]))
        ys.append(_voice_run(e, fr, cuda))
        yrs.append(ref.process(fr))
        total += fr
        b += 1
    y, yr = np.concatenate(ys, 1), np.concatenate(yrs, 1)
    assert np.isfinite(yr).mean() > 0.9
    assert voice_bits_equal(y, yr), first_mismatch(y, yr)


@pytest.mark.parametrize("kind", ["voice", "voice_moog"])
def test_voice_long_run_event_storm(cuda, kind):
    """200 blocks with NoteOn / NoteOff for a random third of the voices at every block boundary
    (retriggers in attack, decay, sustain and release; notes repeated and changed, so portamento
    and both envelopes restart from every segment) and a config change half way: the voices stay
    within the parity tolerance of the oracle and finite."""
    n, blocks = 128, 200
    rng = np.random.default_rng(57)
    cfg = voice_configs(rng, n)
    notes = [int(v) for v in rng.integers(36, 97, n)]
    e, ref = _voice_pair(n, cfg, notes, kind=kind)
    ys, yrs = [], []
    for b in range(blocks):
        if b == blocks // 2:
            cfg = voice_configs(rng, n)
            e.set_params(0, cfg)
            for i in range(n):
                ref.config(i, cfg[:, i])
        if b:
            who = np.flatnonzero(rng.random(n) < 1 / 3)
            on = rng.random(len(who)) < 0.5
            nn = rng.integers(36, 97, len(who))
            ev = [(int(i), int(o), int(m)) for i, o, m in zip(who, on, nn)]
            e.note_events(ev)
            for i, o, m in ev:
                ref.note(i, bool(o), m)
        ys.append(_voice_run(e, 256, cuda))
        yrs.append(ref.process(256))
    y, yr = np.concatenate(ys, 1), np.concatenate(yrs, 1)
    assert np.all(np.isfinite(y))
    assert rel_err(y[0].T, yr[0].T) <= VOICE_TOL


@pytest.mark.parametrize("kind", ["voice", "voice_moog"])
def test_voice_tiny_ragged_blocks(cuda, kind):
    """Voices rendered in 4..40-frame callbacks (partial 16-sample chunks, one launch each) with
    note events between them: within the parity tolerance of the oracle run as one stream."""
    n = 70
    rng = np.random.default_rng(88)
    cfg = voice_configs(rng, n)
    notes = [int(v) for v in rng.integers(36, 97, n)]
    e, ref = _voice_pair(n, cfg, notes, kind=kind)
    ys, yrs, total = [], [], 0
    while total < 3000:
        b = 4 * int(rng.integers(1, 11))
        if total and rng.random() < 0.2:
            who = np.flatnonzero(rng.random(n) < 0.5)
            ev = [(int(i), int(rng.random() < 0.5), int(rng.integers(36, 97))) for i in who]
            e.note_events(ev)
            for i, o, m in ev:
                ref.note(i, bool(o), m)
        ys.append(_voice_run(e, b, cuda))
        yrs.append(ref.process(b))
        total += b
    y, yr = np.concatenate(ys, 1), np.concatenate(yrs, 1)
    assert np.all(np.isfinite(y))
    assert rel_err(y[0].T, yr[0].T) <= VOICE_TOL


def test_voice_golden_and_pins(cuda, golden):
    g = golden["voice"]
    p = np.asarray(g["params"], np.float32)
    e, _ = _voice_pair(g["n"], p, g["notes"])
    ya = _voice_run(e, g["note_off_at"], cuda)
    e.note_events([(i, 0, g["notes"][i]) for i in range(g["n"])])
    yb = _voice_run(e, g["frames"] - g["note_off_at"], cuda)
    y = np.concatenate([ya, yb], 1)
    vo = O.Voice(g["n"])
    for i in range(g["n"]):
        vo.config(i, p[:, i])
        vo.note(i, True, g["notes"][i])
    yr = vo.process(g["note_off_at"])
    for i in range(g["n"]):
        vo.note(i, False, g["notes"][i])
    yr = np.concatenate([yr, vo.process(g["frames"] - g["note_off_at"])], 1)
    assert rel_err(y[0].T, yr[0].T) <= VOICE_TOL
    # synth_test.cpp:102-148 pins, on the GPU: NoteOn, NoteOff, first sample == 0
    e2 = engine("voice", 1)
    e2.note_events([(0, 1, 60), (0, 0, 60)])
    assert _voice_run(e2, 4, cuda)[0, 0, 0] == 0
    e2.note_events([(0, 1, 60)])
    v = _voice_run(e2, 4, cuda)[0, :, 0]
    assert v[1] != 0 and v[1] != 1


@pytest.mark.parametrize("kind", ["voice", "voice_moog"])
def test_voice_unconfigured_defaults(cuda, kind):
    """Init without Update: DaisySP defaults in envelopes and Svf / LadderFilter (SynthVoice.h:31-39)."""
    n = 4
    notes = [40, 60, 72, 90]
    e, ref = _voice_pair(n, None, notes, kind=kind)
    y = np.concatenate([_voice_run(e, 512, cuda) for _ in range(4)], 1)
    yr = ref.process(2048)
    assert rel_err(y[0].T, yr[0].T) <= VOICE_TOL


@pytest.mark.parametrize("kind", ["voice", "voice_moog"])
def test_voice_gate_frequency_update_events(cuda, kind):
    """Voice.h:33-57 calls beyond NoteOn/NoteOff through olfx_voice_events / olfx_update:
    GateOff then GateOn without retrigger (SynthVoice.h:231-239), SetFrequency (:264-267) under
    portamento, and Update() alone (member defaults, SynthVoice.h:285-311) on voices never
    configured; each lands at the next block, in order, against the oracle."""
    from ol_dsp_amd import _lib
    n = 64
    rng = np.random.default_rng(33)
    cfg = voice_configs(rng, n)
    cfg[15, :] = rng.uniform(0.0, 0.01, n).astype(np.float32)     # portamento: SetFrequency glides
    notes = [int(v) for v in rng.integers(36, 97, n)]
    e, ref = _voice_pair(n, cfg, notes, kind=kind)
    half = n // 2
    # a second bank never configured: Update() only (the engine's default params == the members')
    e2, ref2 = _voice_pair(n, None, notes, kind=kind)
    e2.update(0, n)
    defaults = np.asarray([[0.0, 0.0, 0.0, 1.0, 0.0, 1.0, 0.2, 0.0, 0.0, 0.8, 0.01, 1.0, 0.0, 1.0, 0.01, 0.0]],
                          np.float32).T.repeat(n, 1)
    for i in range(n):
        ref2.config(i, defaults[:, i])
    ys, yrs, y2, yr2 = [], [], [], []
    for blk in range(8):
        if blk == 2:
            e.voice_events([(i, _lib.EV_SET_FREQUENCY, 0, 110.0 * (1 + i % 7)) for i in range(half)])
            for i in range(half):
                ref.event(i, 4, 0, 110.0 * (1 + i % 7))
        if blk == 3:
            e.voice_events([(i, _lib.EV_GATE_OFF) for i in range(n)])
            for i in range(n):
                ref.event(i, 3)
        if blk == 5:
            e.voice_events([(i, _lib.EV_GATE_ON) for i in range(0, n, 2)] +
                           [(i, _lib.EV_NOTE_ON, 60) for i in range(1, n, 2)])
            for i in range(n):
                ref.event(i, 2 if i % 2 == 0 else 1, 60)
            e2.voice_events([(i, _lib.EV_GATE_OFF) for i in range(n)])
            for i in range(n):
                ref2.event(i, 3)
        ys.append(_voice_run(e, 256, cuda))
        yrs.append(ref.process(256))
        y2.append(_voice_run(e2, 256, cuda))
        yr2.append(ref2.process(256))
    y, yr = np.concatenate(ys, 1), np.concatenate(yrs, 1)
    assert np.all(np.isfinite(y))
    assert rel_err(y[0].T, yr[0].T) <= VOICE_TOL
    y2, yr2 = np.concatenate(y2, 1), np.concatenate(yr2, 1)
    assert np.any(yr2 != 0)
    assert rel_err(y2[0].T, yr2[0].T) <= VOICE_TOL


def test_voice_moog_golden_and_state_carry(cuda, golden):
    """MoogFilter voices against the frozen fixture, in ragged blocks (the LadderFilter state and
    oldinput_ carry across launches), plus the synth_test.cpp:102-148 first-sample pin."""
    g = golden["voice_moog"]
    p = np.asarray(g["params"], np.float32)
    e, _ = _voice_pair(g["n"], p, g["notes"], kind="voice_moog")
    parts, done = [], 0
    for b in (4, 12, 60, 700, g["note_off_at"] - 776):     # olfx_process: multiples of 4
        parts.append(_voice_run(e, b, cuda))
        done += b
    assert done == g["note_off_at"]
    e.note_events([(i, 0, g["notes"][i]) for i in range(g["n"])])
    parts.append(_voice_run(e, g["frames"] - g["note_off_at"], cuda))
    y = np.concatenate(parts, 1)
    vo = O.Voice(g["n"], moog=True)
    for i in range(g["n"]):
        vo.config(i, p[:, i])
        vo.note(i, True, g["notes"][i])
    yr = vo.process(g["note_off_at"])
    for i in range(g["n"]):
        vo.note(i, False, g["notes"][i])
    yr = np.concatenate([yr, vo.process(g["frames"] - g["note_off_at"])], 1)
    assert [f"{O.fnv1a64_lr(yr[0, :, i], yr[0, :, i]):016x}" for i in range(g["n"])] == g["fnv1a64"]
    assert np.all(np.isfinite(y))
    assert rel_err(y[0].T, yr[0].T) <= VOICE_TOL
    e2 = engine("voice_moog", 1)
    e2.note_events([(0, 1, 60)])
    v = _voice_run(e2, 4, cuda)[0, :, 0]
    assert v[0] == 0 and v[1] != 0 and v[1] != 1


# ------------------------------------------------------------------------------------- chain
def test_chain_vs_composed_oracle(cuda):
    n = 96
    rng = np.random.default_rng(31)
    pc = chorus_params(rng, n)
    pp = chorus_params(rng, n)[[0, 7]]
    pd = dt_params(rng, n, 0.1)
    p = np.concatenate([pc, pp, pd], 0)
    x = fast_noise(n, 2048, seed=31)
    e = engine("chain", n)
    e.set_params(0, p)
    y = run_gpu(e, x, [256] * 8, cuda)
    c1, c2, d = O.Chorus(n), O.Chorus(n, mode=1), O.Dattorro(n)
    for i in range(n):
        for f in range(8):
            c1.set(i, f, float(pc[f, i]))
        c2.set(i, "pitch", float(pp[0, i]))
        c2.set(i, "window", float(pp[1, i]))
        for f in range(7):
            d.set(i, f, float(pd[f, i]))
    yr = d.process(c2.process(c1.process(x)))
    assert bits_equal(y, yr), first_mismatch(y, yr)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 68, 129])
def test_chain_ragged_groups_and_short_blocks(cuda, n):
    """The chain's stages at group edges (the pitch role's stereo lanes past the last instance mirror
    it; one, two and three 64-instance groups, the last partial) and blocks of 4 and 20 frames (a
    lone short chunk, a full chunk plus a short one): bit-exact against the composed oracle."""
    rng = np.random.default_rng(53 + n)
    pc, pp, pd = chorus_params(rng, n), chorus_params(rng, n)[[0, 7]], dt_params(rng, n, 0.0)
    pd[0] = rng.uniform(0, 0.05, n)
    x = fast_noise(n, 600, seed=53 + n)
    e = engine("chain", n)
    e.set_params(0, np.concatenate([pc, pp, pd], 0))
    y = run_gpu(e, x, [4, 20, 256, 4, 316], cuda)
    c1, c2, d = _chain_oracle(n, pc, pp, pd)
    yr = d.process(c2.process(c1.process(x)))
    assert bits_equal(y, yr), first_mismatch(y, yr)


def _chain_oracle(n, pc, pp, pd):
    c1, c2, d = O.Chorus(n), O.Chorus(n, mode=1), O.Dattorro(n)
    _chain_oracle_set(c1, c2, d, n, pc, pp, pd)
    return c1, c2, d


def _chain_oracle_set(c1, c2, d, n, pc, pp, pd):
    for i in range(n):
        for f in range(8):
            c1.set(i, f, float(pc[f, i]))
        c2.set(i, "pitch", float(pp[0, i]))
        c2.set(i, "window", float(pp[1, i]))
        for f in range(7):
            d.set(i, f, float(pd[f, i]))


def test_chain_predelays_long_run_and_param_change(cuda):
    """The fused chain over 70,000 frames (the reverb's uint16 t passes the t = 32,768 modulation
    turn and wraps, the chorus and pitch rings wrap many times), per-instance pre-delays on both
    sides of the chunk and row edges of the row-layout ring (0..20, 28..33, 47, 48: a window partly
    in the chunk's own input), the block edges, the maximum and past it (8176..8191 read positions
    the launch has not yet overwritten; 8192 acts as 0), chunks starting off a row (blocks of 4 and
    132 frames shift t0 by 4 and 8 mod 16), a ragged instance count (two groups, the second
    partial) and every parameter changed at frame 35,000: bit-exact against the composed oracle."""
    n = 100
    rng = np.random.default_rng(41)
    pc, pp, pd = chorus_params(rng, n), chorus_params(rng, n)[[0, 7]], dt_params(rng, n, 0.0)
    edge = np.array([0, 1, 3, 4, 7, 8, 9, 12, 13, 15, 16, 17, 19, 20, 28, 31, 32, 33, 47, 48, 255, 256, 257,
                     4799, 4800, 8176, 8177, 8180, 8190, 8191, 8192, 8200], np.float64) / 4800
    pd[0] = rng.uniform(0, 1, n)
    pd[0, 64:64 + len(edge)] = edge
    pd[0, :8] = edge[:8]
    x = fast_noise(n, 70000, seed=41)
    e = engine("chain", n)
    e.set_params(0, np.concatenate([pc, pp, pd], 0))
    y1 = run_gpu(e, x[:, :35000], [4096] * 8 + [2096, 4, 132], cuda)
    c1, c2, d = _chain_oracle(n, pc, pp, pd)
    yr1 = d.process(c2.process(c1.process(x[:, :35000])))
    pc2, pp2, pd2 = chorus_params(rng, n), chorus_params(rng, n)[[0, 7]], dt_params(rng, n, 0.0)
    pd2[0] = rng.uniform(0, 1, n)
    e.set_params(0, np.concatenate([pc2, pp2, pd2], 0))
    _chain_oracle_set(c1, c2, d, n, pc2, pp2, pd2)
    y2 = run_gpu(e, x[:, 35000:], [4096] * 8 + [2232], cuda)
    yr2 = d.process(c2.process(c1.process(x[:, 35000:])))
    y, yr = np.concatenate([y1, y2], 1), np.concatenate([yr1, yr2], 1)
    assert bits_equal(y, yr), first_mismatch(y, yr)


def test_chain_predelays_at_the_row_window_edges(cuda):
    """The chain's reverb role with 64-instance groups whose pre-delays all sit near the edges of its
    row window (dattorro_stage.h rows_network: a chunk reads positions of its own chunk below 16,
    its row prefetch two chunks ahead reaches the chunk below 48): all in 48..63, one at 47 among
    48..63, 48..8191, a partial fourth group at 48; blocks that start chunks off a row (4, 132
    frames) and end on partial chunks: bit-exact against the composed oracle."""
    n = 200
    rng = np.random.default_rng(77)
    pc, pp, pd = chorus_params(rng, n), chorus_params(rng, n)[[0, 7]], dt_params(rng, n, 0.0)
    smp = np.concatenate([rng.integers(48, 64, 64), rng.integers(48, 64, 64), rng.integers(48, 8192, 64),
                          np.full(8, 48)]).astype(np.float64)
    smp[0] = 48
    smp[64 + 17] = 47
    pd[0] = (smp + 0.5) / 4800                   # uint16(value * 4800) = smp
    x = fast_noise(n, 6000, seed=77)
    e = engine("chain", n)
    e.set_params(0, np.concatenate([pc, pp, pd], 0))
    y = run_gpu(e, x, [256, 4, 132, 1024, 36, 2048, 500, 2000], cuda)
    c1, c2, d = _chain_oracle(n, pc, pp, pd)
    yr = d.process(c2.process(c1.process(x)))
    assert bits_equal(y, yr), first_mismatch(y, yr)


# ------------------------------------------------------------------------------- fx rack
def _fxrack_pair(n, p):
    e = engine("fxrack", n)
    e.set_params(0, p)
    ref = O.FxRack(n)
    for i in range(n):
        for f in range(p.shape[0]):
            ref.set(i, f, float(p[f, i]))
    return e, ref


@pytest.mark.parametrize("n", [36, 37, 96])
def test_fxrack_vs_oracle(cuda, n):
    """FxRack<2> bit-exact against the oracle: ragged instance counts, partial chunks, and
    delays from 0 to 47999 samples (every 4th instance shorter than a chunk)."""
    rng = np.random.default_rng(n)
    p = fxrack_params(rng, n)
    p[0, 1] = 1.0                     # the clamp to 47,999
    p[0, 2] = 0.0                     # delay 0: reads the sample written 48,000 frames ago
    x = fast_noise(n, 3000, seed=n)
    e, ref = _fxrack_pair(n, p)
    y = run_gpu(e, x, [256] * 5 + [4, 12, 240, 1464], cuda)
    yr = ref.process(x, threads=8)
    assert bits_equal(y, yr), first_mismatch(y, yr)


def test_fxrack_long_run_wraps_and_param_change(cuda):
    """110,000 frames: the 48,000-position rings wrap twice; the delay time changes between
    blocks (DelayFx::Update, Fx.h:209-216)."""
    n = 64
    rng = np.random.default_rng(5)
    p = fxrack_params(rng, n)
    x = fast_noise(n, 110000, seed=5)
    e, ref = _fxrack_pair(n, p)
    y1 = run_gpu(e, x[:, :60000], [4096] * 14 + [2656], cuda)
    yr1 = ref.process(x[:, :60000], threads=8)
    p2 = fxrack_params(rng, n)
    e.set_params(0, p2[:1])
    for i in range(n):
        ref.set(i, 0, float(p2[0, i]))
    y2 = run_gpu(e, x[:, 60000:], [4096] * 12 + [848], cuda)
    yr2 = ref.process(x[:, 60000:], threads=8)
    y, yr = np.concatenate([y1, y2], 1), np.concatenate([yr1, yr2], 1)
    assert bits_equal(y, yr), first_mismatch(y, yr)


def test_fxrack_firmware_topology(cuda):
    """OLFX_FR_TOPOLOGY 1, the Daisy synth firmware's callback (ol_daisy/app/synth/main.cpp:78-86:
    DelayFx<1> -> stereo copy -> ReverbFx<2> -> FilterFx<2> in place, no master), mixed with
    FxRack<2> instances in one engine: bit-exact against the oracle; channel 1 of a firmware
    instance is its reverb output and does not depend on input channel 1."""
    n = 96
    rng = np.random.default_rng(77)
    p = np.concatenate([fxrack_params(rng, n), np.zeros((1, n), np.float32)], 0)
    p[11, 1::2] = 1.0
    x = fast_noise(n, 1200, seed=77)
    e, ref = _fxrack_pair(n, p)
    y = run_gpu(e, x, [256, 256, 4, 684], cuda)
    yr = ref.process(x, threads=8)
    assert bits_equal(y, yr), first_mismatch(y, yr)
    assert np.any(y[1, :, 1::2] != 0) and np.all(y[1, :, 0::2] == 0)
    x2 = x.copy()
    x2[1] = fast_noise(n, 1200, seed=78)[1]          # another input channel 1
    e2, _ = _fxrack_pair(n, p)
    y2 = run_gpu(e2, x2, [1200], cuda)
    assert bits_equal(y2[:, :, 1::2], y[:, :, 1::2])


def test_fxrack_golden_and_channel1_silent(cuda, golden):
    g = golden["fxrack"]
    p = np.asarray(g["params"], np.float32)
    x = noise_block(g["n"], g["frames"], g["input_base"])
    e = engine("fxrack", g["n"])
    e.set_params(0, p)
    y = run_gpu(e, x, [2048] * 29 + [608], cuda)
    assert [f"{O.fnv1a64_lr(y[0, :, i], y[1, :, i]):016x}" for i in range(g["n"])] == g["fnv1a64"]
    assert np.all(y[1] == 0)



# ------------------------------------------------------------------- control changes (8f row 4)
def _tiny_blocks(rng, total):
    """Random block lengths, multiples of 4 from 4 to 40 frames, summing to total."""
    out, left = [], total
    while left > 0:
        b = min(left, 4 * int(rng.integers(1, 11)))
        out.append(b)
        left -= b
    return out


@pytest.mark.parametrize("kind", ["chain", "chorus", "pitchshift", "dattorro", "fxrack"])
@pytest.mark.parametrize("n", [1, 70])
def test_tiny_ragged_blocks(cuda, kind, n):
    """Host callbacks of 4..40 frames (every chunk partial or short, one launch per callback),
    a single instance and a ragged count: bit-exact against the oracle."""
    rng = np.random.default_rng(1000 + n)
    frames = 3000
    x = fast_noise(n, frames, seed=n + 7)
    blocks = _tiny_blocks(rng, frames)
    e = engine(kind, n)
    if kind == "chain":
        pc, pp, pd = chorus_params(rng, n), chorus_params(rng, n)[[0, 7]], dt_params(rng, n, 0.0)
        pd[0] = rng.uniform(0, 0.01, n)                  # pre-delays 0..48: registers and ring
        e.set_params(0, np.concatenate([pc, pp, pd], 0))
        c1, c2, d = _chain_oracle(n, pc, pp, pd)
        yr = d.process(c2.process(c1.process(x)))
    elif kind in ("chorus", "pitchshift"):
        p = chorus_params(rng, n)
        p[0, ::3] = 3.0                                  # fastest phasor: wraps inside the run
        ref = O.Chorus(n, mode=0 if kind == "chorus" else 1)
        if kind == "chorus":
            e.set_params(0, p)
            for i in range(n):
                for f in range(8):
                    ref.set(i, f, float(p[f, i]))
        else:
            e.set_params(0, p[[0, 7]])
            for i in range(n):
                ref.set(i, "pitch", float(p[0, i]))
                ref.set(i, "window", float(p[7, i]))
        yr = ref.process(x, threads=8)
    elif kind == "dattorro":
        p = dt_params(rng, n, 0.0)
        p[0] = rng.uniform(0, 0.01, n)
        e.set_params(0, p)
        ref = O.Dattorro(n)
        for i in range(n):
            for f in range(7):
                ref.set(i, f, float(p[f, i]))
        yr = ref.process(x, threads=8)
    else:
        p = np.concatenate([fxrack_params(rng, n), np.zeros((1, n), np.float32)], 0)
        p[11, ::2] = 1.0
        e, ref = _fxrack_pair(n, p)
        yr = ref.process(x, threads=8)
    y = run_gpu(e, x, blocks, cuda)
    assert bits_equal(y, yr), first_mismatch(y, yr)


def test_control_changes_equal_mapped_params(cuda):
    """olfx_control applies the reference's CC handlers: an engine driven by MIDI / hardware
    control changes matches one given the mapped values by set_param (bit-exact), and the fx
    rack also matches the oracle configured with those values."""
    import ol_dsp_amd as ofx
    n = 8
    evs = [(i, cc, v) for i in range(n) for cc, v in ((35, 3 + 9 * i), (36, 50), (39, 80), (37, 70),
                                                      (45, 90), (47, 20 * i % 128), (34, 64), (7, 100))]
    evs += [(0, 45, 0.3, "hw"), (1, 35, 0.25, "hw"), (2, 32, 99)]       # cc 32: reverb stub, ignored
    e1, e2 = engine("fxrack", n), engine("fxrack", n)
    e1.control(evs)
    ref = O.FxRack(n)
    for ev in evs:
        m = ofx.control_map("fxrack", ev[1], ev[2], ev[3] if len(ev) > 3 else "midi")
        if m is not None:
            e2.set_param(ev[0], m[0], m[1])
            ref.set(ev[0], m[0], m[1])
    x = fast_noise(n, 2048, seed=8)
    y1, y2 = run_gpu(e1, x, [256] * 8, cuda), run_gpu(e2, x, [256] * 8, cuda)
    yr = ref.process(x)
    assert bits_equal(y1, y2) and bits_equal(y1, yr), first_mismatch(y1, yr)

    # voice: cutoff / envelope CCs, and osc_1_mix (cc 114), which only re-runs Update() --
    # an unconfigured voice then leaves the DaisySP defaults for the SynthVoice member values
    nv = 4
    vevs = [(0, 41, 90), (0, 75, 40), (1, 5, 30), (2, 114, 64), (3, 41, 0.5, "hw")]
    v1, v2 = engine("voice", nv), engine("voice", nv)
    v1.control(vevs)
    for ev in vevs:
        m = ofx.control_map("voice", ev[1], ev[2], ev[3] if len(ev) > 3 else "midi")
        if m[0] == "update_only":
            v2.set_param(ev[0], 0, v2.get_param(ev[0], 0))    # configure with unchanged members
        else:
            v2.set_param(ev[0], m[0], m[1])
    for v in (v1, v2):
        v.note_events([(i, 1, 48 + 5 * i) for i in range(nv)])
    a, b = _voice_run(v1, 1024, cuda), _voice_run(v2, 1024, cuda)
    assert bits_equal(a, b), first_mismatch(a, b)


# ---------------------------------------------------------- voice buses: Polyvoice (8a A17)
def test_mix_buses_bit_exact(cuda):
    """olfx_mix adds each bus's voices in list order, one float add per voice: bit-identical to the
    reference's `*frame_out += frame_buffer` (Polyvoice.h:28-33) over the same voice samples, on
    the device and through host buffers, accumulating into a non-zero bus buffer; ragged buses."""
    import torch
    n = 300
    rng = np.random.default_rng(5)
    cfg = voice_configs(rng, n)
    cfg[2] *= 0.25              # moderate Svf drive: every voice stays finite (NaN payloads differ)
    notes = [int(v) for v in rng.integers(36, 97, n)]
    e, _ = _voice_pair(n, cfg, notes)
    perm = [int(v) for v in rng.permutation(n)]
    buses = [perm[k:k + 8] for k in range(0, 240, 8)] + [perm[240:241], [], perm[241:300]]
    e.mix_config(buses)
    assert e.n_buses == len(buses)
    y = _voice_run(e, 512, cuda)
    assert np.all(np.isfinite(y))
    init = rng.standard_normal((512, len(buses))).astype(np.float32)
    want = O.mix_ref(y, buses, init)
    dev = e.mix(torch.from_numpy(y).to(cuda), torch.from_numpy(init.copy()).to(cuda))
    torch.cuda.synchronize()
    assert bits_equal(dev.cpu().numpy(), want)
    assert bits_equal(e.mix(y, init.copy()), want)
    # a frame count off the kernel's four-frame step: the tail frames take the scalar path
    assert bits_equal(e.mix(np.ascontiguousarray(y[..., :509, :]), init[:509].copy()), want[:509])
    back = perm[241:300][::-1]                   # the order of the adds is the list's
    e.mix_config([back])
    assert bits_equal(e.mix(y), O.mix_ref(y, [back]))


@pytest.mark.parametrize("n,sizes", [(300, [8]), (3000, [8]), (2000, [4, 12, 0, 8, 20]), (2100, [1, 7, 0, 12, 3])])
def test_mix_contiguous_buses_bit_exact(cuda, n, sizes):
    """Buses that are contiguous voice runs in voice order: on multiples of 4 voices (voice_mix_v4:
    float4 runs) -- buses of 8 (the bench's Polyvoice layout; 3000 voices -> 375 buses, more than
    one block of 256), a last bus of 4 (300), ragged runs of 4..20 with empty buses -- and off them
    (2100: voice_mix_v2); frame counts on and off the four-frame step: bit-identical to Polyvoice's
    in-order adds into a non-zero bus buffer."""
    import torch
    rng = np.random.default_rng(n)
    cfg = voice_configs(rng, n)
    cfg[2] *= 0.25
    notes = [int(v) for v in rng.integers(36, 97, n)]
    e, _ = _voice_pair(n, cfg, notes)
    buses, v, k = [], 0, 0
    while v < n:
        m = min(sizes[k % len(sizes)], n - v)
        buses.append(list(range(v, v + m)))
        v += m
        k += 1
    e.mix_config(buses)
    y = _voice_run(e, 256, cuda)
    assert np.all(np.isfinite(y))
    init = rng.standard_normal((256, len(buses))).astype(np.float32)
    want = O.mix_ref(y, buses, init)
    dev = e.mix(torch.from_numpy(y).to(cuda), torch.from_numpy(init.copy()).to(cuda))
    torch.cuda.synchronize()
    assert bits_equal(dev.cpu().numpy(), want)
    assert bits_equal(e.mix(np.ascontiguousarray(y[..., :250, :]), init[:250].copy()), want[:250])


def test_mix_config_rejects_bad_lists(cuda):
    import ol_dsp_amd as ofx
    e = engine("voice", 16)
    for bad in ([[0, 1], [1]], [[16]]):
        with pytest.raises(ofx.OlfxError):
            e.mix_config(bad)
    with pytest.raises(ofx.OlfxError):            # no buses configured
        e.mix(np.zeros((1, 4, 16), np.float32))
    e.mix_config([[3, 2], [5]])
    assert e.n_buses == 2
    e.mix_config([])
    assert e.n_buses == 0
    with pytest.raises(ofx.OlfxError):
        engine("chorus", 4).mix_config([[0]])


def test_polyvoice_allocation_vs_oracle(cuda):
    """ol::synth::Polyvoice (Polyvoice.h:35-51): NoteOn takes the group's first voice not Playing(),
    NoteOff its first voice Playing() that note.  The GPU voices follow oracle voices driven by that
    rule (within the voice tolerance) and every bus is the in-order sum of its voices."""
    import torch
    import ol_dsp_amd as ofx
    n, k = 12, 3
    rng = np.random.default_rng(8)
    cfg = voice_configs(rng, n)
    cfg[2] *= 0.25
    e, ref = _voice_pair(n, cfg, None, on=False)
    groups = [list(range(g * k, g * k + k)) for g in range(n // k)]
    poly = ofx.Polyvoice(e, groups)
    playing = [0] * n                                   # the reference rule, for the oracle side

    def on(g, note):
        poly.note_on(g, note)
        for v in groups[g]:
            if not playing[v]:
                ref.note(v, True, note)
                playing[v] = note
                return

    def off(g, note):
        poly.note_off(g, note)
        for v in groups[g]:
            if playing[v] == note:
                ref.note(v, False, note)
                playing[v] = 0
                return

    for g in range(len(groups)):
        for note in (48, 55, 60, 67):                   # the fourth finds no free voice
            on(g, note + g)
    ys, bs, yrs = [], [], []
    for blk in range(6):
        if blk == 2:
            for g in range(len(groups)):
                off(g, 55 + g)
        if blk == 3:
            for g in range(len(groups)):
                on(g, 72 + g)                           # takes the voice freed at block 2
        vo = torch.empty((1, 256, n), device=cuda)
        bus = poly.process(vo)
        torch.cuda.synchronize()
        ys.append(vo.cpu().numpy())
        bs.append(bus.cpu().numpy())
        yrs.append(ref.process(256))
    y, yr, bus = np.concatenate(ys, 1), np.concatenate(yrs, 1), np.concatenate(bs, 0)
    assert poly.playing.tolist() == playing
    assert np.all(np.isfinite(y))
    assert rel_err(y[0].T, yr[0].T) <= VOICE_TOL
    assert bits_equal(bus, O.mix_ref(y, groups))


# ----------------------------------------------------------------------------- sample rates
@pytest.mark.parametrize("sr", [44100.0, 96000.0])
@pytest.mark.parametrize("kind", ["chorus", "pitchshift", "fxrack", "chain"])
def test_effects_at_other_sample_rates(cuda, kind, sr):
    """Every effect kind at 44.1 and 96 kHz (the reference's Init(sample_rate): RNBO's ms -> sample
    conversions and ring sizes, DelayFx's time scale, mono-chorus's cutoff map; the reverb's delays
    are in samples): bit-exact against the oracle built for the same rate, over ragged blocks."""
    n = 70
    rng = np.random.default_rng(int(sr) + len(kind))
    x = fast_noise(n, 3000, seed=int(sr) % 1000 + len(kind))
    e = engine(kind, n, sample_rate=sr)
    if kind in ("chorus", "pitchshift"):
        p = chorus_params(rng, n)
        if kind == "pitchshift":
            p = p[[0, 7]]
        e.set_params(0, p)
        ref = O.Chorus(n, sample_rate=sr, mode=0 if kind == "chorus" else 1)
        for i in range(n):
            for f in range(p.shape[0]):
                ref.set(i, f if kind == "chorus" else ("pitch", "window")[f], float(p[f, i]))
        yr = ref.process(x)
    elif kind == "fxrack":
        p = np.concatenate([fxrack_params(rng, n), (np.arange(n) % 5)[None, :].astype(np.float32)], 0)
        e.set_params(0, p)
        ref = O.FxRack(n, sample_rate=sr)
        for i in range(n):
            for f in range(p.shape[0]):
                ref.set(i, f, float(p[f, i]))
        yr = ref.process(x, threads=8)
    else:
        pc, pp, pd = chorus_params(rng, n), chorus_params(rng, n)[[0, 7]], dt_params(rng, n, 0.0)
        pd[0] = rng.uniform(0, 1, n)
        e.set_params(0, np.concatenate([pc, pp, pd], 0))
        c1, c2, d = O.Chorus(n, sample_rate=sr), O.Chorus(n, sample_rate=sr, mode=1), O.Dattorro(n)
        _chain_oracle_set(c1, c2, d, n, pc, pp, pd)
        yr = d.process(c2.process(c1.process(x)))
    y = run_gpu(e, x, [256, 4, 60, 1024, 300, 1356], cuda)
    assert bits_equal(y, yr), first_mismatch(y, yr)


@pytest.mark.parametrize("sr", [44100.0, 96000.0])
@pytest.mark.parametrize("kind", ["voice", "voice_moog"])
def test_voices_at_other_sample_rates(cuda, rcp_table, kind, sr):
    """SynthVoice::Init(sample_rate) at 44.1 and 96 kHz (oscillator increment, envelope and
    portamento rates, the Svf's / ladder's frequency maps): bit-exact against the oracle's
    kernel-arithmetic mode for the same rate, through a NoteOn and a NoteOff."""
    n = 64
    rng = np.random.default_rng(int(sr) + 7)
    cfg = voice_configs(rng, n)
    notes = [int(v) for v in rng.integers(36, 97, n)]
    e = engine(kind, n, sample_rate=sr)
    ref = O.Voice(n, sample_rate=sr, moog=kind == "voice_moog", kernel_arith=True)
    e.set_params(0, cfg)
    for i in range(n):
        ref.config(i, cfg[:, i])
    e.note_events([(i, 1, notes[i]) for i in range(n)])
    for i in range(n):
        ref.note(i, True, notes[i])
    ya = np.concatenate([_voice_run(e, 256, cuda) for _ in range(6)], 1)
    yra = ref.process(1536)
    e.note_events([(i, 0, notes[i]) for i in range(n)])
    for i in range(n):
        ref.note(i, False, notes[i])
    yb = np.concatenate([_voice_run(e, 256, cuda) for _ in range(6)], 1)
    yrb = ref.process(1536)
    y, yr = np.concatenate([ya, yb], 1), np.concatenate([yra, yrb], 1)
    assert np.any(y != 0)
    assert voice_bits_equal(y, yr), first_mismatch(y, yr)
