"""Shared test helpers: seeded inputs, parameter draws, bit comparisons."""
from __future__ import annotations

import numpy as np

import oracle as O


def noise_block(n: int, frames: int, base: int = 0, ch: int = 2) -> np.ndarray:
    """[ch][frames][n] xorshift32 white noise, seeded per (instance, channel)."""
    x = np.empty((ch, frames, n), dtype=np.float32)
    for i in range(n):
        for c in range(ch):
            x[c, :, i] = O.xorshift_noise(O.instance_seed(base + i, c), frames)
    return x


def fast_noise(n: int, frames: int, seed: int = 0, ch: int = 2) -> np.ndarray:
    rng = np.random.default_rng(seed)
    return (rng.random((ch, frames, n), dtype=np.float32) - 0.5).astype(np.float32)


def bits_equal(a: np.ndarray, b: np.ndarray) -> bool:
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def first_mismatch(a: np.ndarray, b: np.ndarray):
    d = np.argwhere(a.view(np.uint32) != b.view(np.uint32))
    return None if len(d) == 0 else (tuple(d[0]), float(a[tuple(d[0])]), float(b[tuple(d[0])]), len(d))


def same_bits_or_nan(a: np.ndarray, b: np.ndarray) -> bool:
    """The same NaN mask, and the same uint32 bits everywhere else: +-Inf, +-0 and subnormals are
    compared exactly.  The sign and payload of a NaN are not compared (x86 and the GPU generate
    different default NaNs): the one relaxation against bits_equal."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    if not np.array_equal(na, nb):
        return False
    return np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def first_mismatch_or_nan(a: np.ndarray, b: np.ndarray):
    """first_mismatch under same_bits_or_nan's rule."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    d = np.argwhere((na != nb) | (~na & ~nb & (a.view(np.uint32) != b.view(np.uint32))))
    return None if len(d) == 0 else (tuple(d[0]), float(a[tuple(d[0])]), float(b[tuple(d[0])]), len(d))


def subnormal_share(y: np.ndarray) -> float:
    """The share of y's non-zero samples that are subnormal (0 if all are zero)."""
    a = np.abs(y)
    sub = (a > 0) & (a < np.finfo(np.float32).tiny)
    return float(np.count_nonzero(sub) / max(1, np.count_nonzero(y != 0)))


def nonfinite_share(y: np.ndarray) -> float:
    return float(np.mean(~np.isfinite(y)))


# ---- signals at the edge of fp32 (tests/test_gpu_edges.py, tests/test_oracle.py) ----
EDGE_FRAMES = 3072
EDGE_BLOCKS = [256, 4, 20, 1024, 300, 1468]


def poison_table(n: int) -> list:
    """(channel, frame, instance, value): single non-finite input samples in the first and the last
    instance and on both sides of a 64-lane wave edge."""
    t = [(0, 100, 0, np.nan), (1, 7, 5, np.inf), (0, 256, 63, -np.inf), (1, 1000, 64, np.nan),
         (0, 3, n - 1, np.inf), (1, 3, n - 1, -np.inf)]
    assert all(i < n for _, _, i, _ in t)
    return t


def poisoned(x: np.ndarray) -> np.ndarray:
    y = x.copy()
    for c, f, i, v in poison_table(x.shape[2]):
        y[c, f, i] = v
    return y


def edge_signals(x: np.ndarray) -> dict:
    """name -> signal [2][frames][n] built on the noise x: subnormal and loud scalings (exact: powers
    of two), a burst that decays into exact zeros, signed zero and constants.  All finite."""
    f = np.float32
    burst = x.copy()
    burst[:, 300:] = 0.0
    alt = np.ones_like(x)
    alt[:, 1::2] = -1.0
    return {"subnormal": x * f(2.0 ** -130), "burst": burst, "loud100": x * f(2.0 ** 100),
            "loud127": x * f(2.0 ** 127), "negzero": np.full_like(x, -0.0), "ones": np.ones_like(x),
            "alternating": alt}


def dt_edge_params(n: int, seed: int = 40) -> np.ndarray:
    """The reverb's parameters of the edge-signal runs: dt_params with pre-delays in [0, 0.02)."""
    rng = np.random.default_rng(seed)
    p = dt_params(rng, n, 0.0)
    p[0] = rng.uniform(0, 0.02, n)
    return p


def dt_corner_params() -> np.ndarray:
    """[7][128]: the corners {0, 1}^7 of the reverb's seven setters (pre-delay 0 and 4800 samples,
    decay at both clamps, gains exactly 0 and 1); bit f of the instance index is field f."""
    i = np.arange(128)
    return np.stack([((i >> f) & 1).astype(np.float32) for f in range(7)])


def rel_err(a: np.ndarray, ref: np.ndarray) -> float:
    """max |a - ref| / max(|ref|, rms(ref)) per instance (SURVEY 8c acceptance floor)."""
    a = a.astype(np.float64)
    ref = ref.astype(np.float64)
    rms = np.sqrt(np.mean(ref ** 2, axis=1, keepdims=True)) + 1e-30
    return float(np.max(np.abs(a - ref) / np.maximum(np.abs(ref), rms)))


def dt_params(rng: np.random.Generator, n: int, pre_delay: float) -> np.ndarray:
    p = np.empty((7, n), dtype=np.float32)
    p[0] = pre_delay
    p[1] = rng.uniform(0.5, 0.95, n)
    p[2] = rng.uniform(0.4, 0.8, n)
    p[3] = rng.uniform(0.4, 0.8, n)
    p[4] = rng.uniform(0.3, 0.8, n)
    p[5] = rng.uniform(0.25, 0.95, n)
    p[6] = rng.uniform(0.05, 0.95, n)
    return p


def dt_reference_cases() -> dict:
    """The runs in which the restated reverb is compared with the reference build itself
    (tests/test_oracle.py; recorded by tests/golden/gen_golden.py into
    tests/golden/dattorro_reference_runs.json): name -> (params [7][n], input [2][frames][n])."""
    rng = np.random.default_rng(5)
    n, frames = 16, 70000            # crosses t = 32768 (modulation turn) and the uint16 wrap
    p = np.empty((7, n), np.float32)
    p[0] = rng.uniform(0, 1, n)      # per-instance pre-delay is fine on the CPU
    p[1:] = rng.uniform(0.05, 0.95, (6, n))
    x = (rng.random((2, frames, n), dtype=np.float32) - 0.5)
    # extremes of the setters: zero pre-delay, decay clamp both ends, zero/unit gains
    edge = [[0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0],
            [1.0, 0.0, 1.0, 1.0, 1.0, 1.0, 1.0],
            [0.5, 0.5, 0.5, 0.5, 0.5, 0.1, 0.5],
            [0.99, 0.9, 0.9, 0.9, 0.9, 0.99, 0.01]]
    runs = {"random_params": (p, x),
            "edge_params": (np.asarray(edge, np.float32).T.copy(), noise_block(len(edge), 5000, 99)),
            "default_params": (None, noise_block(2, 3000, 3))}
    # signals at the edge of fp32 on which the reverb stays finite (edge_signals), 8 instances, and
    # the 128 corners of the seven setters over the input of the GPU corner run
    sig = edge_signals(fast_noise(8, EDGE_FRAMES, seed=40))
    for name in ("subnormal", "loud100", "loud127", "burst", "negzero"):
        runs["edge_signal_" + name] = (dt_edge_params(8), sig[name])
    runs["corner_params"] = (dt_corner_params(), fast_noise(128, 4096, seed=4))
    # one pre-delay for all instances (the engine's position-major pre-delay tap, dattorro_block_v4):
    # the delays it serves from registers (0..8), the first from the ring (9), past a 256-frame call
    # and the setter's maximum; and 70,000 frames at the longest delay the 8,192-slot ring holds
    for d in UNIFORM_PD:
        runs[f"uniform_pd_{d}"] = _uniform_pd_run(d, 4, 2048)
    runs["uniform_long"] = _uniform_pd_run(8191, 8, 70000)
    return runs


UNIFORM_PD = (0, 1, 3, 4, 5, 8, 9, 257, 4800)
UNIFORM_PD_RUNS = [f"uniform_pd_{d}" for d in UNIFORM_PD] + ["uniform_long"]


def predelay_value(d) -> np.ndarray:
    """The float32 setter value(s) of a pre-delay of d samples, built as test_dattorro_predelay_beyond_max
    builds them (d / 4800 rounded to float32); checked to give d back through uint16(value * 4800.f)."""
    v = (np.asarray(d, np.float64) / 4800).astype(np.float32)
    assert np.array_equal((v * np.float32(4800.0)).astype(np.uint16), np.asarray(d)), d
    return v


def _uniform_pd_run(d: int, n: int, frames: int):
    """Parameters and input drawn as random_params draws them, with their own seed and every
    instance's pre-delay d samples."""
    rng = np.random.default_rng([5, d, frames])
    p = np.empty((7, n), np.float32)
    p[0] = predelay_value(d)
    p[1:] = rng.uniform(0.05, 0.95, (6, n))
    return p, (rng.random((2, frames, n), dtype=np.float32) - 0.5)


def run_dattorro(bank, params, x: np.ndarray, threads: int = 1) -> np.ndarray:
    """Set params [7][n] (None = the defaults) on an oracle reverb bank and process x."""
    if params is not None:
        for i in range(params.shape[1]):
            for f in range(7):
                bank.set(i, f, float(params[f, i]))
    return bank.process(x, threads)


def lr_hashes(y: np.ndarray) -> list:
    return [f"{O.fnv1a64_lr(y[0, :, i], y[1, :, i]):016x}" for i in range(y.shape[2])]


def chorus_params(rng: np.random.Generator, n: int) -> np.ndarray:
    p = np.empty((8, n), dtype=np.float32)
    p[0] = rng.uniform(0, 3, n)
    p[1] = rng.uniform(0, 1, n)
    p[2] = rng.uniform(0, 0.95, n)
    p[3] = rng.uniform(0, 1, n)
    p[4] = rng.uniform(0, 1, n)
    p[5] = rng.uniform(0.08, 1, n)
    p[6] = rng.uniform(0.01, 1, n)
    p[7] = rng.uniform(4, 10, n)
    return p


def voice_configs(rng: np.random.Generator, n: int) -> np.ndarray:
    p = np.empty((16, n), dtype=np.float32)
    p[0] = rng.uniform(100, 8000, n)
    p[1] = rng.uniform(0, 0.9, n)
    p[2] = rng.uniform(0, 1, n)
    p[3] = rng.uniform(0, 1, n)
    p[4] = rng.uniform(0.001, 0.5, n)
    p[5] = rng.uniform(0, 1, n)
    p[6] = rng.uniform(0.001, 0.5, n)
    p[7] = rng.uniform(0, 1, n)
    p[8] = rng.uniform(0.001, 0.5, n)
    p[9] = rng.uniform(0.2, 1, n)
    p[10] = rng.uniform(0.001, 0.5, n)
    p[11] = rng.uniform(0, 1, n)
    p[12] = rng.uniform(0.001, 0.5, n)
    p[13] = rng.uniform(0, 1, n)
    p[14] = rng.uniform(0.001, 0.5, n)
    p[15] = rng.uniform(0, 0.05, n)
    return p

def fxrack_params(rng: np.random.Generator, n: int) -> np.ndarray:
    """FxRack<2> member values (FR_FIELDS order), seeded; every 4th instance gets a delay shorter
    than a 16-frame chunk (time * 48000 in [0, 17)), the path that reads its own chunk's writes."""
    p = np.empty((11, n), dtype=np.float32)
    p[0] = rng.uniform(0, 1, n)
    p[0, ::4] = rng.uniform(0, 17, len(p[0, ::4])) / 48000
    p[1] = rng.uniform(0, 0.9, n)
    p[2] = rng.uniform(0, 1, n)
    p[3] = rng.uniform(100, 12000, n)
    p[4] = rng.uniform(0, 0.8, n)
    p[5] = rng.uniform(0, 1, n)
    p[6] = rng.uniform(100, 12000, n)
    p[7] = rng.uniform(0, 0.8, n)
    p[8] = rng.uniform(0, 1, n)
    p[9] = rng.integers(0, 5, n).astype(np.float32)
    p[10] = rng.uniform(0, 1, n)
    return p
