"""The level meters' test cases, stated once for tests/test_meter_ref.py (the reference alone, CPU) and
tests/test_gpu_meter.py (the kernel against the reference): the call schedule, the parameter mixes and the edge
signals, each with the condition it is there for, asserted on tests/meter_ref.py."""
from __future__ import annotations

import functools

import numpy as np

import meter_ref as M
from ol_dsp_amd.workload import noise_np

# 3,072 frames: chunk tails of 4 (4, 20) and 12 (300, 1468), a one-chunk call (4), whole chunks (256, 1024)
CALLS = [256, 4, 20, 1024, 300, 1468]
FRAMES = sum(CALLS)
STARTS = np.concatenate([[0], np.cumsum(CALLS)]).tolist()
assert FRAMES == 3072 and {c % 16 for c in CALLS} == {0, 4, 12}

W44 = np.float32(44100) / np.float32(375)             # 117.6: no count ever equals it
WINDOWS = np.array([1, 2, 3, 16, 128, 300, W44, 0], np.float32)      # 0: the rate's default
HOLDS = np.array([5, 16, 256, 1000, 96000], np.float32)


@functools.lru_cache(maxsize=None)
def _noise(n: int, ch: int, frames: int, first: int) -> np.ndarray:
    x = noise_np(first, n, frames, ch)
    x.setflags(write=False)
    return x


def noise(n: int, ch: int = 2, frames: int = FRAMES, first: int = 0) -> np.ndarray:
    """[ch][frames][n] seeded uniform noise in [-0.5, 0.5) (computed once per shape, read-only)."""
    return _noise(n, ch, frames, first)


def mixed_windows(n: int) -> np.ndarray:
    return WINDOWS[np.arange(n) % len(WINDOWS)]


def mixed_holds(n: int) -> np.ndarray:
    return HOLDS[(np.arange(n) // 3) % len(HOLDS)]


def reference(n, ch, x, calls=CALLS, modes=(True,), window=None, hold=None, changes=None, sample_rate=48000.0):
    """The envelope and the levels after every call: (env [ch][frames][n], [levels after call k])."""
    ref = M.MeterRef(n, ch, sample_rate)
    if window is not None:
        ref.set("window", np.broadcast_to(np.asarray(window, np.float32), (n,)))       # a scalar: every instance
    if hold is not None:
        ref.set("peak_hold", np.broadcast_to(np.asarray(hold, np.float32), (n,)))
    env = np.zeros(x.shape, np.float32)
    levels, f0 = [], 0
    for k, m in enumerate(calls):
        for field, values, first in (changes or {}).get(k, ()):
            ref.set(field, values, first)
        e = ref.process(x[:, f0:f0 + m], envelope=bool(modes[k % len(modes)]))
        if e is not None:
            env[:, f0:f0 + m] = e
        levels.append(ref.levels())
        f0 += m
    return env, levels


# ---- window changes between calls ----
def window_changes(n: int):
    """Ahead of call 2 (frame 260) the window-16 instances go to 128: a larger window.  Ahead of call 4 (frame 1304)
    the window-300 instances go to 100, below their running count (1304 % 300 = 104): no reset ever again."""
    w = mixed_windows(n)
    up = np.flatnonzero(w == 16)
    down = np.flatnonzero(w == 300)
    changes = {2: [("window", np.float32(128), int(i)) for i in up], 4: [("window", np.float32(100), int(i)) for i in down]}
    return w, changes, up, down


def check_window_changes(levels, up, down) -> None:
    """On the reference: after the change below the count, the count only grows."""
    if len(down):
        assert np.all(levels[3]["count"][down] == 104)
        assert np.all(levels[4]["count"][down] == 104 + 300) and np.all(levels[5]["count"][down] == 104 + 300 + 1468)
    if len(up):
        # 260 % 16 = 4 frames counted at the change, then a reset whenever the count stands at 128
        assert np.all(levels[5]["count"][up] == (4 + FRAMES - 260 - 1) % 128 + 1)


# ---- peak hold: where the expiries fall ----
def expiry_frames(hold: float, frames: int = FRAMES) -> list:
    """The frames after which the reference's peak_count is back at 0, found by running it a frame at a time."""
    ref = M.MeterRef(1, 1)
    ref.set("peak_hold", hold)
    x = np.ones((1, 1, 1), np.float32)
    out = []
    for f in range(frames):
        ref.process(x, envelope=False)
        if ref.state["peak_count"][0, 0] == 0:
            out.append(f)
    return out


def check_hold_expiries() -> None:
    """Over CALLS, the mixed holds expire inside a chunk, on a chunk's last frame and on a call's last frame."""
    where = set()
    for h in (5.0, 16.0, 256.0, 1000.0):
        for f in expiry_frames(h):
            k = max(c for c in range(len(CALLS)) if STARTS[c] <= f)
            off = f - STARTS[k]
            where.add("call_last" if off == CALLS[k] - 1 else "chunk_last" if off % 16 == 15 else "inside")
    assert where == {"call_last", "chunk_last", "inside"}, where
    assert expiry_frames(96000.0) == []


# ---- edge signals (window 128 everywhere), each with its condition on the reference ----
POISONED = lambda n: sorted({0, 5, 63, 64, n - 1})     # noqa: E731
EDGES = ["scale_2^-70", "scale_2^-75", "scale_2^100", "one_nan", "inf", "all_-0", "all_+1", "alternating_+-1"]


def edge(name: str, n: int, ch: int = 2):
    """(x, hold or None): the case's input and hold, its condition asserted on the reference."""
    base = noise(n, ch)
    hold = None
    if name.startswith("scale_"):
        x = base * np.float32(2.0 ** int(name.split("^")[1]))
    elif name == "one_nan":
        x = base.copy()
        x[0, 300, POISONED(n)] = np.nan
    elif name == "inf":
        x = base.copy()
        p = POISONED(n)
        x[0, 300, p[0::2]] = np.inf
        x[0, 300, p[1::2]] = -np.inf
        hold = np.float32(2000)                          # expires at frame 1999, in the last call
    elif name == "all_-0":
        x = np.full(base.shape, -0.0, np.float32)
    elif name == "all_+1":
        x = np.ones(base.shape, np.float32)
    elif name == "alternating_+-1":
        x = np.ones(base.shape, np.float32)
        x[:, 1::2] = -1
    else:
        raise KeyError(name)
    x = np.ascontiguousarray(x, np.float32)

    # the condition, on the reference alone (frame by frame where the sum is looked at)
    w = np.float32(128)
    env, levels = reference(n, ch, x, window=w, hold=hold)
    total = FRAMES * n * ch
    with np.errstate(all="ignore"):
        if name == "scale_2^-70":
            sums = _sums(n, ch, x, w)
            tiny = np.finfo(np.float32).tiny
            assert np.count_nonzero((sums > 0) & (sums < tiny)) >= 0.99 * total
            assert np.count_nonzero(env != 0) >= 0.99 * total
        elif name == "scale_2^-75":
            assert np.all(env == 0) and np.all(levels[-1]["peak"] > 0)
        elif name == "scale_2^100":
            assert np.all(np.isposinf(env)) and np.all(np.isfinite(levels[-1]["peak"]))
        elif name in ("one_nan", "inf"):
            p = POISONED(n)
            bad = ~np.isfinite(env[0][:, p])
            assert np.all(bad[300:384]) and not np.any(bad[:300]) and not np.any(bad[384:])
            others = np.setdiff1d(np.arange(n), p)
            assert np.all(np.isfinite(env[0][:, others])) and np.all(np.isfinite(env[1:]))
            for lv in levels:
                assert not np.any(np.isnan(lv["peak"]))
            if name == "inf":
                assert np.all(np.isposinf(levels[3]["peak"][p, 0])) and np.all(np.isposinf(levels[4]["peak"][p, 0]))
                assert np.all(np.isfinite(levels[5]["peak"]))
        elif name == "all_-0":
            assert np.all(env == 0) and not np.any(np.signbit(env)) and np.all(levels[-1]["peak"] == 0)
        else:
            assert np.all(env == 1) and np.all(levels[-1]["peak"] == 1)
    return x, hold


def _sums(n, ch, x, window):
    ref = M.MeterRef(n, ch)
    ref.set("window", np.full(n, window, np.float32))
    out = np.empty(x.shape, np.float32)
    for f in range(x.shape[1]):
        ref.process(x[:, f:f + 1], envelope=False)
        out[:, f] = ref.state["sum"]
    return out
