"""The level meters' reference: ol::core::Rms (modules/corelib/ol_corelib.h:61-85) and the sandbox firmware's
peak-hold follower (modules/ol_daisy/workouts/sandbox/main.cpp:98-137), restated in numpy fp32.

Per signal (one channel of one instance) and frame, in this order (include/olfx.h):

    if count == window: sum = 0; count = 0            before the add
    sum = sum + x * x;  count = count + 1.0f
    rms = sqrtf(sum / count)                          what Rms::Process returns
    peak = fabsf(x) if peak < fabsf(x) else peak
    peak_count = peak_count + 1.0f
    if peak_count == hold: peak_count = 0; peak = 0

Every value is a float32 and every operation one IEEE single-precision operation (numpy's float32 multiply, add,
divide and square root are correctly rounded and never contracted), vectorised over the signals with one loop
over frames.  tests/test_meter_ref.py holds this file to fixtures recorded from the reference's own class.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np

FIELDS = ("rms", "peak", "sum", "count", "peak_count")
DEFAULT_HOLD = np.float32(96000.0)       # 2 * 48000, a literal in the firmware


def default_window(sample_rate: float) -> np.float32:
    """Rms::Init(sample_rate, 0): sample_rate / 375 in t_sample."""
    return np.float32(sample_rate) / np.float32(375)


class MeterRef:
    """n instances x `channels` independent signals; window and peak_hold per instance."""

    def __init__(self, n: int, channels: int = 2, sample_rate: float = 48000.0):
        self.n, self.channels, self.sample_rate = int(n), int(channels), float(sample_rate)
        self.window = np.zeros(self.n, np.float32)            # the parameter: 0 = the rate's default
        self.hold = np.full(self.n, DEFAULT_HOLD, np.float32)
        self.reset()

    def reset(self) -> None:
        """Fresh state; the parameters stay, as olfx_reset leaves a meter's."""
        self.state = {f: np.zeros((self.channels, self.n), np.float32) for f in FIELDS}

    def set(self, field: str, values, first: int = 0) -> None:
        v = np.atleast_1d(np.asarray(values, np.float32))
        assert np.all(np.isfinite(v))
        {"window": self.window, "peak_hold": self.hold}[field][first:first + len(v)] = v

    def resolved_window(self) -> np.ndarray:
        return np.where(self.window != 0, self.window, default_window(self.sample_rate)).astype(np.float32)

    def process(self, x: np.ndarray, envelope: bool = True) -> Optional[np.ndarray]:
        """x [channels][frames][n].  Envelope mode returns the rms after every frame; summary mode returns
        None and leaves the last frame's rms in the state -- the same state either way."""
        x = np.asarray(x, np.float32)
        assert x.shape[0] == self.channels and x.shape[2] == self.n, x.shape
        frames = x.shape[1]
        window = self.resolved_window()[None, :]
        hold = self.hold[None, :]
        s = self.state
        total, count, rms, peak, pc = s["sum"], s["count"], s["rms"], s["peak"], s["peak_count"]
        env = np.empty_like(x) if envelope else None
        one, zero = np.float32(1), np.float32(0)
        with np.errstate(all="ignore"):
            for f in range(frames):
                xf = x[:, f, :]
                hit = count == window
                total = np.where(hit, zero, total)
                count = np.where(hit, zero, count)
                total = total + xf * xf
                count = count + one
                if envelope:
                    rms = np.sqrt(total / count)
                    env[:, f, :] = rms
                ax = np.abs(xf)
                peak = np.where(peak < ax, ax, peak)
                pc = pc + one
                over = pc == hold
                pc = np.where(over, zero, pc)
                peak = np.where(over, zero, peak)
            if not envelope and frames:
                rms = np.sqrt(total / count)
        self.state = {"sum": total.astype(np.float32), "count": count.astype(np.float32), "rms": rms.astype(np.float32),
                      "peak": peak.astype(np.float32), "peak_count": pc.astype(np.float32)}
        return env

    def levels(self) -> Dict[str, np.ndarray]:
        """As Engine.levels(): [n][channels] per field."""
        return {f: np.ascontiguousarray(self.state[f].T) for f in FIELDS}


def run_schedule(ref: MeterRef, x: np.ndarray, calls: Sequence[int], modes: Sequence[bool],
                 changes: Optional[Dict[int, Sequence]] = None) -> np.ndarray:
    """x cut into consecutive calls of `calls` frames; call k runs in envelope mode if modes[k % len(modes)], and
    changes[k] = [(field, values, first), ...] is set ahead of it.  Returns the envelope [channels][frames][n] with
    NaN-free zeros where a summary call wrote nothing."""
    assert sum(calls) == x.shape[1]
    out = np.zeros_like(x, dtype=np.float32)
    f0 = 0
    for k, m in enumerate(calls):
        for field, values, first in (changes or {}).get(k, ()):
            ref.set(field, values, first)
        env = ref.process(x[:, f0:f0 + m], envelope=bool(modes[k % len(modes)]))
        if env is not None:
            out[:, f0:f0 + m] = env
        f0 += m
    return out


def fnv1a64(a: np.ndarray) -> int:
    """FNV-1a over the little-endian bytes of a float32 array (the recorder's hash of a long run)."""
    h = 0xCBF29CE484222325
    for b in np.ascontiguousarray(a, np.float32).view(np.uint8).ravel().tolist():
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h
