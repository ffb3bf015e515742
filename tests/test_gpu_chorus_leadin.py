"""The ring-free chorus kernel's segment start (chorus_stage_rf.h): the lead-in chunk that fills the
psv window's old slots through the fast path, the line carry from it into chunk 0, the direct pass
it falls back to when a phasor wraps inside its 16 positions, and the loads a segment's last chunk no
longer issues.  BIT-EXACT against the CPU oracle, the checker of test_gpu_chorus_ringfree.py.

Shapes: n = 33 (per-lane I/O, ragged second wave), 36 (row I/O, ragged), 64 (row I/O, two full waves);
every run is ring-free throughout.  What a launch shape is meant to reach is checked on the CPU, from
the oracle's own formulas (chorus_support.tap_delay, the pitch phasor in 64-bit integers), ahead of
the GPU run: a shape that stopped reaching it would fail there, not pass emptily.

The pitch phasor advances pitch / sr cycle per frame: at pitch 3 and 48 kHz tap A wraps every 16,000
frames and tap B half a cycle from it, so the first wrap over recorded (non-zero) history is tap B's
at position 8,000.  The wrap shape therefore runs 520 blocks of 16 frames, not 300: with 300 the
only wrap a lead-in meets is the one at position 0, whose history is all zero."""
import math

import numpy as np
import pytest

import oracle as O
from chorus_support import COLUMNS, DEPTH, PHASE, PITCH, RATE, WINDOW, apply, corner_draw, draw, run, tap_delay
from helpers import bits_equal, fast_noise, first_mismatch

pytestmark = pytest.mark.gpu

SR = 48000.0
CHUNK, SEGMENT = 16, 256

ONE_CHUNK = [16] * 40                                 # every launch: one lead-in, one chunk
RAGGED = [4, 8, 12, 16, 20, 32, 48] * 18              # partial and generic first chunks after a lead-in
RING_WRAP = [256] * 9                                 # the ninth starts at ring position 2048 = 0
BELOW_WRAP = [2044, 16, 256]                          # a segment start 4 positions below the ring's wrap
SEGMENTS = [272, 512, 1028]                           # several segments per launch, a 4-frame last chunk
PHASOR_WRAP = [16] * 520                              # column 7's tap B wraps at position 8,000

# seeds of the phasor-wrap shape: the launch whose lead-in spans position 8,000 depends on column 7's
# drawn depth, rate and phase (the lead L); these satisfy wrap_starts() below
WRAP_SEEDS = {33: 1335, 36: 1336, 64: 1369}


def engine(n):
    import ol_dsp_amd as ofx
    return ofx.Engine("chorus", n)


def segment_starts(blocks):
    """(first frame, frames) of every segment a launch is cut into at the latest: launch starts and every
    256 frames inside a launch (a wave may halve a segment; the halves' starts are not counted)."""
    out, f0 = [], 0
    for frames in blocks:
        for s in range(0, frames, SEGMENT):
            out.append((f0 + s, min(SEGMENT, frames - s)))
        f0 += frames
    return out


def delays(p, i, f0, frames):
    return [tap_delay(SR, f, p[DEPTH, i], p[RATE, i], p[PHASE, i]) for f in range(f0, f0 + frames)]


def has_small_lead(p, blocks):
    """A segment start where some instance's delay stays below 14 over the first chunk: whatever the
    segment's length, its lower bound (the lead L) is < 15, so chunk 0's x patch lands in the windows."""
    return any(max(delays(p, i, f0, CHUNK)) < 14.0
               for f0, _ in segment_starts(blocks) for i in range(p.shape[1]))


def has_large_lead(p, blocks):
    """A segment start where some instance's delay stays at 33 or more over the whole segment (and so
    over either half of it): L >= 31, every patched slot past the windows."""
    return any(min(delays(p, i, f0, frames)) >= 33.0
               for f0, frames in segment_starts(blocks) for i in range(p.shape[1]))


def wrap_starts(p, blocks, i=7, history=2048):
    """Segment starts whose 16 lead-in positions w0 - L - 16 .. w0 - L - 1 span a wrap of instance i's
    pitch phasor (tap A's, or tap B's half a cycle on), for L one either side of the double-precision
    lower bound as well, and lie past `history` (the ring has wrapped: the positions hold signal)."""
    inc = int(math.floor(float(p[PITCH, i]) / SR * 2.0 ** 64 + 0.5))
    m = 1 << 64
    out = []
    for w0, frames in segment_starts(blocks):
        lead = int(math.floor(max(min(delays(p, i, w0, frames)) - 0.01, 0.0)))

        def wraps(L):
            a0 = ((w0 - L - CHUNK) * inc) % m
            b0 = (a0 + (m >> 1)) % m
            return (a0 + (CHUNK - 1) * inc) % m < a0 or (b0 + (CHUNK - 1) * inc) % m < b0
        if all(wraps(L) for L in (lead - 1, lead, lead + 1)) and w0 - lead - CHUNK - 1 >= history:
            out.append(w0)
    return out


def check(cuda, n, p, blocks, seed):
    x = fast_noise(n, sum(blocks), seed=seed)
    e, ref = engine(n), O.Chorus(n)
    apply(e, ref, p)
    y, yr, modes = run(e, ref, x, blocks, cuda)
    assert modes == [1] * len(blocks)
    assert bits_equal(y, yr), first_mismatch(y, yr)


@pytest.mark.parametrize("n", [33, 36, 64])
@pytest.mark.parametrize("name,blocks,both_leads", [
    ("one_chunk", ONE_CHUNK, True),
    ("ragged", RAGGED, True),
    ("ring_wrap", RING_WRAP, False),
    ("below_wrap", BELOW_WRAP, False),
    ("segments", SEGMENTS, True),
])
def test_leadin_launch_shapes(cuda, n, name, blocks, both_leads):
    """Launches of one chunk, ragged launches, segment starts at and just below the x ring's wrap, and
    launches of several segments, over the drawn parameters with chorus_support.COLUMNS' corners."""
    p = draw(n, 1200 + n)
    assert all(f in (DEPTH, RATE, PHASE, PITCH, WINDOW) for col in COLUMNS.values() for f in col)
    if both_leads:
        assert has_small_lead(p, blocks) and has_large_lead(p, blocks)
    if name == "ring_wrap":
        assert sum(blocks[:8]) % 2048 == 0
    if name == "below_wrap":
        assert blocks[0] % 2048 == 2044
    check(cuda, n, p, blocks, 500 + n)


@pytest.mark.parametrize("blocks", [RAGGED, SEGMENTS], ids=["ragged", "segments"])
def test_leadin_corner_parameters(cuda, blocks):
    """The line-carry stress draw (pitch 0 and 0.01, the three windows, the three depths and rates)."""
    check(cuda, 36, corner_draw(36, 1250), blocks, 560)


@pytest.mark.parametrize("n", [33, 36, 64])
def test_leadin_phasor_wrap_falls_back(cuda, n):
    """16-frame launches across column 7's (pitch 3, window 4 ms) tap-B wrap at position 8,000: one
    launch's lead-in spans it and the wave takes the direct pass for its old slots; the launches
    around it take the lead-in."""
    p = draw(n, WRAP_SEEDS[n])
    assert has_small_lead(p, PHASOR_WRAP) and has_large_lead(p, PHASOR_WRAP)
    hits = wrap_starts(p, PHASOR_WRAP)
    assert hits, "no lead-in of this draw spans a phasor wrap over recorded history"
    check(cuda, n, p, PHASOR_WRAP, 600 + n)
