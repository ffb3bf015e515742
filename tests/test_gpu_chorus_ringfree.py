"""The ring-free chorus kernel (chorus_block_rf1, ol_dsp_amd/csrc/chorus_stage_rf.h) and the switch to
and from the ring kernel (chorus_block_v11 after a chorus-ring materialise): BIT-EXACT against the
CPU oracle's chorus bank, the checker of test_gpu_parity.py.

Shapes: n = 33 (per-lane I/O, ragged second wave), 36 (row I/O, ragged), 64 (row I/O, two full waves).
Every case runs at least 2,304 frames: more than the 1,154-frame chorus history plus the 480-frame
pitch window, so every psv the tap reads has been recomputed from wrapped ring data.  The drawn
parameters carry fixed columns (chorus_support.COLUMNS) that reach the kernel's edges."""
import numpy as np
import pytest

import oracle as O
from chorus_support import DEPTH, HISTORY, PITCH, WINDOW, apply, draw, run
from helpers import bits_equal, fast_noise, first_mismatch

pytestmark = pytest.mark.gpu


def engine(n):
    import ol_dsp_amd as ofx
    return ofx.Engine("chorus", n)


@pytest.mark.parametrize("n", [33, 36, 64])
def test_ringfree_blocks_of_256(cuda, n):
    """Steady state in 256-frame blocks: ring-free from frame 0 (the pitch is set before the first
    block: all history is zero) to the end."""
    blocks = [256] * 10
    p = draw(n, 700 + n)
    x = fast_noise(n, sum(blocks), seed=n)
    e, ref = engine(n), O.Chorus(n)
    apply(e, ref, p)
    assert e.kernel_name == "chorus_block_v11"          # the kind's ring kernel; the mode has its own accessor
    y, yr, modes = run(e, ref, x, blocks, cuda)
    assert modes == [1] * len(blocks)
    assert bits_equal(y, yr), first_mismatch(y, yr)


@pytest.mark.parametrize("n", [33, 36, 64])
def test_ringfree_mixed_block_sizes(cuda, n):
    """Calls of 4, 20 and 256 frames (partial chunks, launches shorter than a chunk, each launch's
    fresh psv window) and one of 1,000 (several segments in one launch)."""
    blocks = [4, 20, 256] * 6 + [1000, 4, 20, 256, 4]
    assert sum(blocks) >= 2304
    p = draw(n, 800 + n)
    x = fast_noise(n, sum(blocks), seed=100 + n)
    e, ref = engine(n), O.Chorus(n)
    apply(e, ref, p)
    y, yr, modes = run(e, ref, x, blocks, cuda)
    assert modes == [1] * len(blocks)
    assert bits_equal(y, yr), first_mismatch(y, yr)


@pytest.mark.parametrize("n", [33, 36, 64])
def test_depth_and_pitch_changes_mid_run(cuda, n):
    """A depth change (no switch), a pitch change (materialise, the ring kernel for the 1,154-frame
    history, then ring-free again) and a pitch set to its current value (no switch): bit-exact through
    each event and for at least 1,280 frames after it."""
    blocks = [256] * 21
    p = draw(n, 900 + n)
    x = fast_noise(n, sum(blocks), seed=200 + n)
    e, ref = engine(n), O.Chorus(n)
    apply(e, ref, p)
    events = {
        3: [(9, DEPTH, 0.93), (1, DEPTH, 0.5)],
        9: [(7, PITCH, 1.25)],
        15: [(7, PITCH, 1.25), (2, PITCH, 0.0)],
    }
    y, yr, modes = run(e, ref, x, blocks, cuda, events)
    ring = -(-HISTORY // 256)                            # blocks of ring mode: 5
    assert modes == [1] * 9 + [0] * ring + [1] * (21 - 9 - ring)
    assert bits_equal(y, yr), first_mismatch(y, yr)


@pytest.mark.parametrize("n", [33, 36])
def test_pitch_changes_on_consecutive_blocks(cuda, n):
    """Pitch and window changes ahead of two consecutive blocks: the second finds the ring current and
    restarts the count; mixed call sizes through the ring-mode stretch."""
    blocks = [256] * 4 + [256, 20, 4, 256, 256, 256, 256, 236] + [256] * 6
    p = draw(n, 1000 + n)
    x = fast_noise(n, sum(blocks), seed=300 + n)
    e, ref = engine(n), O.Chorus(n)
    apply(e, ref, p)
    events = {4: [(0, PITCH, 2.0), (n - 1, PITCH, 0.5)], 5: [(n - 1, WINDOW, 5.5), (3, PITCH, 2.9)]}
    y, yr, modes = run(e, ref, x, blocks, cuda, events)
    # the count restarts at block 5: 20 + 4 + 256 * 4 + 236 = 1,284 >= 1,154 only after block 11
    since = np.cumsum([0] + blocks[5:])
    expect = [1] * 4 + [0] + [1 if s >= HISTORY else 0 for s in since[:len(blocks) - 5]]
    assert modes == expect
    assert modes[12:] == [1] * 6 and modes[4:11] == [0] * 7
    assert bits_equal(y, yr), first_mismatch(y, yr)


def test_reset_returns_to_ring_free(cuda):
    """olfx_reset in the middle of a ring-mode stretch: ring-free from the first frame after it, with
    the pitch set before that frame, against a fresh oracle."""
    n = 36
    p = draw(n, 1100)
    x = fast_noise(n, 256 * 4, seed=400)
    e, ref = engine(n), O.Chorus(n)
    apply(e, ref, p)
    y, yr, modes = run(e, ref, x, [256] * 4, cuda, {2: [(5, PITCH, 2.2)]})
    assert modes == [1, 1, 0, 0] and e.chorus_ring_free == 0
    assert bits_equal(y, yr), first_mismatch(y, yr)
    e.reset()
    assert e.chorus_ring_free == 1 and e.frames_processed == 0
    blocks = [256] * 9
    p2 = draw(n, 1101)
    x2 = fast_noise(n, sum(blocks), seed=401)
    ref2 = O.Chorus(n)
    apply(e, ref2, p2)
    y, yr, modes = run(e, ref2, x2, blocks, cuda)
    assert modes == [1] * len(blocks)
    assert bits_equal(y, yr), first_mismatch(y, yr)
