"""The chorus kind's two kernels at the places test_gpu_chorus_ringfree.py leaves out: the ring kernel
(chorus_block_v11<FULL>) held for long runs, the switch (chorus_materialise, then the ring kernel for one
chorus history) across workgroups, at 44.1 and 96 kHz, at the edges of the frame count, through a stream
switch, host I/O and signals at the edge of fp32.  BIT-EXACT against oracle.Chorus built for the same
sample rate.

Every expected mode list comes from chorus_support.expected_modes(blocks, changes, H(sr)), never from
the engine, and is also written out where it is short.  Two devices carry most cases:
  the keeper  -- the last instance's window flipped 5.5 <-> 5.6 ms ahead of every block from block 1 on
      restarts the count each time, so every block after the first (4 frames: a change before the first
      frame does not count) runs the ring kernel whatever its length;
  a witness   -- depth 1, phase 0, rate 0.01, mix 1: its tap sits at the largest delay, so its output
      depends on every position a materialise fills.  Each test asserts, in double from the oracle's
      own formula, that the witness's delay at the change frame is at least H - 4."""
import math

import numpy as np
import pytest

import oracle as O
from chorus_support import (CUTOFF, DEPTH, MIX, PHASE, PITCH, Q, RATE, WINDOW, apply, apply_oracle,
                            corner_draw, draw, expected_modes, history, keeper_events, run, run_oracle,
                            set_witnesses, tap_delay, witness_delay)
from helpers import (bits_equal, chorus_params, edge_signals, fast_noise, first_mismatch,
                     first_mismatch_or_nan, nonfinite_share, same_bits_or_nan, subnormal_share)

pytestmark = pytest.mark.gpu

SR = 48000.0
H48 = history(SR)
X_RING = {44100.0: 2048, 96000.0: 4096}       # positions of the ring-free kernel's input ring


def engine(n, sr=SR):
    import ol_dsp_amd as ofx
    return ofx.Engine("chorus", n, sample_rate=sr)


def new_pitch(p, i):
    """A pitch for instance i that differs from its current one by at least 0.3 Hz."""
    return float(np.float32((float(p[PITCH, i]) + 1.37) % 3.0))


def test_history_and_mode_arithmetic():
    """The conventions the cases below build on: H at the three rates, and the mode lists for a change
    ahead of block 3 of 256-frame blocks, for one before the first frame and for the keeper."""
    assert (history(48000.0), history(44100.0), history(96000.0)) == (1154, 1062, 2306)
    assert expected_modes([256] * 14, {3}, H48) == [1] * 3 + [0] * 5 + [1] * 6
    assert expected_modes([256] * 3, {0}, H48) == [1] * 3           # a change before the first frame
    blocks = [4, 4096, 4, 256]
    assert expected_modes(blocks, set(keeper_events(8, blocks)), H48) == [1, 0, 0, 0]


# ------------------------------------------------------------------- 1, 2: ring mode held
@pytest.mark.parametrize("n", [70, 72])
def test_ring_mode_held_long_run(cuda, n):
    """The ring kernel for 34,720 frames on end (the keeper), 4,096-frame launches and tails: at pitch
    2.5 .. 3 Hz tap A's phasor wraps at least once and tap B's at least twice in every instance.
    n = 70 runs the per-lane I/O, n = 72 the rows."""
    blocks = [4] + [4096] * 8 + [1408, 4, 12, 272, 256]
    frames = sum(blocks)
    assert frames == 34724
    rng = np.random.default_rng(1200 + n)
    p = chorus_params(rng, n)
    p[PITCH] = rng.uniform(2.5, 3.0, n)
    p[DEPTH] = rng.choice([0.08, 0.2, 1.0], n)
    p[RATE] = rng.choice([0.01, 0.5, 1.0], n)
    p[WINDOW] = rng.choice([4.0, 7.3, 10.0], n)
    p[WINDOW, n - 1] = 5.5
    assert np.all(frames * p[PITCH, :n - 1].astype(np.float64) / SR >= 1.5)
    events = keeper_events(n, blocks)
    expect = expected_modes(blocks, set(events), H48)
    assert expect == [1] + [0] * (len(blocks) - 1)
    x = fast_noise(n, frames, seed=1200 + n)
    e, ref = engine(n), O.Chorus(n)
    apply(e, ref, p)
    y, yr, modes = run(e, ref, x, blocks, cuda, events)
    assert modes == expect
    assert bits_equal(y, yr), first_mismatch(y, yr)


def test_ring_mode_held_blocks_with_tails(cuda):
    """The ring kernel held (the keeper) over the corner draw of test_chorus_line_carry_stress (pitch 0
    and 0.01 included), block-sized launches and tails of 4, 12, 240 and 20 frames."""
    n = 96
    blocks = [4] + [256] * 24 + [4, 12, 240, 20, 256]
    p = corner_draw(n, 77)
    p[WINDOW, n - 1] = 5.5
    events = keeper_events(n, blocks)
    expect = expected_modes(blocks, set(events), H48)
    assert expect == [1] + [0] * (len(blocks) - 1)
    x = fast_noise(n, sum(blocks), seed=1300)
    e, ref = engine(n), O.Chorus(n)
    apply(e, ref, p)
    y, yr, modes = run(e, ref, x, blocks, cuda, events)
    assert modes == expect
    assert bits_equal(y, yr), first_mismatch(y, yr)


# ------------------------------------------------------------------- 3: switch across workgroups
@pytest.mark.parametrize("n", [130, 200, 1028])
def test_switch_across_workgroups(cuda, n):
    """A pitch change with more than 128 instances: chorus_materialise runs a second block in x (4
    threads of it at n = 130) and the chorus kernels a second workgroup.  Witnesses on both sides of
    the edge (1, 33, 126, 127, 128, n - 1) read the whole materialised history; 33, 127, 128 and n - 1
    change their own pitch, so a fill under the new coefficients shows, 1 and 126 do not."""
    blocks = [256] * 14
    witnesses = [1, 33, 126, 127, 128, n - 1]
    changed = [0, 31, 32, 33, 127, 128, n - 1]
    p = set_witnesses(draw(n, 1400 + n), witnesses)
    events = {3: [(i, PITCH, new_pitch(p, i)) for i in changed]}
    assert witness_delay(SR, 3 * 256) >= H48 - 4
    expect = expected_modes(blocks, {3}, H48)
    assert expect == [1] * 3 + [0] * 5 + [1] * 6
    x = fast_noise(n, sum(blocks), seed=1400 + n)
    e, ref = engine(n), O.Chorus(n)
    apply(e, ref, p)
    y, yr, modes = run(e, ref, x, blocks, cuda, events)
    assert modes == expect
    assert bits_equal(y, yr), first_mismatch(y, yr)


@pytest.mark.parametrize("n", [130, 1028])
def test_switch_across_workgroups_deep_history(cuda, n):
    """test_switch_across_workgroups with the change ahead of block 8: at frame 768 the deepest
    positions a witness reads lie before the start of the run, where the rings hold the zeros a
    materialise would write anyway; at frame 2,048 all 1,154 positions of the history (and the 480
    frames of input behind the deepest) are signal, so an unfilled or wrong position at any depth of
    any witness's history shows."""
    blocks = [256] * 18
    at = 8
    assert sum(blocks[:at]) >= H48 + 480
    witnesses = [1, 33, 126, 127, 128, n - 1]
    p = set_witnesses(draw(n, 1450 + n), witnesses)
    events = {at: [(i, PITCH, new_pitch(p, i)) for i in (0, 31, 32, 33, 127, 128, n - 1)]}
    assert witness_delay(SR, sum(blocks[:at])) >= H48 - 4
    expect = expected_modes(blocks, {at}, H48)
    assert expect == [1] * 8 + [0] * 5 + [1] * 5
    x = fast_noise(n, sum(blocks), seed=1450 + n)
    e, ref = engine(n), O.Chorus(n)
    apply(e, ref, p)
    y, yr, modes = run(e, ref, x, blocks, cuda, events)
    assert modes == expect
    assert bits_equal(y, yr), first_mismatch(y, yr)


# ------------------------------------------------------------------- 4: other sample rates
@pytest.mark.parametrize("n", [36, 70])
@pytest.mark.parametrize("sr", [44100.0, 96000.0])
def test_switch_at_other_sample_rates(cuda, sr, n):
    """44.1 kHz (history 1,062, x ring 2,048) and 96 kHz (2,306 and 4,096): a pitch change ahead of
    block 4, the ring kernel for ceil(H / 256) blocks, then ring-free in calls of 1,024, 4, 20 and 256
    frames for more than x ring + H + 10 ms, so that every position the tap reads has been recomputed
    from wrapped ring data; then a window change on another instance -- a second materialise, on a
    wrapped ring -- and on through the ring stretch into ring-free mode again."""
    H = history(sr)
    unit = [1024, 4, 20, 256]
    ring = math.ceil(H / 256)
    free = X_RING[sr] + H + math.ceil(0.010 * sr)
    stretch = unit * math.ceil(free / sum(unit))
    tail = unit * math.ceil((H + 1280) / sum(unit))
    blocks = [256] * 4 + [256] * ring + stretch + tail
    second = 4 + ring + len(stretch)
    assert sum(stretch) >= free and sum(tail) >= H + 1280
    witnesses = [1, n - 1]
    p = set_witnesses(draw(n, 1500 + n + int(sr) // 1000), witnesses)
    events = {4: [(i, PITCH, new_pitch(p, i)) for i in (n - 1, 3, 10)],
              second: [(5, WINDOW, 4.5 if p[WINDOW, 5] > 7.0 else 9.5)]}
    for b in events:
        assert witness_delay(sr, sum(blocks[:b])) >= H - 4
    expect = expected_modes(blocks, set(events), H)
    # ring mode from each change until H frames have passed, ring-free everywhere else
    assert expect[:4 + ring + 1] == [1] * 4 + [0] * ring + [1]
    assert expect[4 + ring:second] == [1] * len(stretch)
    after = np.cumsum([0] + tail)[:len(tail)]
    assert expect[second:] == [1 if s >= H else 0 for s in after] and expect[-1] == 1 and expect[second] == 0
    x = fast_noise(n, sum(blocks), seed=1500 + n)
    e, ref = engine(n, sr), O.Chorus(n, sample_rate=sr)
    apply(e, ref, p)
    y, yr, modes = run(e, ref, x, blocks, cuda, events)
    assert modes == expect
    assert bits_equal(y, yr), first_mismatch(y, yr)


# ------------------------------------------------------------------- 5: edges of the count
COUNT_EDGES = [
    # (blocks, the block the pitch changes ahead of, the modes)
    # a. a materialise from rings that hold 4 frames
    pytest.param([4] + [256] * 11, 1, [1] + [0] * 5 + [1] * 6, id="change_after_4_frames"),
    # b. the count reaches the history exactly: 1,152 + 4 = 1,156 >= 1,154 > 1,152
    pytest.param([256] * 3 + [1152, 4, 4] + [256] * 6, 3, [1] * 3 + [0, 0, 1] + [1] * 6, id="count_reaches_history"),
    # c. the first ring-free launches after a ring stretch are shorter than a chunk and ragged: the tail
    #    pass and generic chunks on data the ring kernel wrote
    pytest.param([256] * 8 + [4, 20, 4, 256] + [256] * 5, 3, [1] * 3 + [0] * 5 + [1] * 9,
                 id="short_launches_after_ring"),
    # d. one launch longer than the history
    pytest.param([256] * 3 + [2048] + [256] * 6, 3, [1] * 3 + [0] + [1] * 6, id="one_long_ring_block"),
]


@pytest.mark.parametrize("blocks,at,stated", COUNT_EDGES)
def test_edges_of_the_count(cuda, blocks, at, stated):
    """The frame count at its edges (COUNT_EDGES), each run on for at least 1,280 frames after the
    change.  Instance 1 is a witness and changes its pitch with three others; n - 1 is one that does not."""
    n = 36
    assert sum(blocks[at:]) >= 1280 and len(stated) == len(blocks)
    p = set_witnesses(draw(n, 1600 + len(blocks)), [1, n - 1])
    events = {at: [(i, PITCH, new_pitch(p, i)) for i in (1, 3, 20, 34)]}
    assert witness_delay(SR, sum(blocks[:at])) >= H48 - 4
    expect = expected_modes(blocks, {at}, H48)
    assert expect == stated
    x = fast_noise(n, sum(blocks), seed=1600 + len(blocks))
    e, ref = engine(n), O.Chorus(n)
    apply(e, ref, p)
    y, yr, modes = run(e, ref, x, blocks, cuda, events)
    assert modes == expect
    assert bits_equal(y, yr), first_mismatch(y, yr)


# ------------------------------------------------------------------- 6: changes that must not switch
@pytest.mark.parametrize("n", [36, 33])
def test_changes_that_do_not_switch(cuda, n):
    """Ring-free throughout.  More than 1,500 frames in, at block boundaries (one ahead of a 4-frame
    block): depth 0.08 -> 1.0 on a phase-0, rate-0.01 instance moves its tap from 180 to 1,152 frames
    back at once, onto pitch-shifter output the kernel has to rebuild from the input ring, and later
    1.0 -> 0.08 back; phase, rate, mix, q and cutoff changes; a pitch of 7.0 on an instance at 3.0 and
    of -2.0 on one at 0.0 clamp to the value in force and change no word."""
    blocks = [256] * 6 + [256, 4, 256, 256, 20, 256] + [256] * 6
    p = draw(n, 1700 + n)
    far, ph, rt, misc = 20, 10, 11, 12
    for f, v in {PHASE: 0.0, RATE: 0.01, DEPTH: 0.08, MIX: 1.0}.items():
        p[f, far] = v
    p[PHASE, ph] = 0.1
    p[RATE, rt] = 0.01
    assert p[PITCH, 3] == 3.0 and p[PITCH, 2] == 0.0
    events = {
        6: [(far, DEPTH, 1.0), (ph, PHASE, 0.6)],
        7: [(rt, RATE, 1.0), (misc, MIX, 0.05), (misc, Q, 0.9), (misc, CUTOFF, 0.95)],      # a 4-frame block
        8: [(3, PITCH, 7.0), (2, PITCH, -2.0)],
        12: [(far, DEPTH, 0.08)],
    }
    assert blocks[7] == 4 and sum(blocks[:6]) >= 1500
    # the tap jumps back by more than 900 frames, and forward again
    t6, t12 = sum(blocks[:6]), sum(blocks[:12])
    assert tap_delay(SR, t6, 1.0, 0.01, 0.0) - tap_delay(SR, t6, 0.08, 0.01, 0.0) > 900
    assert tap_delay(SR, t12, 1.0, 0.01, 0.0) - tap_delay(SR, t12, 0.08, 0.01, 0.0) > 900
    assert sum(blocks[12:]) >= 1280
    x = fast_noise(n, sum(blocks), seed=1700 + n)
    e, ref = engine(n), O.Chorus(n)
    apply(e, ref, p)
    y, yr, modes = run(e, ref, x, blocks, cuda, events)
    assert modes == [1] * len(blocks)
    assert bits_equal(y, yr), first_mismatch(y, yr)


# ------------------------------------------------------------------- 7: streams and host I/O
def test_streams_and_host_io_at_the_materialise(cuda):
    """The same script twice: device buffers with the blocks alternating between two streams, so the
    block the pitch change lands on (materialise, scatter and ring kernel) runs on another stream
    than the block before it; and host arrays staged by the library.  Both bit-exact against the
    oracle and against each other."""
    import torch
    n = 72
    blocks = [256] * 12
    p = set_witnesses(draw(n, 1800), [1, n - 1])
    events = {5: [(i, PITCH, new_pitch(p, i)) for i in (1, 3, 40, 71)]}
    assert witness_delay(SR, 5 * 256) >= H48 - 4
    expect = expected_modes(blocks, {5}, H48)
    assert expect == [1] * 5 + [0] * 5 + [1] * 2
    x = fast_noise(n, sum(blocks), seed=1800)
    ref = O.Chorus(n)
    apply_oracle(ref, p)
    yr = run_oracle(ref, x, blocks, events)
    es, eh = engine(n), engine(n)
    es.set_params(0, p)
    eh.set_params(0, p)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    # every input made before the loop and kept alive: a freed tensor's memory would be reused by the
    # caching allocator while the other stream still reads it
    xb = [np.ascontiguousarray(x[:, b * 256:(b + 1) * 256]) for b in range(len(blocks))]
    xs = [torch.from_numpy(v).to(cuda) for v in xb]
    torch.cuda.synchronize()
    outs, modes_s, modes_h, host = [], [], [], []
    for b in range(len(blocks)):
        for inst, field, value in events.get(b, []):
            es.set_param(inst, field, value)
            eh.set_param(inst, field, value)
        modes_s.append(es.chorus_ring_free)
        modes_h.append(eh.chorus_ring_free)
        s = streams[b % 2]
        with torch.cuda.stream(s):
            outs.append(es.process(xs[b], stream=s.cuda_stream))
        host.append(eh.process(xb[b]))
    torch.cuda.synchronize()
    ys = np.concatenate([o.cpu().numpy() for o in outs], 1)
    yh = np.concatenate(host, 1)
    assert modes_s == expect and modes_h == expect
    assert bits_equal(ys, yr), first_mismatch(ys, yr)
    assert bits_equal(yh, yr), first_mismatch(yh, yr)
    assert bits_equal(ys, yh), first_mismatch(ys, yh)


# ------------------------------------------------------------------- 8: edge signals through a switch
@pytest.mark.parametrize("n", [70, 72])
@pytest.mark.parametrize("signal", ["subnormal", "loud127"])
def test_edge_signals_through_a_switch(cuda, signal, n):
    """helpers.edge_signals' subnormal (x * 2^-130) and loud127 (x * 2^127) input through a pitch change
    on four instances ahead of block 5: the materialise reads and writes subnormal (or huge) history.
    Oracle-side conditions as in test_gpu_edges.test_signal_edges: at least half of the oracle's
    non-zero samples subnormal; at least 5 % of them non-finite under loud127."""
    blocks = [256] * 12
    p = set_witnesses(draw(n, 1900 + n), [1, n - 1])
    events = {5: [(i, PITCH, new_pitch(p, i)) for i in (1, 3, 40, n - 1)]}
    assert witness_delay(SR, 5 * 256) >= H48 - 4
    expect = expected_modes(blocks, {5}, H48)
    assert expect == [1] * 5 + [0] * 5 + [1] * 2
    x = edge_signals(fast_noise(n, sum(blocks), seed=40))[signal]
    ref = O.Chorus(n)
    apply_oracle(ref, p)
    yr = run_oracle(ref, x, blocks, events)
    sub, nonfin = subnormal_share(yr), nonfinite_share(yr)
    print(f"\nn={n} {signal}: oracle subnormal share of non-zero {100 * sub:.1f} %, "
          f"non-finite share {100 * nonfin:.1f} %")
    if signal == "subnormal":
        assert np.any(yr != 0) and sub >= 0.5
    else:
        assert nonfin >= 0.05
    e, ref2 = engine(n), O.Chorus(n)
    apply(e, ref2, p)
    y, yr2, modes = run(e, ref2, x, blocks, cuda, events)
    assert modes == expect
    assert same_bits_or_nan(yr2, yr)                     # the oracle again, alongside the engine
    assert same_bits_or_nan(y, yr), first_mismatch_or_nan(y, yr)
