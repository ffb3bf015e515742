"""Shared by the chorus-kind mode tests (test_gpu_chorus_ringfree.py, test_gpu_chorus_modes.py): the
drawn parameters with their fixed columns, the block-by-block runner against the CPU oracle, and what a
test needs to state its expectations WITHOUT asking the engine: the chorus history H(sr), the mode
each block must run in, the keeper that holds ring mode and the witness that reads the whole history."""
import math

import numpy as np

from helpers import chorus_params

PITCH, MIX, Q, CUTOFF, PHASE, DEPTH, RATE, WINDOW = range(8)
HISTORY = 1154                      # frames the ring kernel runs after a pitch / window change (48 kHz)

# instance -> {field: value}.  The LFO advances 0.5 Hz / 48 kHz = 1.04e-5 cycle per frame at rate 1:
# a phase offset just below 1/2 (or 1) makes the delay pass its minimum 0 (or its maximum) mid-run.
COLUMNS = {
    0: {DEPTH: 0.08, RATE: 1.0, PHASE: 0.488},     # delay through 0: psv of the current chunk's own frames
    1: {DEPTH: 1.0, PHASE: 0.0},                    # delay 1,152, the largest
    2: {PITCH: 0.0},                                # unit ratio: the pitch windows advance exactly one line
    3: {PITCH: 3.0},                                # fastest advance: two-line steps and phasor wraps
    4: {DEPTH: 1.0, RATE: 1.0, PHASE: 0.75},        # the fastest delay sweep (|d'| = 0.038 frame / frame)
    5: {DEPTH: 1.0, RATE: 1.0, PHASE: 0.994},       # delay through its maximum mid-run
    6: {DEPTH: 0.08, PITCH: 3.0, WINDOW: 10.0, PHASE: 0.5},   # delay 0 with the longest pitch window
    7: {PITCH: 3.0, WINDOW: 4.0},
}

# An instance whose chorus tap sits at the largest delay (depth 1, LFO phase 0 at the slowest rate) and
# whose output is all wet: it reads every position a materialise fills.
WITNESS = {DEPTH: 1.0, PHASE: 0.0, RATE: 0.01, MIX: 1.0}


def draw(n, seed):
    p = chorus_params(np.random.default_rng(seed), n)
    for i, col in COLUMNS.items():
        for f, v in col.items():
            p[f, i] = v
    return p


def corner_draw(n, seed):
    """test_gpu_parity.test_chorus_line_carry_stress's draw: every parameter that shapes a tap window
    at its corners (pitch 0 and 0.01 included)."""
    rng = np.random.default_rng(seed)
    p = np.empty((8, n), np.float32)
    p[PITCH] = rng.choice([0.0, 0.01, 1.0, 2.5, 3.0], n)
    p[MIX] = rng.uniform(0, 1, n)
    p[Q] = rng.uniform(0, 0.95, n)
    p[CUTOFF] = rng.uniform(0, 1, n)
    p[PHASE] = rng.uniform(0, 1, n)
    p[DEPTH] = rng.choice([0.08, 0.2, 1.0], n)
    p[RATE] = rng.choice([0.01, 0.5, 1.0], n)
    p[WINDOW] = rng.choice([4.0, 7.3, 10.0], n)
    return p


def set_witnesses(p, instances):
    for i in instances:
        for f, v in WITNESS.items():
            p[f, i] = v
    return p


def apply_oracle(ref, p):
    for i in range(p.shape[1]):
        for f in range(8):
            ref.set(i, f, float(p[f, i]))


def apply(e, ref, p):
    e.set_params(0, p)
    apply_oracle(ref, p)


def run(e, ref, x, blocks, cuda, events=None):
    """Block by block through the engine; events[b] = [(inst, field, value), ...] applied to the engine
    and the oracle ahead of block b.  Returns the engine's output, the oracle's, and the mode the
    engine reported ahead of each block (after that block's sets)."""
    import torch
    events = events or {}
    outs, refs, modes = [], [], []
    f0 = 0
    for b, frames in enumerate(blocks):
        for inst, field, value in events.get(b, []):
            e.set_param(inst, field, value)
            ref.set(inst, field, float(value))
        modes.append(e.chorus_ring_free)
        xh = np.ascontiguousarray(x[:, f0:f0 + frames])
        outs.append(e.process(torch.from_numpy(xh).to(cuda)).cpu().numpy())
        refs.append(ref.process(xh, threads=8))
        f0 += frames
    torch.cuda.synchronize()
    return np.concatenate(outs, axis=1), np.concatenate(refs, axis=1), modes


def run_oracle(ref, x, blocks, events=None):
    """The oracle's side of run() alone."""
    events = events or {}
    refs, f0 = [], 0
    for b, frames in enumerate(blocks):
        for inst, field, value in events.get(b, []):
            ref.set(inst, field, float(value))
        refs.append(ref.process(np.ascontiguousarray(x[:, f0:f0 + frames]), threads=8))
        f0 += frames
    return np.concatenate(refs, axis=1)


def history(sr):
    """H(sr): the spec's largest chorus delay (2 x 12 ms, in whole frames) plus 2."""
    return 2 * math.ceil(12 * sr / 1000) + 2


def expected_modes(blocks, changes, H):
    """The mode ahead of each block (1 ring-free, 0 ring kernel) when a pitch or window word changes
    ahead of the blocks in `changes`: the ring kernel from a change until H frames have passed since
    the latest one; a change before the first frame does not count (all history is zero)."""
    modes, seen, since = [], 0, None       # frames so far; frames since the latest change that counted
    for b, frames in enumerate(blocks):
        if b in changes and seen > 0:
            since = 0
        modes.append(1 if since is None or since >= H else 0)
        seen += frames
        if since is not None:
            since += frames
    return modes


def keeper_events(n, blocks):
    """The last instance's window flipped between 5.5 and 5.6 ms ahead of every block from block 1 on
    (its parameters start at 5.5): every block after the first runs the ring kernel."""
    return {b: [(n - 1, WINDOW, 5.6 if b % 2 else 5.5)] for b in range(1, len(blocks))}


def tap_delay(sr, frame, depth, rate, phase):
    """The chorus tap's delay in frames at `frame`, in double, by the oracle's own formula
    (oracle/chorus_ref.c derive / chorus_split: D cos(2 pi (frame rate_hz / sr + phase)) + D)."""
    depth, rate, phase = (float(np.float32(v)) for v in (depth, rate, phase))
    rate_hz = 0.01 + rate * (0.5 - 0.01)
    D = (1.0 + depth * (12.0 - 1.0)) * sr / 1000.0
    return D * math.cos(2.0 * math.pi * (frame * rate_hz / sr + phase)) + D


def witness_delay(sr, frame):
    return tap_delay(sr, frame, WITNESS[DEPTH], WITNESS[RATE], WITNESS[PHASE])
