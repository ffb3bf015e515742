"""The fused kinds' edge cases (tests/synth_svf_edge_cases.py) for OLFX_KIND_DRUMKIT, as data: the same corner
matrices (_voice_corners per voice slot x _rack_corners), ragged 1,024-frame split, containment calls and sample
rates, with both rack topologies in every case and tests/drumkit_ref.py as the reference.

tests/test_drumkit_edge_ref.py runs every reference alone on the CPU and asserts its condition;
tests/test_gpu_edges_drumkit.py runs the same cases on the engine and asserts the same condition before it
compares (bit-exact).  The references need the committed v_rcp_f32 table installed.

The kind has no audio input and its setters refuse non-finite values, so it has no signal and no poison case.
"""
from __future__ import annotations

import numpy as np

import drumkit_ref as DK
from edge_fused_cases import RAGGED_1024, RATES, _rack_corners, _say, _sounding, _voice_corners
from test_gpu_edges import CONTAIN_CALLS

CORNER_SHAPES = [(130, 4), (70, 8)]          # three groups; the waves that run two voices
CONTAIN_SHAPES = [(70, 4), (70, 8)]          # the last group's D1 wave has no kit
RATE_N = 33
FTYPE = DK.RACK0 + 9


def setup(n: int, P: int, gain: float = 1.0):
    """script_sum_order's bank (times `gain`, a power of two), looping assignments and reordered map: every voice
    sounds."""
    bank, samples, kmap = DK.script_sum_order(n, P)[1:4]
    return [("bank", [x * np.float32(gain) for x in bank[1]]), samples, kmap]


def corner_script(n: int, P: int):
    """Each of the 139 fields before the topology at its corner value with probability 1/2 (every voice slot its
    own _voice_corners draw, the rack's _rack_corners, master volume included), else at the interior value of
    drumkit_ref.params(n, 35); the filter type is the corner matrix's integer; the topology is i % 2.  Every
    voice gets its NoteOn; 1024 ragged frames; a NoteOff of each kit's voice 0; 1024 more."""
    rng = np.random.default_rng(35)
    topo = (np.arange(n) % 2)[None, :].astype(np.float32)
    corner = np.concatenate([_voice_corners(rng, n) for _ in range(DK.SLOTS)] + [_rack_corners(rng, n), topo], 0)
    interior = DK.params(n, 35)
    assert corner.shape == interior.shape == (DK.NPARAMS, n)
    p = np.where(rng.random((DK.NPARAMS, n)) < 0.5, corner, interior).astype(np.float32)
    p[FTYPE] = corner[FTYPE]
    p[DK.TOPOLOGY] = topo[0]
    # the bank an eighth as loud: at full level the sum of up to eight resonating voices drives the rack's corner
    # draws (feedback 1, resonance 1) to non-finite levels on three kits, and the case, like the synths', asks
    # for a finite reference
    s = [("params", p)] + setup(n, P, 0.125) + [("events", DK.notes_on(n, P, note=DK.note_of)), ("check_playing",)]
    s += [("block", b) for b in RAGGED_1024]
    s += [("events", [(i, DK.EV_NOTE_OFF, DK.note_of(i, 0)) for i in range(n)]), ("check_playing",)]
    s += [("block", b) for b in RAGGED_1024]
    return s


def corner_condition(n: int, P: int, yr: np.ndarray, topo: np.ndarray) -> None:
    """Finite; at each topology channel 0 is non-zero on at least a third of its kits (a corner draw silences
    some: amp amounts 0, master volume 0, delay balance 1 with a one-second delay); channel 1 is non-zero on at
    least a third of the topology-1 kits and all +-0 on every topology-0 one."""
    assert np.all(np.isfinite(yr))
    snd = _sounding(yr)
    at1 = topo == 1.0
    assert at1.any() and (~at1).any()
    c0_0, c0_1, c1_1 = float(np.mean(snd[0][~at1])), float(np.mean(snd[0][at1])), float(np.mean(snd[1][at1]))
    _say(f"drumkit n={n} P={P} half-corners: channel 0 non-zero on {100 * c0_0:.0f} % of the reference's topology-0 "
         f"kits and {100 * c0_1:.0f} % of its topology-1 ones, channel 1 on {100 * c1_1:.0f} % of the topology-1 ones; "
         f"largest sample {np.abs(yr).max():.1f}")
    assert min(c0_0, c0_1, c1_1) >= 1 / 3
    assert not np.any(snd[1][~at1])


def contain_script(n: int, P: int):
    return ([("params", DK.params(n, 5))] + setup(n, P) + [("events", DK.notes_on(n, P, note=DK.note_of))] +
            [("block", b) for b in CONTAIN_CALLS])


def contain_condition(yr: np.ndarray, ref) -> None:
    """The scripts' own condition: finite, so that the NaN sentinel is unmistakable; channel 1 all zeros at
    topology 0 -- zeros the kernel must have written."""
    DK.condition(yr, ref)


def rate_script():
    s = DK.script_ragged_frames(RATE_N)
    s[0] = ("params", DK.params(RATE_N, 5))
    return s


def rate_condition(yr: np.ndarray, ref, yr48: np.ndarray) -> None:
    DK.condition(yr, ref)
    assert np.any(yr.view(np.uint32) != yr48.view(np.uint32))
