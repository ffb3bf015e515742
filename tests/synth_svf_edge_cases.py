"""The synth's edge cases (tests/edge_fused_cases.py, section C) for OLFX_KIND_SYNTH_SVF, as data: the
same corner matrices (_voice_corners x _rack_corners), shapes, ragged 1,024-frame split and sample rates,
with both rack topologies in every case and tests/synth_svf_ref.py as the reference.

tests/test_synth_svf_edge_ref.py runs every reference alone on the CPU and asserts its condition;
tests/test_gpu_edges_synth_svf.py runs the same cases on the engine and asserts the same condition before
it compares (synth_ref.bits_equal).  The references need the committed v_rcp_f32 table installed.
"""
from __future__ import annotations

import numpy as np

import synth_ref as SYN
import synth_svf_ref as SV
from edge_fused_cases import (FTYPE, RAGGED_1024, RATES, SYNTH_CORNER_SHAPES, SYNTH_RATE_N, _rack_corners, _say,
                              _sounding, _voice_corners)
from test_gpu_edges import CONTAIN_CALLS

CORNER_SHAPES = SYNTH_CORNER_SHAPES          # (256, 4), (70, 8): the wave that runs two voices
CONTAIN_SHAPES = [(70, 4), (70, 8)]          # the last group's D1 wave has no instrument
RATE_N = SYNTH_RATE_N


def corner_script(n: int, P: int):
    """edge_fused_cases.synth_corner_script with the Svf synth's topologies: each of the 27 fields before
    the topology at its corner value with probability 1/2 (voice fields as test_voice_corners -- the
    filter drive is live here --, rack fields as the plate rack's corners, master volume included), else
    at the interior value of synth_svf_ref.params(n, 35); the filter type is the corner matrix's integer;
    the topology is i % 2.  Every voice gets a NoteOn from the ends and the middle of the MIDI range;
    1024 ragged frames; a NoteOff of each instrument's first note; 1024 more."""
    rng = np.random.default_rng(35)
    topo = (np.arange(n) % 2)[None, :].astype(np.float32)
    corner = np.concatenate([_voice_corners(rng, n), _rack_corners(rng, n), topo], 0)
    interior = SV.params(n, 35)
    assert corner.shape == interior.shape == (28, n)
    p = np.where(rng.random((28, n)) < 0.5, corner, interior).astype(np.float32)
    p[FTYPE] = corner[FTYPE]
    p[SV.TOPOLOGY] = topo[0]
    notes = rng.choice([1, 21, 60, 108, 127], (n, P))
    s = [("params", p), ("events", [(i, SYN.EV_NOTE_ON, int(notes[i, v])) for i in range(n) for v in range(P)]),
         ("check_playing",)]
    s += [("block", b) for b in RAGGED_1024]
    s += [("events", [(i, SYN.EV_NOTE_OFF, int(notes[i, 0])) for i in range(n)]), ("check_playing",)]
    s += [("block", b) for b in RAGGED_1024]
    return s


def corner_condition(n: int, P: int, yr: np.ndarray, topo: np.ndarray) -> None:
    """Finite; at each topology channel 0 is non-zero on at least a third of its instruments (a corner
    draw silences some: amp amount 0, master volume 0, delay balance 1 with a one-second delay); channel 1
    is non-zero on at least a third of the topology-1 instruments and all +-0 on every topology-0 one."""
    assert np.all(np.isfinite(yr))
    snd = _sounding(yr)
    at1 = topo == 1.0
    assert at1.any() and (~at1).any()
    c0_0, c0_1, c1_1 = float(np.mean(snd[0][~at1])), float(np.mean(snd[0][at1])), float(np.mean(snd[1][at1]))
    _say(f"synth_svf n={n} P={P} half-corners: channel 0 non-zero on {100 * c0_0:.0f} % of the reference's "
         f"topology-0 instruments and {100 * c0_1:.0f} % of its topology-1 ones, channel 1 on {100 * c1_1:.0f} % of "
         f"the topology-1 ones; largest sample {np.abs(yr).max():.1f}")
    assert min(c0_0, c0_1, c1_1) >= 1 / 3
    assert not np.any(snd[1][~at1])


def contain_script(n: int, P: int):
    return [("params", SV.params(n, 5)), ("events", SYN.notes_on(n, P))] + [("block", b) for b in CONTAIN_CALLS]


def contain_condition(yr: np.ndarray, ref) -> None:
    """The containment runs: the scripts' own condition (finite, so that the NaN sentinel is unmistakable;
    channel 1 all zeros at topology 0 -- zeros the kernel must have written)."""
    SV.condition(yr, ref.topology_of_frames())


def rate_script():
    return SV.with_topologies(SYN.script_ragged_frames(RATE_N), 5)


def rate_condition(yr: np.ndarray, ref, yr48: np.ndarray) -> None:
    SV.condition(yr, ref.topology_of_frames())
    assert np.any(yr.view(np.uint32) != yr48.view(np.uint32))
