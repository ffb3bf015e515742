"""The reference for OLFX_KIND_SYNTH_SVF: tests/synth_ref.py's composition with the library's own voice
and the rack at each instrument's topology -- existing oracles only, no new arithmetic.

Per block, for n instruments of P voices ([2][frames][n] float32 out):
  1. v = O.Voice(P * n, moog=False, kernel_arith=True): voice p * n + i is voice p of instrument i
     (voice_block_v5's arithmetic with the committed v_rcp_f32 model, oracle/voice_ref.c);
  2. mono = O.mix_ref(v, [[0 * n + i, 1 * n + i, ...]]): Polyvoice::Process from 0.0f;
  3. out = O.FxRack(n) on (mono, 0) with instance i at instrument i's topology: 1 the firmware callback,
     0 FxRack<2>::Process with its master volume (output channel 1 is 0.0f x master).
The Polyvoice rule, the script format and the scripts themselves are synth_ref's; the parameters are
workload.RANGES["synth_svf"], which are the synth's draw field for field (the same hash of seed, field
and instrument) with the topology drawn from {0, 1} instead of fixed at 1.

The condition every script's reference must meet (condition()): finite everywhere; channel 0 non-zero
for every instrument; channel 1 non-zero for every instrument over the frames it spends at topology 1
and all +-0 over the frames it spends at topology 0.  tests/test_synth_svf_ref.py holds every GPU
script to it on the CPU; tests/test_gpu_synth_svf.py asserts it again before comparing.
"""
from __future__ import annotations

import numpy as np

import oracle as O
import synth_ref as SR
from ol_dsp_amd import workload

NV, NR, FIELDS, TOPOLOGY = SR.NV, SR.NR, SR.FIELDS, SR.TOPOLOGY
MASTER = NV + O.FR_FIELDS.index("master_volume")
EV_NOTE_OFF, EV_NOTE_ON, EV_GATE_ON, EV_GATE_OFF = SR.EV_NOTE_OFF, SR.EV_NOTE_ON, SR.EV_GATE_ON, SR.EV_GATE_OFF
install_rcp, remove_rcp, bits_equal, notes_on = SR.install_rcp, SR.remove_rcp, SR.bits_equal, SR.notes_on


class Synth(SR.Synth):
    """synth_ref.Synth over SvfFilter voices; the rack's topology is per instrument, 0 or 1."""

    def __init__(self, n: int, voices: int = 4, sample_rate: float = 48000.0):
        super().__init__(n, voices, sample_rate)
        self.voice = O.Voice(voices * n, sample_rate, moog=False, kernel_arith=True)
        self.topo_log = []                                   # per block: (frames, topology [n])

    def set(self, inst: int, field, value: float) -> None:
        f = FIELDS.index(field) if isinstance(field, str) else int(field)
        if f != TOPOLOGY:
            return super().set(inst, f, value)
        assert float(value) in (0.0, 1.0)
        self.p[f, inst] = np.float32(value)
        self.rack.set(inst, f - NV, float(value))

    def process(self, frames: int, threads: int = 4) -> np.ndarray:
        assert np.all(np.isin(self.p[TOPOLOGY], [0.0, 1.0]))
        self.topo_log.append((frames, self.p[TOPOLOGY].copy()))
        return super().process(frames, threads)

    def topology_of_frames(self) -> np.ndarray:
        """[frames][n]: each instrument's topology at each frame processed so far."""
        return np.concatenate([np.tile(t[None, :], (f, 1)) for f, t in self.topo_log], 0)


def run_ref(script, n: int, voices: int = 4, threads: int = 4, sample_rate: float = 48000.0):
    """synth_ref.run_ref on the Svf synth: ([2][frames][n], the Synth)."""
    ref = Synth(n, voices, sample_rate)
    ref.trace = []
    out = []
    for step in script:
        if step[0] == "params":
            ref.set_params(step[1])
        elif step[0] == "set":
            ref.set(step[1], step[2], step[3])
        elif step[0] == "events":
            for inst, type_, note in step[1]:
                ref.event(inst, type_, note)
        elif step[0] == "block":
            out.append(ref.process(step[1], threads))
        elif step[0] == "check_playing":
            ref.trace.append(ref.playing.copy())
    return np.concatenate(out, 1), ref


def condition(yr: np.ndarray, topo: np.ndarray) -> None:
    """yr [2][frames][n], topo [frames][n] (Synth.topology_of_frames)."""
    assert topo.shape == yr.shape[1:]
    assert np.isfinite(yr).all(), np.argwhere(~np.isfinite(yr))[:4]
    silent = np.flatnonzero(~np.any(yr[0] != 0, axis=0))
    assert silent.size == 0, ("channel 0 silent", silent[:8])
    at1, at0 = topo == 1.0, topo == 0.0
    assert np.all(at1 | at0)
    # topology 1: the reverb's channel 1 sounds on every instrument that spends frames there
    silent = np.flatnonzero(np.any(at1, axis=0) & ~np.any((yr[1] != 0) & at1, axis=0))
    assert silent.size == 0, ("channel 1 silent at topology 1", silent[:8])
    # topology 0: 0.0f x master, every frame
    loud = np.argwhere((yr[1] != 0) & at0)
    assert loud.size == 0, ("channel 1 non-zero at topology 0", loud[:4])


def params(n: int, seed: int) -> np.ndarray:
    return workload.instance_params("synth_svf", 0, n, seed)


def with_topologies(script, seed: int):
    """A synth_ref script with each ("params", p) step's topology row replaced by the Svf synth's draw:
    every other field of workload.RANGES["synth_svf"] is the synth's own."""
    out = []
    for step in script:
        if step[0] == "params":
            p = step[1].copy()
            q = params(p.shape[1], seed)
            p[TOPOLOGY] = q[TOPOLOGY]
            keep = np.arange(p.shape[0]) != TOPOLOGY
            keep[SR.RACK_TIME] = False                       # (the delay-line script overwrites some times)
            assert np.array_equal(p[keep], q[keep])
            step = ("params", p)
        out.append(step)
    return out


def script_topology_mix(n: int = 70):
    """Even instruments at topology 0, odd ones at 1 (both in every lane pair of D); master volumes
    0.25 .. 1.6, none of them 1; between the blocks a few instruments switch 0 -> 1 and 1 -> 0, one of
    them back again."""
    p = params(n, 7)
    p[TOPOLOGY] = np.arange(n) % 2
    p[MASTER] = np.float32(0.25) + np.float32(1.35) * (np.arange(n) % 7).astype(np.float32) / np.float32(6)
    p[MASTER, p[MASTER] == 1.0] = 1.125
    assert not np.any(p[MASTER] == 1.0)
    s = [("params", p), ("events", notes_on(n, 4)), ("block", 256)]
    s += [("set", i, TOPOLOGY, 1.0) for i in (0, 32, 64, 68)] + [("set", i, TOPOLOGY, 0.0) for i in (1, 33, 63, 69)]
    s += [("block", 100), ("set", 0, TOPOLOGY, 0.0), ("set", 69, TOPOLOGY, 1.0), ("block", 256)]
    return s


GPU_SCRIPTS = {
    **{f"ragged_instances_{n}": (lambda n=n: (with_topologies(SR.script_ragged_instances(n), 5), n, 4))
       for n in (1, 33, 65, 130)},
    **{f"voices_{P}": (lambda P=P: (with_topologies(SR.script_voices(P), 6), 65, P)) for P in (1, 2, 5, 8)},
    "ragged_frames": lambda: (with_topologies(SR.script_ragged_frames(), 5), 65, 4),
    "delay_lines": lambda: (with_topologies(SR.script_delay_lines(), 6), 65, 4),
    "topology_mix": lambda: (script_topology_mix(), 70, 4),
    "storm": lambda: (SR.resolve_storm(with_topologies(SR.script_storm(total=2000), 5), 33), 33, 4),
    "param_change": lambda: (with_topologies(SR.script_param_change(), 5), 33, 4),
}
