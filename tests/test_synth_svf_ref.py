"""tests/synth_svf_ref.py anchored on the CPU: the composed Svf-synth reference reduces to its parts where
it must at both topologies, and every script tests/test_gpu_synth_svf.py runs on the engine gives a
reference that meets the condition those tests state (synth_svf_ref.condition: finite; channel 0 non-zero
for every instrument; channel 1 non-zero at topology 1 and all +-0 at topology 0)."""
import numpy as np
import pytest

import oracle as O
import synth_ref as SR
import synth_svf_ref as SV
from helpers import bits_equal, first_mismatch, voice_configs


@pytest.fixture(scope="module", autouse=True)
def rcp():
    SV.install_rcp()
    yield
    SV.remove_rcp()


def test_one_voice_is_the_svf_voice_through_the_rack_at_its_topology():
    """P = 1: the instrument is its voice (0.0f + v) in channel 0 of an O.FxRack instance at the
    instrument's topology, zeros in channel 1 -- the Svf voice, not the Moog one."""
    n, frames = 6, 700
    rng = np.random.default_rng(3)
    p = SV.params(n, 5)
    p[:SV.NV] = voice_configs(rng, n)
    p[SV.TOPOLOGY] = np.arange(n) % 2
    s = SV.Synth(n, voices=1)
    s.set_params(p)
    voice, moog = O.Voice(n, moog=False, kernel_arith=True), O.Voice(n, moog=True, kernel_arith=True)
    rack = O.FxRack(n)
    for i in range(n):
        voice.config(i, p[:SV.NV, i])
        moog.config(i, p[:SV.NV, i])
        for f in range(SV.NR):
            rack.set(i, f, float(p[SV.NV + f, i]))
        for v in (s, voice, moog):
            v.event(i, SV.EV_NOTE_ON, 50 + i)
    y = s.process(frames)
    mono = (np.float32(0.0) + voice.process(frames)[0]).astype(np.float32)
    yr = rack.process(np.stack([mono, np.zeros_like(mono)]))
    SV.condition(y, s.topology_of_frames())
    assert bits_equal(y, yr), first_mismatch(y, yr)
    assert not bits_equal(mono, moog.process(frames)[0])


def test_topology_zero_applies_the_master_and_silences_channel_one():
    """Two instruments with the same parameters but the topology: channel 0 of the topology-0 one is the
    topology-1 one's times the master volume (the same chain up to filter1), channel 1 is 0.0f x master."""
    n, frames = 2, 600
    p = SV.params(n, 6)
    p[:, 1] = p[:, 0]
    p[SV.TOPOLOGY] = [0.0, 1.0]
    p[SV.MASTER] = 0.625
    s = SV.Synth(n, voices=4)
    s.set_params(p)
    for i in range(n):
        for note in (48, 64, 79):
            s.event(i, SV.EV_NOTE_ON, note)
    y = s.process(frames)
    SV.condition(y, s.topology_of_frames())
    assert bits_equal(y[0][:, 0], (y[0][:, 1] * np.float32(0.625)).astype(np.float32))
    assert np.all(y[1][:, 0] == 0) and np.any(y[1][:, 1] != 0)
    with pytest.raises(AssertionError):
        SV.condition(y, s.topology_of_frames()[:, ::-1])       # the condition tells the topologies apart


def test_scripts_carry_both_topologies():
    for name in sorted(SV.GPU_SCRIPTS):
        script, n, _ = SV.GPU_SCRIPTS[name]()
        topo = script[0][1][SV.TOPOLOGY]
        assert set(np.unique(topo)) <= {0.0, 1.0}
        assert n == 1 or set(np.unique(topo)) == {0.0, 1.0}, name
    script, n, _ = SV.GPU_SCRIPTS["topology_mix"]()
    p = script[0][1]
    assert np.array_equal(p[SV.TOPOLOGY], np.arange(n) % 2) and not np.any(p[SV.MASTER] == 1.0)
    switches = [(s[1], s[3]) for s in script if s[0] == "set" and s[2] == SV.TOPOLOGY]
    assert {v for _, v in switches} == {0.0, 1.0} and len(switches) >= 8
    # the delay-line script keeps synth_ref's line delays on the first and last instruments
    script, n, _ = SV.GPU_SCRIPTS["delay_lines"]()
    d = (script[0][1][SR.RACK_TIME] * np.float32(48000.0)).astype(np.int64)
    assert set(SR.LINE_DELAYS) <= set(d[:7].tolist()) and set(SR.LINE_DELAYS) <= set(d[-7:].tolist())


@pytest.mark.parametrize("name", sorted(SV.GPU_SCRIPTS))
def test_gpu_scripts_meet_their_condition(name):
    script, n, voices = SV.GPU_SCRIPTS[name]()
    yr, ref = SV.run_ref(script, n, voices, threads=8)
    SV.condition(yr, ref.topology_of_frames())
