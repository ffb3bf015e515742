"""tests/synth_ref.py anchored on the CPU: the composed synth reference reduces to its parts where it
must, follows the Polyvoice rule, and every script the GPU tests run on the engine gives a reference
that meets the condition those tests state (finite everywhere, both channels non-zero for every
instrument)."""
import numpy as np
import pytest

import oracle as O
import synth_ref as SR
from helpers import bits_equal, first_mismatch, voice_configs


@pytest.fixture(scope="module", autouse=True)
def rcp():
    SR.install_rcp()
    yield
    SR.remove_rcp()


def test_one_voice_dry_rack_is_the_voice_through_filterfx():
    """P = 1, the delay's and the reverb's balance 0: the instrument is its voice (0.0f + v) through
    FilterFx<2> alone -- the Svf on channel 0, channel 1 in place."""
    n, frames = 5, 700
    rng = np.random.default_rng(3)
    p = SR.params(n, 5)
    p[:SR.NV] = voice_configs(rng, n)
    p[SR.NV + O.FR_FIELDS.index("delay_balance")] = 0.0
    p[SR.NV + O.FR_FIELDS.index("reverb_balance")] = 0.0
    p[SR.NV + O.FR_FIELDS.index("filter_cutoff")] = 20000.0       # wide open
    p[SR.NV + O.FR_FIELDS.index("filter_resonance")] = 0.0
    s = SR.Synth(n, voices=1)
    s.set_params(p)
    voice = O.Voice(n, moog=True, kernel_arith=True)
    filt = O.FxRack(n)
    for i in range(n):
        voice.config(i, p[:SR.NV, i])
        for f in range(SR.NR):
            filt.set(i, f, float(p[SR.NV + f, i]))
        filt.set(i, "topology", 4.0)                               # FilterFx<2> alone
        s.event(i, SR.EV_NOTE_ON, 50 + i)
        voice.event(i, SR.EV_NOTE_ON, 50 + i)
    y = s.process(frames)
    mono = (np.float32(0.0) + voice.process(frames)[0]).astype(np.float32)
    yr = filt.process(np.stack([mono, mono]))
    SR.condition(y)
    assert bits_equal(y, yr), first_mismatch(y, yr)


def test_note_order_decides_the_voice_and_the_sum_order():
    """Two instruments with the same parameters and the same three notes in opposite order: the rule
    gives each note another voice, so the voices are each other's mirror and the sums add them in
    another order."""
    n, frames = 2, 1500
    p = SR.params(n, 6)
    p[:, 1] = p[:, 0]
    s = SR.Synth(n, voices=4)
    s.set_params(p)
    for note in (48, 64, 79):
        s.event(0, SR.EV_NOTE_ON, note)
    for note in (79, 64, 48):
        s.event(1, SR.EV_NOTE_ON, note)
    assert s.playing.tolist() == [[48, 64, 79, 0], [79, 64, 48, 0]]
    s.event(0, SR.EV_NOTE_OFF, 64)
    s.event(1, SR.EV_NOTE_OFF, 64)
    s.event(0, SR.EV_NOTE_ON, 72)                                  # the freed voice 1, not voice 3
    s.event(1, SR.EV_NOTE_ON, 72)
    assert s.playing.tolist() == [[48, 72, 79, 0], [79, 72, 48, 0]]
    s.event(0, SR.EV_SET_FREQUENCY, 0)                             # a nop
    s.event(0, SR.EV_NOTE_ON, 50)
    s.event(0, SR.EV_NOTE_ON, 51)                                  # no voice free: dropped
    s.event(1, SR.EV_NOTE_ON, 50)
    assert s.playing.tolist() == [[48, 72, 79, 50], [79, 72, 48, 50]]
    v = s.voice.process(frames)                                    # [1][frames][4 n], voice p n + i
    for pa, pb in ((0, 2), (1, 1), (2, 0), (3, 3)):
        assert bits_equal(v[0][:, pa * n + 0], v[0][:, pb * n + 1])
    # instrument 1's sum is instrument 0's voices added in the order 2, 1, 0, 3
    m = O.mix_ref(v, s.buses)
    m_rev = O.mix_ref(v, [[2 * n, 1 * n, 0 * n, 3 * n]])
    assert bits_equal(m[:, 1], m_rev[:, 0])
    assert np.any(m[:, 0].view(np.uint32) != m[:, 1].view(np.uint32))


@pytest.mark.parametrize("name", sorted(SR.GPU_SCRIPTS))
def test_gpu_scripts_meet_their_condition(name):
    """The reference of every script tests/test_gpu_synth.py runs: finite for every instrument, both
    channels non-zero for every instrument (a draw that fails here gets another seed here)."""
    script, n, voices = SR.GPU_SCRIPTS[name]()
    yr, _ = SR.run_ref(script, n, voices, threads=8)
    SR.condition(yr)
