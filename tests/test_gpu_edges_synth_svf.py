"""GPU edges of synth_svf_block_v1, the synth's questions of tests/test_gpu_edges_fused.py put to
OLFX_KIND_SYNTH_SVF at both rack topologies: every parameter corner (the voice's with its live filter
drive, the rack's with its live master volume), one float written outside `out` (the zero channel of
topology 0 is a store like any other), a sample-rate constant left at 48000.  The cases, their references
and the condition each reference must meet are tests/synth_svf_edge_cases.py (held on the CPU by
tests/test_synth_svf_edge_ref.py); every test here asserts that condition again before it compares,
bit-exact with synth_ref.bits_equal, and prints the shares (pytest -s).

The kind has no audio input and its setters refuse non-finite values, so it has no signal and no poison
case."""
import pytest

import ol_dsp_amd as ofx
import synth_svf_edge_cases as C
import synth_svf_ref as SV
from helpers import first_mismatch
from test_gpu_edges_fused import _contained_calls
from test_gpu_synth_svf import run_engine

pytestmark = pytest.mark.gpu


def _check_k(y, yr):
    assert SV.bits_equal(y, yr), first_mismatch(y, yr)


@pytest.mark.parametrize("n,P", C.CORNER_SHAPES)
def test_half_corners(cuda, rcp_table, n, P):
    """256 instruments of 4 voices and 70 of 8, topology i % 2: each field at its corner with probability
    1/2, else at an interior value; notes from the ends and the middle of the MIDI range on every voice,
    1,024 ragged frames, a NoteOff of each instrument's first note, 1,024 more.  Bit-exact, and
    Engine.playing equals the rule's table after both event steps."""
    script = C.corner_script(n, P)
    yr, ref = SV.run_ref(script, n, P, threads=8)
    C.corner_condition(n, P, yr, script[0][1][SV.TOPOLOGY])
    y, _ = run_engine(script, n, P, cuda, trace=ref.trace)
    _check_k(y, yr)


@pytest.mark.parametrize("n,P", C.CONTAIN_SHAPES)
@pytest.mark.parametrize("host", [False, True])
def test_buffers_contained(cuda, rcp_table, n, P, host):
    """_contained_calls with in = None and guards around the two output planes, 16-byte aligned and one
    float off, device and host buffers."""
    script = C.contain_script(n, P)
    yr, ref = SV.run_ref(script, n, P, threads=8)
    C.contain_condition(yr, ref)
    for offset in (0, 1):
        e = ofx.Engine("synth_svf", n, voices=P)
        e.set_params(0, script[0][1])
        e.note_events(script[1][1])
        y = _contained_calls(e, None, n, offset, cuda, host)
        assert e.kernel_name == "synth_svf_block_v1"
        _check_k(y, yr)


@pytest.mark.parametrize("sr", C.RATES)
def test_at_other_sample_rates(cuda, rcp_table, sr):
    """44.1 and 96 kHz, 33 instruments of 4 voices on the ragged_frames script: the reference meets the
    scripts' condition and is not the 48 kHz one; bit-exact."""
    script, n = C.rate_script(), C.RATE_N
    yr, ref = SV.run_ref(script, n, 4, threads=8, sample_rate=sr)
    C.rate_condition(yr, ref, SV.run_ref(script, n, 4, threads=8)[0])
    y, _ = run_engine(script, n, 4, cuda, e=ofx.Engine("synth_svf", n, voices=4, sample_rate=sr))
    _check_k(y, yr)
