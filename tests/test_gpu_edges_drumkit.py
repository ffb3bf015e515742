"""GPU edges of drumkit_block_v1, the fused kinds' questions of tests/test_gpu_edges_synth_svf.py put to
OLFX_KIND_DRUMKIT at both rack topologies: every parameter corner (each voice slot's own, the rack's with its
live master volume), one float written outside `out`, a sample-rate constant left at 48000.  The cases, their
references and the condition each reference must meet are tests/drumkit_edge_cases.py (held on the CPU by
tests/test_drumkit_edge_ref.py); every test here asserts that condition again before it compares, bit-exact, and
prints the shares (pytest -s).

The kind has no audio input and its setters refuse non-finite values, so it has no signal and no poison case."""
import pytest

import drumkit_edge_cases as C
import drumkit_ref as DK
import ol_dsp_amd as ofx
from helpers import first_mismatch
from test_gpu_drumkit import apply, run_engine
from test_gpu_edges_fused import _contained_calls

pytestmark = pytest.mark.gpu


def _check_k(y, yr):
    assert DK.bits_equal(y, yr), first_mismatch(y, yr)


@pytest.mark.parametrize("n,P", C.CORNER_SHAPES)
def test_half_corners(cuda, rcp_table, n, P):
    """130 kits of 4 voices and 70 of 8, topology i % 2: each field of each slot at its corner with probability
    1/2, else at an interior value; 1,024 ragged frames, a NoteOff of each kit's voice 0, 1,024 more.  Bit-exact,
    and Engine.playing equals the reference's table after both event steps."""
    script = C.corner_script(n, P)
    yr, ref = DK.run_ref(script, n, P, threads=8)
    C.corner_condition(n, P, yr, script[0][1][DK.TOPOLOGY])
    y, _ = run_engine(script, n, P, cuda, trace=ref.trace)
    _check_k(y, yr)


@pytest.mark.parametrize("n,P", C.CONTAIN_SHAPES)
@pytest.mark.parametrize("host", [False, True])
def test_buffers_contained(cuda, rcp_table, n, P, host):
    """_contained_calls with in = None and guards around the two output planes, 16-byte aligned and one float
    off, device and host buffers."""
    script = C.contain_script(n, P)
    yr, ref = DK.run_ref(script, n, P, threads=8)
    C.contain_condition(yr, ref)
    for offset in (0, 1):
        e = ofx.Engine("drumkit", n, voices=P)
        for step in script[:5]:
            apply(e, step, P)
        y = _contained_calls(e, None, n, offset, cuda, host)
        assert e.kernel_name == "drumkit_block_v1"
        _check_k(y, yr)


@pytest.mark.parametrize("sr", C.RATES)
def test_at_other_sample_rates(cuda, rcp_table, sr):
    """44.1 and 96 kHz, 33 kits of 4 voices on the ragged_frames script: the reference meets the scripts'
    condition and is not the 48 kHz one; bit-exact."""
    script, n = C.rate_script(), C.RATE_N
    yr, ref = DK.run_ref(script, n, 4, threads=8, sample_rate=sr)
    C.rate_condition(yr, ref, DK.run_ref(script, n, 4, threads=8)[0])
    y, _ = run_engine(script, n, 4, cuda, e=ofx.Engine("drumkit", n, voices=4, sample_rate=sr))
    _check_k(y, yr)
