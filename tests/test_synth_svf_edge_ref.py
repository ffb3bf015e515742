"""The references of tests/synth_svf_edge_cases.py alone, on the CPU: every case that
tests/test_gpu_edges_synth_svf.py runs on the engine gives a reference with the edge the case is about --
the half-corners finite and audible at both topologies with channel 1 silent at topology 0, the
containment runs finite, the other sample rates different from 48 kHz.  A condition that fails here
means the case builder is wrong, not the bound."""
import numpy as np
import pytest

import synth_svf_edge_cases as C
import synth_svf_ref as SV


@pytest.fixture(scope="module", autouse=True)
def rcp():
    SV.install_rcp()
    yield
    SV.remove_rcp()


@pytest.mark.parametrize("n,P", C.CORNER_SHAPES)
def test_half_corners(n, P):
    script = C.corner_script(n, P)
    p = script[0][1]
    at_corner = np.isin(p[:SV.NV + 9], [0.0, 1.0, 20000.0])
    assert 0.4 < at_corner.mean() < 0.6                  # half the fields at an end of their range
    assert np.array_equal(p[SV.TOPOLOGY], np.arange(n) % 2)
    assert {0.0, 1.0} <= set(np.unique(p[SV.MASTER]).tolist())   # the master's corners, live at topology 0
    assert sum(s[1] for s in script if s[0] == "block") == 2048
    yr, ref = SV.run_ref(script, n, P, threads=8)
    assert len(ref.trace) == 2 and np.all(ref.trace[0] != 0) and np.all(ref.trace[1][:, 0] == 0)
    C.corner_condition(n, P, yr, p[SV.TOPOLOGY])


@pytest.mark.parametrize("n,P", C.CONTAIN_SHAPES)
def test_containment_runs_are_finite(n, P):
    yr, ref = SV.run_ref(C.contain_script(n, P), n, P, threads=8)
    C.contain_condition(yr, ref)


@pytest.mark.parametrize("sr", C.RATES)
def test_rates(sr):
    script, n = C.rate_script(), C.RATE_N
    yr, ref = SV.run_ref(script, n, 4, threads=8, sample_rate=sr)
    yr48, _ = SV.run_ref(script, n, 4, threads=8)
    C.rate_condition(yr, ref, yr48)
