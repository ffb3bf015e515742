"""The drum kit's edge cases (tests/drumkit_edge_cases.py) on the CPU: every reference the GPU edge tests compare
with meets the condition its case states."""
import pytest

import drumkit_edge_cases as C
import drumkit_ref as DK


@pytest.fixture(scope="module", autouse=True)
def rcp():
    DK.install_rcp()
    yield
    DK.remove_rcp()


@pytest.mark.parametrize("n,P", C.CORNER_SHAPES)
def test_half_corners(n, P):
    script = C.corner_script(n, P)
    yr, ref = DK.run_ref(script, n, P)
    C.corner_condition(n, P, yr, script[0][1][DK.TOPOLOGY])
    assert len(ref.trace) == 2 and yr.shape == (2, 2048, n)


@pytest.mark.parametrize("n,P", C.CONTAIN_SHAPES)
def test_containment_runs(n, P):
    yr, ref = DK.run_ref(C.contain_script(n, P), n, P)
    C.contain_condition(yr, ref)


@pytest.mark.parametrize("sr", C.RATES)
def test_other_sample_rates(sr):
    script, n = C.rate_script(), C.RATE_N
    yr, ref = DK.run_ref(script, n, 4, sample_rate=sr)
    C.rate_condition(yr, ref, DK.run_ref(script, n, 4)[0])
