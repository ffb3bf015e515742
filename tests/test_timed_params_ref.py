"""The references of tests/timed_param_cases.py alone, on the CPU: every case that tests/test_gpu_timed_params.py
runs against the oracle gives a reference in which its timed change matters -- identical to the same case without
the timed records before the first changed frame, different after it for every changed voice that sounds -- and
the extended split-oracle driver agrees with timed_cases' own where a parameter time is a call boundary.  A condition
that fails here means the case builder is wrong, not the bar."""
import numpy as np
import pytest

import synth_ref as SYN
import timed_cases as C
import timed_param_cases as P
from helpers import first_mismatch, same_bits_or_nan


@pytest.fixture(scope="module", autouse=True)
def rcp():
    SYN.install_rcp()
    yield
    SYN.remove_rcp()


@pytest.mark.parametrize("kind", P.KINDS)
def test_every_timed_change_matters(kind):
    cases = P.cases(kind)
    assert set(cases) == set(P.CASE_NAMES) - ({"portamento_in_glide"} if kind == "voice_sample" else set())
    for name, case in cases.items():
        s, calls = case[0], case[1]
        yr = P.split_oracle(C.reference(s), calls)
        y0 = P.split_oracle(C.reference(s), P.without_params(calls))
        P.condition(name, case, yr, y0)


def test_the_cases_are_what_they_say():
    cases = P.cases("voice")
    sweep = cases["cutoff_sweep"][1][0][3]
    assert sorted({f for f, _ in sweep}) == list(range(0, 64, 4)) and len(sweep) == 16 * P.N
    s = cases["configured_by_a_timed_record"][0]
    assert s.configured == list(range(0, P.N, 2))
    on = cases["change_with_note_on"][1][0]
    assert {ev[0] for ev in on[1]} == {24} == {f for f, _ in on[3]}
    corners = cases["fp32_corners"][1][0][3]
    assert sorted({f for f, _ in corners}) == [4, 12]
    assert set(np.unique(np.stack([op[2] for _, op in corners]))) == {0.0, 1.0, 20000.0}
    assert cases["resonance_and_drive"][4] == [] and P.cases("voice_moog")["resonance_and_drive"][4] == list(range(1, P.N, 2))


@pytest.mark.parametrize("kind", P.KINDS)
def test_driver_agrees_with_boundary_work(kind):
    """A column at frame 16 of a 64-frame call is timed_cases' boundary work of a call that starts there."""
    s, calls = P.cases(kind)["configured_by_a_timed_record"][:2]
    untimed, _, _, tp, _ = calls[0]
    assert {f for f, _ in tp} == {16}
    y = P.split_oracle(C.reference(s), calls)
    want = C.split_oracle(C.reference(s), [(untimed, [], [], 16), ([], [], [op for _, op in tp], 48), ([], [], [], 64)])
    assert same_bits_or_nan(y, want), first_mismatch(y, want)
    # carried over: queued a call earlier at frame 64 + 16, it lands where the next call's own record at 16 does
    early = [(untimed, [], [], [(80, op) for _, op in tp], 64), ([], [], [], [], 64)]
    late = [(untimed, [], [], [], 64), ([], [], [], tp, 64)]
    y1, y2 = P.split_oracle(C.reference(s), early), P.split_oracle(C.reference(s), late)
    assert same_bits_or_nan(y1, y2), first_mismatch(y1, y2)
    assert not same_bits_or_nan(y1, y)
