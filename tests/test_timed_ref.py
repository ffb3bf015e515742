"""The references of tests/timed_cases.py alone, on the CPU: every case that tests/test_gpu_timed_paths.py
runs against the oracle gives a reference that meets the case's condition, the score contains what it is
meant to contain, and the split-oracle driver's carry-over arithmetic agrees with itself when the same
score is cut into other calls.  A condition that fails here means the case builder is wrong, not the bar."""
import numpy as np
import pytest

import synth_ref as SYN
import timed_cases as C
from helpers import bits_equal, first_mismatch, same_bits_or_nan


@pytest.fixture(scope="module", autouse=True)
def rcp():
    SYN.install_rcp()
    yield
    SYN.remove_rcp()


@pytest.mark.parametrize("kind", C.KINDS)
def test_score(kind):
    s, calls = C.score(kind)
    assert len(calls) == C.SCORE_CALLS and [c[3] for c in calls[:8]] == C.SCORE_FRAMES
    assert {ev[2] for c in calls for ev in c[1]} == {0, 1, 2, 3, 4}            # all five event types, timed
    assert all(ev[0] % 4 == 0 and ev[0] < 2.5 * c[3] for c in calls for ev in c[1])
    assert any(ev[0] >= c[3] for c in calls for ev in c[1])
    assert {op[0] for c in calls for op in c[2]} == {"params", "member"}
    if kind != "voice_sample":
        touched = set(s.configured) | {op[1] for c in calls for op in c[2]}
        assert touched == set(range(0, s.n, 2))                               # the odd voices: Init's defaults
    facts = C.score_facts(calls)
    print(f"\n{kind} score facts: {facts}")
    for name in ("calls_over_the_cap", "single_quad_runs", "carried_two_calls", "crowded_twice", "setfreq_after_noteon"):
        assert facts[name] >= 1, name
    yr = C.split_oracle(C.reference(s), calls)
    assert yr.shape == (1, sum(c[3] for c in calls), s.n)
    C.score_condition(kind, yr)


@pytest.mark.parametrize("kind", C.KINDS)
def test_score_recut(kind):
    """The same absolute event times and the same total in as few calls as the boundary work allows and in
    pieces of at most 16 frames: the driver's output is the same, bit for bit."""
    s, calls = C.score(kind)
    yr = C.split_oracle(C.reference(s), calls)
    for piece in (None, 16):
        lengths = C.recut_lengths(calls, piece)
        again = C.recut(calls, lengths)
        assert len(again) != len(calls) and sum(lengths) == yr.shape[1]
        assert sum(len(c[0]) + len(c[1]) for c in again) == sum(len(c[0]) + len(c[1]) for c in calls)
        y2 = C.split_oracle(C.reference(s), again)
        assert same_bits_or_nan(y2, yr), (piece, first_mismatch(y2, yr))
    assert len(C.recut_lengths(calls)) == 3 and max(C.recut_lengths(calls, 16)) == 16


@pytest.mark.parametrize("kind", C.KINDS)
def test_corners(kind):
    s, calls = C.corner_case(kind)
    assert s.n == 256 and set(np.unique(s.cfg)) == {0.0, 1.0, 20000.0}
    assert sorted({ev[0] for ev in calls[0][1]}) == [12, 20, 36, 40, 44, 48] and not calls[1][1]
    yr = C.split_oracle(C.reference(s), calls)
    assert yr.shape == (1, 128, 256) and not yr[0, :12].any()
    C.corner_condition(kind, yr)


def test_sampler_case():
    s, calls = C.sampler_case()
    yr = C.split_oracle(C.reference(s), calls)
    assert yr.shape == (1, 256, C.SAMPLER_N)
    C.sampler_condition(s, yr)
    # every voice is paused for exactly one quad and replayed from frame 0: its output from its NoteOn on is
    # not what an unbroken run gives
    plain = C.split_oracle(C.reference(s), [([], [ev for ev in calls[0][1] if ev[0] == 0], [], 256)])
    assigned = [r[0] for r in s.recs if r[1] is not None]
    assert not bits_equal(yr[:, 24:, assigned], plain[:, 24:, assigned])
    assert bits_equal(yr[:, :8], plain[:, :8])


def test_launches_restate_the_cap():
    """17 event times past frame 0 in one call are 18 segments: two launches, the second starting at the
    time that did not fit; an event at frame == n_frames is frame 0 of the next call."""
    timed = [(4 * k, 0, C.NOTE_ON, 60, 0.0) for k in range(1, 18)] + [(128, 1, C.NOTE_ON, 60, 0.0)]
    ls = C.launches([([], timed, [], 128), ([], [], [], 4)])
    assert [len(l) for l in ls[0]] == [16, 2] and ls[0][1][0][0] == 64
    assert len(ls[1]) == 1 and ls[1][0][0][0] == 0 and ls[1][0][0][1][0] == ((1, C.NOTE_ON, 60, 0.0), 1)
