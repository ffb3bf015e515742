"""tests/timed_note_cases.py anchored on the CPU: the driver resolves a timed script by the rule include/olfx.h
states, and every case the GPU tests run gives a reference that meets the condition those tests state -- finite
everywhere, both channels non-zero for every instrument (channel 0 alone at topology 0) -- with the expected
Playing() tables."""
import numpy as np
import pytest

import synth_ref as SR
import timed_note_cases as C

ON, OFF = C.NOTE_ON, C.NOTE_OFF
CASES = C.cases()


@pytest.fixture(scope="module", autouse=True)
def rcp():
    SR.install_rcp()
    yield
    SR.remove_rcp()


def test_resolve_restates_the_rule():
    """Frame 0 at the call; (frame, queueing order) across calls; a note at the call's end as it returns, ahead of
    the next untimed one; a note past it carried with its frame reduced."""
    s = [("timed", [(8, 0, ON, 60), (0, 1, ON, 61), (64, 2, OFF, 62), (8, 3, ON, 63)]), ("events", [(4, ON, 64)]),
         ("timed", [(4, 5, ON, 65), (8, 6, ON, 66), (136, 7, ON, 67)]), ("block", 64), ("events", [(8, ON, 68)]),
         ("block", 64), ("check_playing",), ("block", 64)]
    assert C.resolve(s) == [
        ("events", [(1, ON, 61)]), ("events", [(4, ON, 64)]), ("block", 4), ("events", [(5, ON, 65)]), ("block", 4),
        ("events", [(0, ON, 60), (3, ON, 63), (6, ON, 66)]), ("block", 56), ("events", [(2, OFF, 62)]),
        ("events", [(8, ON, 68)]), ("block", 64), ("check_playing",), ("block", 8), ("events", [(7, ON, 67)]), ("block", 56)]
    assert C.launches(s) == [[3], [1], [2]]


def test_case_shapes():
    """What the cases are meant to contain: the six event frames, the crowded groups, the launches."""
    kind, s, n, P = CASES["synth-sparse-P4"]
    timed = next(step[1] for step in s if step[0] == "timed")
    assert sorted({ev[0] for ev in timed}) == C.FRAMES and C.launches(s) == [[7], [1]]
    assert max(sum(1 for f, i, _, _ in timed if f == 4 and i // 64 == g) for g in range(2)) <= 4
    kind, s, n, P = CASES["drumkit-all_on-P8"]
    timed = next(step[1] for step in s if step[0] == "timed")
    assert sum(1 for ev in timed if ev[0] == 12) == n * P and C.launches(s) == [[4], [1]]
    assert C.launches(CASES["synth_svf-seventeen"][1]) == [[16, 1], [1]]
    assert C.launches(CASES["drumkit-carry"][1]) == [[1], [1], [3], [1]]


@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_meets_the_condition(name):
    kind, script, n, P = CASES[name]
    yr, ref = C.run_reference(kind, script, n, P)
    assert yr.shape == (2, sum(s[1] for s in script if s[0] == "block"), n)
    C.condition(kind, yr, ref)
    assert len(ref.trace) == sum(1 for s in script if s[0] == "check_playing") >= 1
    tr = [np.asarray(t) for t in ref.trace]
    note = C.note_of(kind, n, P)
    case = name.split("-")[1]
    if case == "allocation":
        for t, want in zip(tr, C.ALLOCATION_PLAYING):
            assert np.array_equal(t, np.tile(want, (n, 1)))
    elif case == "carry" and kind != "drumkit":
        # released as call 1 returned; the untimed NoteOn found that voice; the last voice retaken in call 3
        assert not tr[0][:, 0].any() and np.all(tr[1][:, 0] == 82) and np.all(tr[2][:, 0] == 82)
        assert np.all(tr[3][:, P - 1] == 81)
    elif case == "carry":
        assert all(tr[0][i, 0] == note(i, 0) for i in range(n)) and not tr[1][:, 0].any()
        assert all(tr[3][i, P - 1] == note(i, P - 1) for i in range(n))
    elif case == "map_change":
        # the note pending at the map change reached voice 1 of the even kits and nobody in the odd ones
        assert np.array_equal(tr[1][1::2], tr[0][1::2])
        assert all(tr[1][i, 1] == note(i, 0) for i in range(0, n, 2))
    elif case == "sparse" and kind != "drumkit":
        w = C.few(n)
        assert np.all(tr[0][w, 0] == 74)             # 72 took voice 0 at 12, left it at 36; 74 took it at 60
