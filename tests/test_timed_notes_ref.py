"""tests/timed_note_cases.py anchored on the CPU: the driver resolves a timed script by the rule include/olfx.h
states, and every case the GPU tests run gives a reference that meets the condition those tests state -- finite
everywhere, both channels non-zero for every instrument (channel 0 alone at topology 0) -- with the expected
Playing() tables.  The same for tests/timed_note_paths.py (the cases of tests/test_gpu_timed_note_paths.py): each
reference meets its case's condition, and what a case is meant to contain -- the score's facts, the capacity case's
record counts, the kit bank's coverage, the launches -- is counted from its script."""
import numpy as np
import pytest

import drumkit_ref as DK
import synth_ref as SR
import timed_note_cases as C
import timed_note_paths as T

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


# ------------------------------------------------------------------------------- tests/timed_note_paths.py
def same_bits(y, yr):
    return y.shape == yr.shape and np.array_equal(y.view(np.uint32), yr.view(np.uint32))


@pytest.mark.parametrize("n,P", T.SCORE_SHAPES + [(65, 4)])
@pytest.mark.parametrize("kind", C.KINDS)
def test_score_facts_and_reference(kind, n, P):
    """The score contains what it is meant to contain, its reference meets the condition, and the same absolute
    times cut into other calls give the reference the same bits and the same final Playing()."""
    s = T.score(kind, n, P)
    assert [b[1] for b in T.steps_of(s, "block")] == T.SCORE_FRAMES + [T.SCORE_TAIL]
    want = {ON, OFF} | (set() if kind == "drumkit" else {C.GATE_ON, C.GATE_OFF})
    assert {ev[2] for st in T.steps_of(s, "timed") for ev in st[1]} == want
    assert not T.steps_of(s, "timed")[-1][1] and T.schedule(s)[-1][1] == {}         # the 8-frame call, the event-free one
    facts = T.score_facts(s, n)
    print(f"\n{kind} n={n} P={P} score facts: {facts}; launches {C.launches(s)}")
    for name, count in facts.items():
        assert count >= 1, name
    yr, ref = T.run_reference(kind, s, n, P)
    assert yr.shape == (2, T.SCORE_TOTAL, n) and len(ref.trace) == len(T.SCORE_FRAMES) + 1
    C.condition(kind, yr, ref)
    for lengths in T.RECUTS:
        again = T.recut(s, lengths)
        assert len(C.launches(again)[0]) >= (4 if len(lengths) == 1 else 1)
        y2, ref2 = T.run_reference(kind, again, n, P)
        assert same_bits(y2, yr), lengths
        assert np.array_equal(ref2.trace[-1], ref.trace[-1])


@pytest.mark.parametrize("kind", C.KINDS)
def test_capacity_case(kind):
    """4 and 5 records in a full group, 4, 5 and 6 in the ragged last one, 63 in a full one -- counted from the
    script -- and every released note is retaken by the voice that held it."""
    s = T.case_capacity(kind)
    counts = T.capacity_counts(kind, s)
    assert counts == T.CAPACITY_COUNTS
    assert {c for at in counts.values() for c in at.values()} == {4, 5, 6, 63} and T.VEV_CAP == 4
    assert C.launches(s) == [[9], [1]]
    timed = T.steps_of(s, "timed")[0][1]
    assert 69 in {ev[1] for ev in timed if ev[0] == 12} and 12 % T.CHUNK
    yr, ref = T.run_reference(kind, s, T.CAPACITY_N, T.CAPACITY_P)
    C.condition(kind, yr, ref)
    assert np.array_equal(ref.trace[1], ref.trace[0]) and np.all(np.asarray(ref.trace[0]) != 0)
    # the releases are audible: without the timed notes the first call differs
    plain, _ = T.run_reference(kind, [st for st in s if st[0] != "timed"], T.CAPACITY_N, T.CAPACITY_P)
    assert same_bits(plain[:, :4], yr[:, :4]) and not same_bits(plain[:, 4:64], yr[:, 4:64])


@pytest.mark.parametrize("n,P", T.KIT_BANK_SHAPES)
def test_kit_bank_case(n, P):
    """Every (sample length, loop configuration) pair that assignments() makes, and every FORCED loop length, gets a
    timed NoteOn at a frame off the chunk grid; some one-shot has ended and some voice is inside its loop when the
    first retrigger comes; the reference meets drumkit_ref.condition."""
    s = T.case_kit_bank(n, P)
    made, got, forced, ended, looping = T.kit_bank_coverage(s, n, P)
    assert got == made and {L for L, _ in made} == set(DK.LENGTHS)
    assert {m for _, m in made} >= {tuple(m) for L in DK.LENGTHS[3:] for m in DK.loop_modes(L)[:2]}
    assert len({(m[0], (m[1] > 0) + (m[2] > 0)) for _, m in made}) >= 4
    assert forced == set(DK.FORCED) and ended and looping
    assert sorted({ev[0] for ev in T.steps_of(s, "timed")[0][1]}) == T.KIT_BANK_FRAMES
    assert C.launches(s) == [[1], [4], [4], [1], [1]]
    yr, ref = T.run_reference("drumkit", s, n, P)
    C.condition("drumkit", yr, ref)
    # the retriggers are audible: the same script without them differs from the first one on
    plain, _ = T.run_reference("drumkit", [st for st in s if st[0] != "timed"], n, P)
    at = T.KIT_BANK_FIRST + 4
    assert same_bits(plain[:, :at], yr[:, :at]) and not same_bits(plain[:, at:], yr[:, at:])


@pytest.mark.parametrize("kind", C.KINDS)
def test_corner_case(kind):
    """The corner scripts with their notes timed meet each suite's own corner condition; nothing sounds ahead of
    the first NoteOn's frame."""
    s = T.case_corners(kind)
    on, off = T.steps_of(s, "timed")
    assert sorted({ev[0] for ev in on[1]}) == [4, 12] and sorted({ev[0] for ev in off[1]}) == [4 + 8, 4 + 100 - 4]
    assert C.launches(s) == [[3], [1], [3], [1], [1]]
    yr, ref = T.run_reference(kind, s, T.CORNER_N, T.CORNER_P)
    assert yr.shape == (2, 1024, T.CORNER_N) and not yr[0, :4].any()
    T.corner_condition(kind, s, yr)
    assert len(ref.trace) == 2 and not np.array_equal(ref.trace[0], ref.trace[1])


@pytest.mark.parametrize("kind", C.KINDS)
def test_engine_path_cases(kind):
    """The slot-ring case is 17 launches of 16 segments; the coefficient case's set and control change the
    reference of the calls after them and nothing before; both references meet the condition."""
    n, P = 65, 4
    s = T.case_ring(kind, n, P)
    assert len(C.launches(s)[0]) == T.KSLOTS + 1
    timed = T.steps_of(s, "timed")[0][1]
    assert {ev[1] for ev in timed} == set(C.few(n)) and sorted({ev[0] for ev in timed}) == list(range(0, T.RING_FRAMES, 4))
    yr, ref = T.run_reference(kind, s, n, P)
    C.condition(kind, yr, ref)
    s = T.case_coefs(kind, n, P)
    yr, ref = T.run_reference(kind, s, n, P)
    C.condition(kind, yr, ref)
    plain, _ = T.run_reference(kind, [st for st in s if st[0] not in ("set", "control")], n, P)
    assert same_bits(plain[:, :128], yr[:, :128])
    for who in (slice(0, n, 2), slice(1, n, 2)):                 # the set's instruments, the control's
        assert not same_bits(plain[:, 128:, who], yr[:, 128:, who])
    if kind != "drumkit":
        lowered = T.lower_controls(kind, s)
        assert not T.steps_of(lowered, "control") and len(T.steps_of(lowered, "set")) > len(T.steps_of(s, "set"))


def test_scale_case_shape():
    for n, P in T.SCALE_SHAPES:
        s = T.case_scale("synth", n, P)
        at = T.schedule(s)[0][1]
        assert sorted(at) == [4, 12, 60] and len(at[12]) == n and len(at[4]) == len(at[60]) < n // 20
        who = T.sampled(n)
        assert who[0] == 0 and who[-1] == n - 1 and 60 <= len(who) <= 70
