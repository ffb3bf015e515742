"""olfx_timed_instrument_params / olfx_timed_instrument_control on the CPU: every case of
tests/timed_instrument_param_cases.py through the composed references (synth_ref, synth_svf_ref, drumkit_ref) as the
split steps its driver resolves it into.  Each reference meets the condition the GPU tests state, and each timed
change is audible: for every record time of a case, the reference without that time's records is the same before
that frame and differs from it on, for every instrument the records change.  The driver's rule is held to
timed_note_cases.resolve on the note-only cases, and its launch model to the cases' own expectations."""
import numpy as np
import pytest

import timed_instrument_param_cases as T
import timed_note_cases as C

CASES = T.cases(65)


@pytest.fixture(scope="module")
def rcp():
    T.SR.install_rcp()
    yield
    T.SR.remove_rcp()


_REF = {}


def reference(name):
    """A case's reference, computed once and left unchanged."""
    if name not in _REF:
        kind, script, n, voices = CASES[name]
        _REF[name] = T.run_reference(kind, script, n, voices, threads=8)
    return _REF[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_condition_and_audible_changes(rcp, name):
    kind, script, n, voices = CASES[name]
    yr, ref = reference(name)
    C.condition(kind, yr, ref)
    times = T.changes(script, kind, voices)
    assert times
    for t, arrivals, who in times:
        yo, _ = T.run_reference(kind, T.without(script, arrivals), n, voices, threads=8)
        assert yo.shape == yr.shape and t < yr.shape[1]
        assert np.array_equal(yo[:, :t].view(np.uint32), yr[:, :t].view(np.uint32)), (t, "differs before its frame")
        same = [i for i in who if np.array_equal(yo[:, t:, i].view(np.uint32), yr[:, t:, i].view(np.uint32))]
        assert not same, (t, "inaudible on", same[:8])


def test_ignored_controls_change_nothing(rcp):
    """CC_IGNORED and a kit's control on a channel nobody sits at: the reference with them is the one without."""
    for kind in T.KINDS:
        _, script, n, voices = CASES[f"{kind}-controls"]
        counted = {a for _, arr, _ in T.changes(script, kind, voices) for a in arr}
        total = sum(len(step[1]) for step in script if step[0] in T.RECORD_STEPS)
        ignored = set(range(total)) - counted
        assert ignored
        yo, _ = T.run_reference(kind, T.without(script, ignored), n, voices, threads=8)
        yr, _ = reference(f"{kind}-controls")
        assert np.array_equal(yo.view(np.uint32), yr.view(np.uint32))


def test_driver_agrees_with_the_note_driver():
    """The combined rule on note-only scripts (a record step that holds nothing forces it) is timed_note_cases.resolve's."""
    for name, (kind, script, n, voices) in C.cases(9).items():
        mine = T.resolve(script + [("tparams", [])])
        theirs = C.resolve(script)
        assert len(mine) == len(theirs), name
        for a, b in zip(mine, theirs):
            assert a[0] == b[0] and (a[0] in ("params", "bank") or a[1:] == b[1:]), (name, a[0])


def test_resolve_orders_records_ahead_of_notes():
    s = [("timed", [(8, 0, 1, 60), (64, 1, 1, 61)]), ("tparams", [(8, 0, 3, 0.5), (0, 2, 3, 0.25)]),
         ("tcontrol", [(8, 1, 41, 64.0, "midi", 0), (64, 0, 42, 10.0, "hw", 0)]), ("block", 64), ("block", 64)]
    assert T.resolve(s) == [("set", 2, 3, 0.25), ("block", 8), ("set", 0, 3, 0.5), ("control", [(1, 41, 64.0, "midi", 0)]),
                            ("events", [(0, 1, 60)]), ("block", 56), ("control", [(0, 42, 10.0, "hw", 0)]), ("events", [(1, 1, 61)]),
                            ("block", 64)]


def test_launch_model():
    """The cases' launches as the host core cuts them (tests/cpp/test_timed_instrument_params_host.cpp pins the core)."""
    for kind in T.KINDS:
        assert T.launches(T.case_boundary(kind, 65, 4), 65, 4, kind)[0] == [12, 8, 16, 28]
        assert T.launches(T.case_seventeen(kind, 65, 4), 65, 4, kind) == [[64, 64], [64]]
        assert T.launches(T.case_frames(kind, 65, 4), 65, 4, kind) == [[64], [64]]
        cap = T.launches(T.case_record_cap(kind, 65, 4), 65, 4, kind)[0]
        assert cap == [24, 40], cap
