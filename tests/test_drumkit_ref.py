"""The drum kit's composed CPU reference (tests/drumkit_ref.py) by itself: every script the GPU tests run meets
the condition they state, and the composition has the properties the kind is defined by."""
import numpy as np
import pytest

import drumkit_ref as DK
from ol_dsp_amd import workload


@pytest.fixture(scope="module", autouse=True)
def rcp():
    DK.install_rcp()
    yield
    DK.remove_rcp()


@pytest.mark.parametrize("name", sorted(DK.GPU_SCRIPTS))
def test_gpu_scripts_meet_the_condition(name):
    script, n, P = DK.GPU_SCRIPTS[name]()
    yr, ref = DK.run_ref(script, n, P)
    DK.condition(yr, ref)
    assert ref.sounding.any()
    if name == "sum_order":
        # the figures the script was chosen for
        orders = ref.log[0][2]
        assert sum(o != sorted(o) for o in orders) == 67
        _, first = DK.run_ref(script[:6], n, P)
        assert np.all(np.any(first.last_voices[0] != 0, axis=0))         # all 350 voices sound
        by_note, by_slot = ref.log[0][3], ref.log[0][4]
        differ = (by_note.view(np.uint32) != by_slot.view(np.uint32)).sum(0)
        assert all(differ[i] >= 24 for i, o in enumerate(orders) if o != sorted(o))
        topo0 = ref.p[DK.TOPOLOGY] == 0.0
        assert int(topo0.sum()) == 37 and not yr[1][:, topo0].any() and yr[1][:, ~topo0].any(axis=0).all()


def test_condition_rejects_an_indistinguishable_order():
    """Voices 1 and 0 swapped sum to the slot order's bits (float addition commutes): condition() says so."""
    n, P = 2, 2
    s = DK.script_sum_order(n, P)
    s[3] = ("map", [(i, p, 40 - p, p) for i in range(n) for p in range(P)])
    s[4] = ("events", [(i, DK.EV_NOTE_ON, 40 - p) for i in range(n) for p in range(P)])
    yr, ref = DK.run_ref(s, n, P)
    with pytest.raises(AssertionError, match="indistinguishable"):
        DK.condition(yr, ref)


def test_one_voices_config_changes_its_kit_only():
    script, n, P = DK.GPU_SCRIPTS["sum_order"]()
    script = script[:6]
    y0, _ = DK.run_ref(script, n, P)
    changed = script[:5] + [("set", 7, 2 * DK.NV + 9, 0.05)] + script[5:]       # slot 2's amp_env_amount of kit 7
    y1, _ = DK.run_ref(changed, n, P)
    differs = np.any(y0.view(np.uint32) != y1.view(np.uint32), axis=(0, 1))
    assert differs[7] and differs.sum() == 1


def test_an_unmapped_voice_does_not_sound_but_ticks():
    script, n, P = DK.GPU_SCRIPTS["sum_order"]()
    base = script[:5]
    # voice 3 of kit 9 triggered, then unmapped before the block: kit 9 sums its other voices only
    unmapped = base + [("map", [(9, None, DK.note_of(9, 3), None)]), ("block", 256)]
    y, ref = DK.run_ref(unmapped, n, P)
    assert 3 not in ref.order(9) and ref.last_voices[0][:, 3 * n + 9].any()     # it ticks on, unheard
    never = base[:3] + [("map", [r for r in base[3][1] if (r[0], r[3]) != (9, 3)]), base[4], ("block", 256)]
    y2, ref2 = DK.run_ref(never, n, P)
    assert not ref2.last_voices[0][:, 3 * n + 9].any()                          # the NoteOn reached nobody
    assert DK.bits_equal(y, y2)
    full, _ = DK.run_ref(base + [("block", 256)], n, P)
    assert np.any(full[:, :, 9] != y[:, :, 9]) and DK.bits_equal(np.delete(full, 9, 2), np.delete(y, 9, 2))


@pytest.mark.parametrize("n,P", [(1, 1), (1, 4), (33, 1), (33, 2), (65, 4), (65, 5), (130, 8)])
def test_forced_loops_cover_the_edge_kits(n, P):
    """Where each forced loop length of assignments() lands: all eight at n P >= 8, one voice each, on the
    outermost kits, and the assignment records say so."""
    placed = DK.forced_loops(n, P)
    assert [m for _, _, m in placed] == DK.FORCED[:min(8, n * P)]
    recs = {(r[0], r[1]): r for r in DK.assignments(n, P)}
    for kit, p, m in placed:
        _, _, sample, mode, ls, le = recs[(kit, p)]
        assert (sample, mode, le - ls + 1) == (11, 1, m) and ls % 2 == 1       # odd cursors of the 1000-frame sample
    if n > 1 and P >= 4:
        assert sum(k == 0 for k, _, _ in placed) == sum(k == n - 1 for k, _, _ in placed) == 4
