"""tests/meter_ref.py (the level meters' numpy restatement) held to the reference's own ol::core::Rms: the
committed recordings tests/golden/rms_reference_runs.json, a fresh recording wherever the reference tree is
present, and every edge case's condition (tests/meter_cases.py) on the restatement alone.  No GPU."""
import importlib.util
import json
import os

import numpy as np
import pytest

import meter_cases as C
import meter_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load_gen():
    spec = importlib.util.spec_from_file_location("gen_rms_golden", os.path.join(ROOT, "tests", "golden", "gen_rms_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _load_gen()
with open(G.FIXTURE) as _f:
    FIX = json.load(_f)


def same_bits_or_nan(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def fixture_rms(run):
    h = run["rms_bits"]
    return np.array([int(h[8 * k:8 * k + 8], 16) for k in range(run["frames"])], np.uint32).view(np.float32)


def test_fixture_covers_what_it_should():
    assert os.path.getsize(G.FIXTURE) < 100 * 1024
    runs = {r["name"]: r for r in FIX["runs"]}
    assert [r["name"] for r in FIX["runs"]] == [r[0] for r in G.RUNS] and all(r["frames"] <= 600 for r in FIX["runs"])
    assert {runs[k]["sample_rate"] for k in ("default_48k", "default_44k1", "default_96k")} == {48000.0, 44100.0, 96000.0}
    assert {r["window"] for r in FIX["runs"]} >= {0.0, 1.0, 3.0, float(C.W44)}
    assert any(r["init_again"] for r in FIX["runs"]) and runs["scale_2^-70"]["scale"] == 2.0 ** -70
    assert runs["one_nan"]["nan_at"] == 300
    assert [r["sample_rate"] for r in FIX["long_runs"]] == [48000.0, 44100.0, 96000.0]
    assert all(r["frames"] == 70000 for r in FIX["long_runs"])
    # the recordings show what the runs are there for
    assert M.default_window(44100.0) == C.W44 and float(M.default_window(48000.0)) == 128 and float(M.default_window(96000.0)) == 256
    nan = np.isnan(fixture_rms(runs["one_nan"]))
    assert nan[300:384].all() and not nan[:300].any() and not nan[384:].any()
    tiny = fixture_rms(runs["scale_2^-70"])
    assert np.count_nonzero(tiny) >= 594 and tiny.max() < 2.0 ** -70


@pytest.mark.parametrize("run", FIX["runs"], ids=[r["name"] for r in FIX["runs"]])
def test_restatement_equals_the_recorded_rms(run):
    x = G.signal(run["stream"], run["frames"], run["scale"], run["nan_at"])
    y = G.restate(x, run["sample_rate"], run["window"], run["init_again"])
    assert same_bits_or_nan(y, fixture_rms(run))


@pytest.mark.parametrize("run", FIX["long_runs"], ids=[str(int(r["sample_rate"])) for r in FIX["long_runs"]])
def test_restatement_equals_the_recorded_long_run(run):
    y = G.restate(G.signal(run["stream"], run["frames"]), run["sample_rate"], 0.0)
    assert f"{int(y.view(np.uint32)[-1]):08x}" == run["last_bits"]
    assert f"{M.fnv1a64(y):016x}" == run["fnv1a64"]


def test_fresh_recording_equals_the_fixture(tmp_path):
    """Where the reference tree is present: the real class, built now at -O2 and at -O0, gives the committed bits."""
    if not G.have_reference():
        pytest.skip("the reference tree is not on this machine")
    for opt in ("-O2", "-O0"):
        exe = G.build_recorder(str(tmp_path), opt=opt)
        fresh = G.record_all(exe)
        assert [r["rms_bits"] for r in fresh["runs"]] == [r["rms_bits"] for r in FIX["runs"]], opt
        assert [r["fnv1a64"] for r in fresh["long_runs"]] == [r["fnv1a64"] for r in FIX["long_runs"]], opt


def test_modes_leave_the_same_state():
    n = 9
    x = C.noise(n)
    kw = dict(window=C.mixed_windows(n), hold=C.mixed_holds(n))
    env, lv_env = C.reference(n, 2, x, modes=(True,), **kw)
    _, lv_sum = C.reference(n, 2, x, modes=(False,), **kw)
    mixed, lv_alt = C.reference(n, 2, x, modes=(True, False), **kw)
    for a, b, c in zip(lv_env, lv_sum, lv_alt):
        for f in M.FIELDS:
            assert same_bits_or_nan(a[f], b[f]) and same_bits_or_nan(a[f], c[f]), f
    for k in range(0, len(C.CALLS), 2):                  # the alternation's envelope calls
        s = slice(C.STARTS[k], C.STARTS[k + 1])
        assert same_bits_or_nan(mixed[:, s], env[:, s])
    # one call or many: the same stream
    whole, lv = C.reference(n, 2, x, calls=[C.FRAMES], **kw)
    assert same_bits_or_nan(whole, env) and all(same_bits_or_nan(lv[0][f], lv_env[-1][f]) for f in M.FIELDS)
    # the run_schedule form
    ref = M.MeterRef(n, 2)
    ref.set("window", kw["window"])
    ref.set("peak_hold", kw["hold"])
    assert same_bits_or_nan(M.run_schedule(ref, x, C.CALLS, (True,)), env)


def test_window_quirks_and_changes():
    n = 16
    w, changes, up, down = C.window_changes(n)
    assert len(up) and len(down)
    env, levels = C.reference(n, 2, C.noise(n), window=w, changes=changes)
    C.check_window_changes(levels, up, down)
    # a fractional window never matches: the count is the frame count
    frac = np.flatnonzero(w == C.W44)
    assert np.all(levels[-1]["count"][frac] == C.FRAMES)
    # window 1: every frame alone, rms = |x|
    one = np.flatnonzero(w == 1)
    assert np.array_equal(env[:, :, one], np.abs(C.noise(n)[:, :, one]))
    # setting a window resets nothing, and reset() keeps the parameters
    ref = M.MeterRef(2, 1)
    ref.set("window", [64.0, 64.0])
    ref.process(np.ones((1, 40, 2), np.float32))
    ref.set("window", [50.0, 50.0])
    assert np.all(ref.state["count"] == 40) and np.all(ref.state["sum"] == 40)
    ref.reset()
    assert np.all(ref.window == 50) and all(np.all(ref.state[f] == 0) for f in M.FIELDS)
    # other rates' defaults
    for sr, expect in ((44100.0, C.FRAMES), (96000.0, 256)):
        _, lv = C.reference(3, 1, C.noise(3, 1), sample_rate=sr)
        assert np.all(lv[-1]["count"] == expect), sr


def test_peak_hold_expiries():
    C.check_hold_expiries()
    assert C.expiry_frames(5.0)[:3] == [4, 9, 14] and C.expiry_frames(2.5) == [] and C.expiry_frames(-1.0) == []
    n = 16
    x = C.noise(n)
    _, levels = C.reference(n, 2, x, hold=C.mixed_holds(n))
    h = C.mixed_holds(n)
    # after the first call (256 frames) the holds 16 and 256 have just expired: the call's last frame
    for hold in (16, 256):
        i = np.flatnonzero(h == hold)
        assert len(i) and np.all(levels[0]["peak_count"][i] == 0) and np.all(levels[0]["peak"][i] == 0)
    i = np.flatnonzero(h == 96000)
    assert np.all(levels[-1]["peak_count"][i] == C.FRAMES)
    assert np.array_equal(levels[-1]["peak"][i], np.abs(x).max(axis=1).T[i])


@pytest.mark.parametrize("name", C.EDGES)
def test_edge_conditions_hold_on_the_reference(name):
    for n in (70, 72):
        x, _ = C.edge(name, n)
        assert x.shape == (2, C.FRAMES, n) and x.dtype == np.float32
