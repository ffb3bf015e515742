"""CPU tests: the oracle against the reference's golden vectors and the reference itself.

Dattorro is PINNED: the C restatement must be bit-identical to the real reference
(libs/dattorro-verb/verb.cpp, compiled into oracle/_ref by oracle/Makefile) and to the committed
fixtures it produced.  Chorus / pitch-shift / voice are UNPINNED spec oracles: their fixtures
freeze the restatement, and the voice reproduces the qualitative pins of
test/synth_test.cpp:102-148.
"""
import ctypes

import numpy as np
import pytest

import oracle as O
from helpers import (EDGE_FRAMES, UNIFORM_PD_RUNS, bits_equal, dt_edge_params, dt_reference_cases, fast_noise, first_mismatch,
                     fxrack_params, lr_hashes, noise_block, poison_table, poisoned, rel_err, run_dattorro,
                     subnormal_share)


# ---------------------------------------------------------------- dattorro, vs golden fixtures
def test_dattorro_impulse_kats(golden):
    imp = np.zeros((1, 48000, 1), np.float32)
    imp[0, 0, 0] = 1.0
    y = O.Dattorro(1).process(imp)
    g = golden["dattorro_impulse"]
    for n, (l, r) in g["kat"].items():
        assert np.float32(y[0, int(n), 0]) == np.float32(l), n
        assert np.float32(y[1, int(n), 0]) == np.float32(r), n
    assert f"{O.fnv1a64_lr(y[0, :, 0], y[1, :, 0]):016x}" == g["fnv1a64"]
    first = np.load(__import__("os").path.join(__import__("os").path.dirname(__file__), "golden",
                                                "dattorro_impulse_4096.npy"))
    assert bits_equal(y[:, :4096, 0], first)


def test_dattorro_impulse_matches_survey_values():
    # SURVEY.md section 8c KAT values (measured there with g++ -O2 -ffp-contract=off)
    kat = {1000: (-5.06734239e-07, -2.88859817e-23), 2000: (0.00382412504, -0.00750800269),
           4800: (0.00366625283, 0.0275579803), 12800: (-0.00399901532, 0.00456911325),
           20800: (-0.00629576156, -0.00478657521), 28800: (0.00383224664, -0.00649412163),
           36800: (-0.00555869937, 0.000979059027), 44800: (-0.000748623977, 0.00146027002),
           47999: (-0.0020442456, 0.00166539999)}
    imp = np.zeros((1, 48000, 1), np.float32)
    imp[0, 0, 0] = 1.0
    y = O.Dattorro(1).process(imp)
    for n in (0, 1, 479, 480, 481):
        assert y[0, n, 0] == 0 and y[1, n, 0] == 0
    for n, (l, r) in kat.items():
        assert abs(y[0, n, 0] - l) <= 1e-8 * max(1.0, abs(l)) * 10 + abs(l) * 1e-8, n
        assert abs(y[1, n, 0] - r) <= abs(r) * 1e-8 + 1e-12, n


def test_dattorro_noise_10s_kat(golden):
    g = golden["dattorro_noise_10s"]
    x = O.xorshift_noise(g["seed"], g["frames"])
    y = O.Dattorro(1).process(x[None, :, None])
    assert f"{O.fnv1a64_lr(y[0, :, 0], y[1, :, 0]):016x}" == g["fnv1a64"]
    s = float(np.sum(y[0, :, 0].astype(np.float64) ** 2))
    assert s == pytest.approx(g["sum_l2"], rel=0, abs=0)
    assert round(s, 3) == g["survey_sum_l2"]


def test_dattorro_param_sweep_golden(golden):
    for g in golden["dattorro_sweep"]:
        p = np.asarray(g["params"], np.float32)
        x = noise_block(g["n"], g["frames"], g["input_base"])
        bank = O.Dattorro(g["n"])
        for i in range(g["n"]):
            for f in range(7):
                bank.set(i, f, float(p[f, i]))
        y = bank.process(x)
        got = [f"{O.fnv1a64_lr(y[0, :, i], y[1, :, i]):016x}" for i in range(g["n"])]
        assert got == g["fnv1a64"], g["pre_delay"]


def test_dattorro_blocked_equals_unblocked():
    """Streaming in 256-frame blocks == one long call (state carried exactly)."""
    x = noise_block(3, 2048, 7)
    a = O.Dattorro(3).process(x)
    b = O.Dattorro(3)
    y = np.concatenate([b.process(x[:, k:k + 256]) for k in range(0, 2048, 256)], axis=1)
    assert bits_equal(a, y)


# ---------------------------------------------------------------- dattorro, vs the reference itself
# The reference's own output for each run of helpers.dt_reference_cases is committed, per
# instance, as the fnv1a64 of its bits (tests/golden/dattorro_reference_runs.json, recorded by
# gen_golden.py from the -O2 build after checking the -O0 build against it): the restatement must
# reproduce it wherever the suite runs, and, where oracle/_ref is built, the reference build itself
# is run beside it and compared bit for bit as well.
@pytest.fixture(scope="module")
def reference_runs():
    import json
    import os
    with open(os.path.join(os.path.dirname(__file__), "golden", "dattorro_reference_runs.json")) as f:
        recorded = json.load(f)
    return {k: (p, x, recorded[k]["fnv1a64"]) for k, (p, x) in dt_reference_cases().items()}


def _port_equals_reference(run, threads=1):
    p, x, recorded = run
    ya = run_dattorro(O.Dattorro(x.shape[2]), p, x, threads)
    assert lr_hashes(ya) == recorded
    if O.ref_available():
        yb = run_dattorro(O.Dattorro(x.shape[2], ref=True), p, x, threads)
        assert lr_hashes(yb) == recorded
        assert bits_equal(ya, yb), first_mismatch(ya, yb)
    return ya


def test_dattorro_port_equals_reference_random_params(reference_runs):
    _port_equals_reference(reference_runs["random_params"], threads=4)


def test_dattorro_port_equals_reference_edge_params(reference_runs):
    """Extremes of the setters: zero pre-delay, decay clamp both ends, zero/unit gains."""
    ya = _port_equals_reference(reference_runs["edge_params"])
    assert np.all(np.isfinite(ya))


def test_dattorro_reference_O0_equals_O2(reference_runs):
    """The reference compiled at -O0 (its CMake default) and at -O2 gives the same bits: the
    recorded output (checked for both builds when it was recorded) is reproduced by each build that
    is present here, and by the restatement."""
    _, x, recorded = reference_runs["default_params"]
    _port_equals_reference(reference_runs["default_params"])
    if O.ref_available() and O.ref_available(o0=True):
        y2, y0 = O.Dattorro(2, ref=True).process(x), O.Dattorro(2, ref=True, o0=True).process(x)
        assert bits_equal(y2, y0), first_mismatch(y2, y0)
        assert lr_hashes(y0) == recorded


@pytest.mark.parametrize("name", ["subnormal", "loud100", "loud127", "burst", "negzero"])
def test_dattorro_port_equals_reference_edge_signals(reference_runs, name):
    """Signals at the edge of fp32 (helpers.edge_signals): the reverb stays finite on each, the
    restatement reproduces the reference's recorded bits, and the subnormal input gives subnormal
    output (nothing on the CPU side flushes)."""
    ya = _port_equals_reference(reference_runs["edge_signal_" + name])
    assert np.all(np.isfinite(ya))
    if name == "subnormal":
        assert subnormal_share(ya) >= 0.5
    if name == "negzero":
        assert not np.any(ya)


def test_dattorro_port_equals_reference_corner_params(reference_runs):
    """The 128 corners {0, 1}^7 of the seven setters, pre-delay 0 and 4800 samples included."""
    ya = _port_equals_reference(reference_runs["corner_params"], threads=4)
    assert np.all(np.isfinite(ya))


@pytest.mark.parametrize("name", UNIFORM_PD_RUNS)
def test_dattorro_port_equals_reference_uniform_predelay(reference_runs, name):
    """One pre-delay for all instances: 0..8 samples (inside the last two 4-frame steps), 9, 257, the
    setter's maximum 4800, and 8191 over 70,000 frames (the ring's longest delay, across t = 32768
    and the uint16 wrap) -- the runs the GPU's uniform-pre-delay network is held to as well.  The
    2,048 frames at 4800 end before the first delayed sample: that run's output is all zeros."""
    ya = _port_equals_reference(reference_runs[name], threads=4)
    assert np.all(np.isfinite(ya)) and np.any(ya != 0) == (name != "uniform_pd_4800")


def test_dattorro_port_equals_reference_poisoned_input():
    """Single NaN / +-Inf input samples (helpers.poison_table): only the poisoned instances differ
    from the clean run, and, where oracle/_ref is built, the restatement equals the reference build
    as arrays, NaN bits included."""
    n = 70
    p, x = dt_edge_params(n), fast_noise(n, EDGE_FRAMES, seed=40)
    xp = poisoned(x)
    ya = run_dattorro(O.Dattorro(n), p, xp, threads=4)
    if O.ref_available():
        yb = run_dattorro(O.Dattorro(n, ref=True), p, xp, threads=4)
        assert bits_equal(ya, yb), first_mismatch(ya, yb)
    bad = sorted({i for _, _, i, _ in poison_table(n)})
    assert all(not np.all(np.isfinite(ya[:, :, i])) for i in bad)
    clean = np.setdiff1d(np.arange(n), bad)
    yc = run_dattorro(O.Dattorro(n), p, x, threads=4)
    assert bits_equal(ya[:, :, clean], yc[:, :, clean])


def test_dattorro_empty_block():
    b = O.Dattorro(2)
    y = b.process(np.zeros((2, 0, 2), np.float32))
    assert y.shape == (2, 0, 2)


# ---------------------------------------------------------------- chorus / pitch-shift (unpinned)
@pytest.mark.parametrize("key,mode", [("chorus", 0), ("pitchshift", 1)])
def test_chorus_frozen_golden(golden, key, mode):
    g = golden[key]
    p = np.asarray(g["params"], np.float32)
    x = noise_block(g["n"], g["frames"], g["input_base"])
    ch = O.Chorus(g["n"], 48000.0, mode)
    for i in range(g["n"]):
        for f in range(8):
            ch.set(i, f, float(p[f, i]))
    y = ch.process(x)
    assert [f"{O.fnv1a64_lr(y[0, :, i], y[1, :, i]):016x}" for i in range(g["n"])] == g["fnv1a64"]


def _dev(y, ref):
    d = np.abs(np.asarray(y, np.float64) - ref)
    rms = np.sqrt(np.mean(ref ** 2, axis=1, keepdims=True))
    return float(np.max(d / np.maximum(np.abs(ref), rms))), float(10 * np.log10(np.sum(ref ** 2) / max(np.sum(d ** 2), 1e-300)))


def _c64(g, mode, p):
    b = O.Chorus64(g["n"], 48000.0, mode)
    for i in range(g["n"]):
        for f in range(8):
            b.set(i, f, float(p[f, i]))
    return b


@pytest.mark.parametrize("key,mode", [("chorus", 0), ("pitchshift", 1)])
def test_chorus_fp32_deviation_from_double(golden, key, mode):
    """The spec's declared deviation (fp32 signal arithmetic, 64-bit fixed-point phasors, spec v2's
    precise tap delays) MEASURED against the same graph in double precision with double phasors
    (gen~ / RNBO arithmetic, oracle/chorus_ref_f64.c) on the golden inputs (6 instances x 6,000
    frames of white noise).  Round 4 (spec v2): chorus 6.5e-6 of max(|ref|, rms) (118 dB), pitch-shift
    8.4e-7 (137 dB); round 3 (fp32 delays): 1.62e-4 / 1.29e-4 (93 dB).  Rounding the double
    restatement's increments to the spec's fixed point changes nothing measurable.  Parity stays
    unpinned (RNBO / genlib absent); this bounds only the arithmetic, below the north star's 1e-5."""
    g = golden[key]
    p = np.asarray(g["params"], np.float32)
    x = noise_block(g["n"], g["frames"], g["input_base"])
    a = O.Chorus(g["n"], 48000.0, mode)
    for i in range(g["n"]):
        for f in range(8):
            a.set(i, f, float(p[f, i]))
    ya = a.process(x)
    out = {}
    for q in (0, 2):
        out[q] = _dev(ya, _c64(g, mode | q, p).process(x))
        print(f"{key} {'fixed-point increments' if q else 'double increments'}: rel {out[q][0]:.3g}, SNR {out[q][1]:.1f} dB")
    for q in (0, 2):
        assert out[q][0] <= 1e-5 and out[q][1] >= 110.0
    assert abs(out[0][0] - out[2][0]) <= 0.1 * out[2][0]


# stage bits of oracle/chorus_ref_f64.c (mode >> 2): fp32 emulation of one stage at a time
_F32 = {"pitch delay": 1, "pitch gains": 2, "pitch interp": 4, "chorus delay": 8, "chorus interp": 16,
        "lores~": 32, "mix": 64}
_FIX_PDELAY, _DBL_CDELAY = 128, 256


def test_chorus_deviation_by_stage(golden):
    """Where the fp32 spec's deviation from double comes from, stage by stage (each stage alone as
    the spec computes it, everything else in double; oracle/chorus_ref_f64.c).  Round 3's delays
    (24-bit phase, fp32 p W and D cos + D) were the whole of it: the chorus delay 1.6e-4, the pitch
    delay 6e-5 (chorus) / 1.3e-4 (pitch-shift); spec v2's delays (fixed-point p W, double D cos + D)
    bring each below 1e-6, and lores~'s fp32 state (6e-6) is what remains; spec v3's fused
    multiply-adds (round 6) take the whole to 5.8e-6."""
    g = golden["chorus"]
    p = np.asarray(g["params"], np.float32)
    x = noise_block(g["n"], g["frames"], g["input_base"])
    ref = _c64(g, 2, p).process(x)
    dev = {k: _dev(_c64(g, 2 | (b << 2), p).process(x), ref)[0] for k, b in _F32.items()}
    for k, v in dev.items():
        print(f"{k:14s} {v:.3g}")
    assert dev["chorus delay"] > 1e-4 and dev["pitch delay"] > 3e-5       # round 3's delays dominated
    assert max(v for k, v in dev.items() if "delay" not in k) < 1e-5     # the signal arithmetic did not
    # all stages as round 3 computed them == round 3's spec (the emulation is faithful: 1.62e-4)
    r3 = _dev(_c64(g, 2 | (127 << 2), p).process(x), ref)[0]
    assert 1.5e-4 < r3 < 1.8e-4
    # spec v2: the fp32 stages (unfused, as emulated here) with the precise delays; the spec oracle
    # is v3 (round 6: the same stages in fused multiply-adds), whose deviation is no larger
    v2 = _dev(_c64(g, 2 | (((127 & ~(1 | 8)) | _FIX_PDELAY | _DBL_CDELAY) << 2), p).process(x), ref)[0]
    a = O.Chorus(g["n"], 48000.0, 0)
    for i in range(g["n"]):
        for f in range(8):
            a.set(i, f, float(p[f, i]))
    v3 = _dev(a.process(x), ref)[0]
    print(f"spec v2 (unfused) {v2:.3g}, spec v3 (the oracle, fused) {v3:.3g}")
    assert 0.5 * v2 <= v3 <= v2
    assert v2 < 1e-5


def test_cos2pi_d_accuracy():
    """spec v2's double cos(2 pi x) (chorus LFO): within 1e-14 of libm's over [-3, 3]."""
    xs = np.linspace(-3, 3, 20001)
    L = O.lib()
    L.oracle_cos2pi_d.restype = ctypes.c_double
    L.oracle_cos2pi_d.argtypes = [ctypes.c_double]
    got = np.array([L.oracle_cos2pi_d(float(v)) for v in xs])
    assert np.max(np.abs(got - np.cos(2 * np.pi * xs))) < 1e-14


def test_cos2pi_accuracy():
    xs = np.linspace(-3, 3, 20001).astype(np.float32)
    got = np.array([O.lib().oracle_cos2pi(float(v)) for v in xs], np.float64)
    assert np.max(np.abs(got - np.cos(2 * np.pi * xs.astype(np.float64)))) < 3e-7


def test_window_gains_accuracy():
    """The pitch-shifter's crossfade windows (pitchshift.gendsp: cos((p0 - 1/2) pi) for tap 0 and
    cos((p1 - 1/2) pi), p1 = (p0 + 1/2) mod 1, for tap 1) from one argument, sin / cos of
    pi min(p, 1 - p): within 3e-7 of both cosines over 24-bit phases, and exact at the ends."""
    import ctypes
    L = O.lib()
    ps = (np.arange(0, 1 << 24, 997, dtype=np.int64).astype(np.float64) / (1 << 24))
    g0, g1 = ctypes.c_float(), ctypes.c_float()
    e = 0.0
    for p in ps:
        L.oracle_win_gains(float(p), ctypes.byref(g0), ctypes.byref(g1))
        p1 = (p + 0.5) % 1.0
        e = max(e, abs(g0.value - np.cos((p - 0.5) * np.pi)), abs(g1.value - np.cos((p1 - 0.5) * np.pi)))
    assert e < 3e-7, e
    L.oracle_win_gains(0.0, ctypes.byref(g0), ctypes.byref(g1))
    assert g0.value == 0.0 and g1.value == 1.0


def test_chorus_behaviour():
    """Mix 0 is exactly dry; pitch 0 makes the shifter a fixed W/2 delay; outputs finite."""
    n = 3
    x = noise_block(n, 4000, 11)
    ch = O.Chorus(n)
    ch.set(0, "mix", 0.0)
    ch.set(1, "pitch", 0.0)
    y = ch.process(x)
    assert np.array_equal(y[:, :, 0], x[:, :, 0])
    assert np.all(np.isfinite(y))
    ps = O.Chorus(n, mode=1)   # pitch 0: taps at delay 1 (gain cos(-pi/2) ~ 0) and W/2 = 240 (gain 1)
    yp = ps.process(x)
    np.testing.assert_allclose(yp[:, 300:, 0], x[:, 300 - 240:4000 - 240, 0], atol=2e-6)


def test_chorus_blocked_equals_unblocked():
    x = noise_block(4, 2048, 21)
    a = O.Chorus(4).process(x)
    b = O.Chorus(4)
    y = np.concatenate([b.process(x[:, k:k + 128]) for k in range(0, 2048, 128)], axis=1)
    assert bits_equal(a, y)


# ---------------------------------------------------------------- voice (unpinned) + reference pins
def test_voice_frozen_golden(golden):
    g = golden["voice"]
    p = np.asarray(g["params"], np.float32)
    vo = O.Voice(g["n"])
    for i in range(g["n"]):
        vo.config(i, p[:, i])
        vo.note(i, True, g["notes"][i])
    ya = vo.process(g["note_off_at"])
    for i in range(g["n"]):
        vo.note(i, False, g["notes"][i])
    yb = vo.process(g["frames"] - g["note_off_at"])
    y = np.concatenate([ya, yb], axis=1)
    assert [f"{O.fnv1a64_lr(y[0, :, i], y[0, :, i]):016x}" for i in range(g["n"])] == g["fnv1a64"]


def test_voice_reference_pins_synth_test():
    """test/synth_test.cpp:102-148 (TEST(Synth, VoiceDefaultConstructor)), restated."""
    vo = O.Voice(1)
    # NoteOn, NoteOff, then first Process -> exactly 0 (first polyBLEP saw sample is 0)
    vo.note(0, True, 60)
    vo.note(0, False, 60)
    assert vo.process(1)[0, 0, 0] == 0
    vo.note(0, True, 60)
    v = vo.process(2)[0, :, 0]
    assert v[-1] != 0 and v[-1] != 1
    # amp_env_amount = 0 -> 0; = 1 -> != 0
    cfg = np.asarray(O.VOICE_DEFAULTS, np.float32)
    cfg[O.VC_FIELDS.index("amp_env_amount")] = 0.0
    vo.config(0, cfg)
    assert vo.process(1)[0, 0, 0] == 0
    cfg[O.VC_FIELDS.index("amp_env_amount")] = 1.0
    vo.config(0, cfg)
    assert vo.process(1)[0, 0, 0] != 0


def test_voice_silent_until_note():
    vo = O.Voice(2)
    assert np.all(vo.process(512) == 0)


@pytest.mark.parametrize("moog", [False, True])
def test_voice_kernel_arith_mode_tracks_the_restatement(golden, moog):
    """The oracle's kernel-arithmetic mode (voice_ref.c: the GPU kernels' contractions, sine
    polynomial and reciprocal; here with the correctly rounded reciprocal, no device table) stays
    within the voice tolerance of the unfused restatement on the golden voices, keeps the
    synth_test.cpp:102-148 first-sample pins, and is not the restatement itself."""
    g = golden["voice_moog" if moog else "voice"]
    p = np.asarray(g["params"], np.float32)
    outs = []
    for karith in (False, True):
        vo = O.Voice(g["n"], moog=moog, kernel_arith=karith)
        for i in range(g["n"]):
            vo.config(i, p[:, i])
            vo.note(i, True, g["notes"][i])
        ya = vo.process(g["note_off_at"])
        for i in range(g["n"]):
            vo.note(i, False, g["notes"][i])
        outs.append(np.concatenate([ya, vo.process(g["frames"] - g["note_off_at"])], axis=1))
    assert rel_err(outs[1][0].T, outs[0][0].T) <= 1e-5
    assert not bits_equal(outs[0], outs[1])
    vo = O.Voice(1, moog=moog, kernel_arith=True)
    vo.note(0, True, 60)
    vo.note(0, False, 60)
    assert vo.process(1)[0, 0, 0] == 0


def test_rcp_model_scales_the_mantissa_table():
    """The v_rcp model (voice_ref.c oracle_rcp_model): no table = correctly rounded 1/x; with a table
    of the 2^23 mantissa results, rcp(m 2^e) = table[m] 2^-e with the sign kept, and 1/x for inputs
    whose result is not normal."""
    xs = np.array([1.0, 1.5, 3.0, 0.007, -27.5, 108.0, 1e-30, 3e37], np.float32)
    O.set_rcp_table(None)
    L = O.lib()
    assert [L.oracle_rcp_model(float(x)) for x in xs] == [float(np.float32(1) / x) for x in xs]
    x = ((np.uint32(127) << np.uint32(23)) | np.arange(1 << 23, dtype=np.uint32)).view(np.float32)
    tab = (np.float32(1.0) / x).view(np.uint32).copy()
    tab[1:] += 1                                       # every result but 1/1 one ulp up
    try:
        O.set_rcp_table(tab)
        got = np.array([L.oracle_rcp_model(float(v)) for v in xs], np.float32)
        want = (np.float32(1) / xs)
        w = want.view(np.uint32).copy()
        w[(xs.view(np.uint32) & 0x7FFFFF) != 0] += 1      # all but the exact powers of two
        assert np.array_equal(got.view(np.uint32), w), (got, w.view(np.float32))
    finally:
        O.set_rcp_table(None)


# ------------------------------------------- MoogFilter voice (daisysp::LadderFilter, unpinned)
def _moog_run(cfg_edit=None, frames=4800, note=48):
    vo = O.Voice(1, moog=True)
    cfg = np.asarray(O.VOICE_DEFAULTS, np.float32)
    cfg[O.VC_FIELDS.index("filter_env_amount")] = 0.0
    for k, v in (cfg_edit or {}).items():
        cfg[O.VC_FIELDS.index(k)] = v
    vo.config(0, cfg)
    vo.note(0, True, note)
    return vo.process(frames)[0, :, 0]


def test_voice_moog_frozen_golden(golden):
    g = golden["voice_moog"]
    p = np.asarray(g["params"], np.float32)
    vo = O.Voice(g["n"], moog=True)
    for i in range(g["n"]):
        vo.config(i, p[:, i])
        vo.note(i, True, g["notes"][i])
    ya = vo.process(g["note_off_at"])
    for i in range(g["n"]):
        vo.note(i, False, g["notes"][i])
    y = np.concatenate([ya, vo.process(g["frames"] - g["note_off_at"])], axis=1)
    assert [f"{O.fnv1a64_lr(y[0, :, i], y[0, :, i]):016x}" for i in range(g["n"])] == g["fnv1a64"]


def test_voice_moog_reference_pins_and_filter_semantics():
    """synth_test.cpp:102-148 pins hold for the firmware's MoogFilter voice too; MoogFilter::SetDrive
    is a no-op (Filter.h:47); the LP24 ladder attenuates a 1 kHz saw far more at 200 Hz than at 8 kHz; a
    resonance past the clamp (K = 4 * 1.8) stays bounded through the tanh."""
    vo = O.Voice(1, moog=True)
    vo.note(0, True, 60)
    vo.note(0, False, 60)
    assert vo.process(1)[0, 0, 0] == 0
    vo.note(0, True, 60)
    v = vo.process(2)[0, :, 0]
    assert v[-1] != 0 and v[-1] != 1
    a = _moog_run({"filter_cutoff": 3000.0, "filter_drive": 0.0})
    b = _moog_run({"filter_cutoff": 3000.0, "filter_drive": 9.0})
    assert bits_equal(a, b)
    lo = _moog_run({"filter_cutoff": 200.0, "filter_resonance": 0.0}, note=84)
    hi = _moog_run({"filter_cutoff": 8000.0, "filter_resonance": 0.0}, note=84)
    rms = lambda y: float(np.sqrt(np.mean(y[2400:].astype(np.float64) ** 2)))
    assert rms(lo) < 0.25 * rms(hi)
    r = _moog_run({"filter_cutoff": 1000.0, "filter_resonance": 5.0}, frames=48000)
    assert np.all(np.isfinite(r)) and np.abs(r).max() < 4.0
    assert not bits_equal(r, _moog_run({"filter_cutoff": 1000.0, "filter_resonance": 1.0}, frames=48000))
    assert bits_equal(r, _moog_run({"filter_cutoff": 1000.0, "filter_resonance": 1.8}, frames=48000))


# ------------------------------------------------------------------------------- fx rack
def test_fxrack_defaults_and_echo():
    """FxRack<2> at its reference defaults (Fx.h): the delay echo arrives exactly
    scale(0.5, 0,1, 0,48000) = 24000 samples later, and channel 1 of the output stays 0 because
    FilterFx writes only channel 0 (Fx.h:88-108) into the zero-initialised buf_c (Fx.h:408)."""
    p = O.fxrack_defaults()
    assert p[0] == 0.5 and p[2] == np.float32(0.33) and p[10] == np.float32(0.8)
    assert p[3] == np.float32(64 * np.float32(1 / 127)) * 20000
    r = O.FxRack(1)
    x = np.zeros((2, 30000, 1), np.float32)
    x[:, 0, 0] = 1.0
    y = r.process(x)
    assert np.all(y[1] == 0)
    assert abs(y[0, 0, 0]) > 0.1
    quiet = np.abs(y[0, 2000:23990, 0]).max()
    echo = np.abs(y[0, 24000:24200, 0]).max()
    assert echo > 100 * quiet


def test_fxrack_sine_never_nan():
    """test/fx_test.cpp:25-55: the delay fed a 20 kHz sine at 48 kHz for one second never
    outputs NaN (here through the whole rack, every filter type, a few delay settings)."""
    n = 10
    r = O.FxRack(n)
    for i in range(n):
        r.set(i, "filter_type", float(i % 5))
        r.set(i, "delay_time", [0.5, 0.0, 1.0, 1e-5, 0.25][i % 5])
    t = np.arange(48000, dtype=np.float64)
    s = (0.5 * np.sin(2 * np.pi * 20000 * t / 48000)).astype(np.float32)
    x = np.broadcast_to(s[None, :, None], (2, 48000, n)).copy()
    y = r.process(x, threads=4)
    assert np.all(np.isfinite(y))


def test_fxrack_blocked_equals_unblocked_and_golden(golden):
    g = golden["fxrack"]
    p = np.asarray(g["params"], np.float32)
    x = noise_block(g["n"], g["frames"], g["input_base"])
    a, b = O.FxRack(g["n"]), O.FxRack(g["n"])
    for i in range(g["n"]):
        for f in range(p.shape[0]):
            a.set(i, f, float(p[f, i]))
            b.set(i, f, float(p[f, i]))
    ya = a.process(x)
    yb = np.concatenate([b.process(x[:, s:s + 1000]) for s in range(0, g["frames"], 1000)], 1)
    assert bits_equal(ya, yb), first_mismatch(ya, yb)
    assert [f"{O.fnv1a64_lr(ya[0, :, i], ya[1, :, i]):016x}" for i in range(g["n"])] == g["fnv1a64"]



# ------------------------------------------------------------- voice buses (Polyvoice, 8a A17)
def test_mix_ref_is_the_in_order_float32_sum():
    """oracle.mix_ref restates Polyvoice::Process's `*frame_out += frame_buffer` (Polyvoice.h:28-33):
    checked against a scalar float32 loop, with an empty bus and a non-zero starting frame."""
    rng = np.random.default_rng(3)
    v = (rng.standard_normal((1, 7, 12)) * 1e3).astype(np.float32)
    buses = [[3, 1, 7], [], [0, 2, 4, 5, 6, 8, 9, 10, 11], [11]]
    init = rng.standard_normal((7, 4)).astype(np.float32)
    got = O.mix_ref(v, buses, init)
    for f in range(7):
        for b, vs in enumerate(buses):
            acc = np.float32(init[f, b])
            for i in vs:
                acc = np.float32(acc + v[0, f, i])
            assert got[f, b].tobytes() == acc.tobytes()


def test_committed_rcp_model():
    """tests/golden/rcp_f32_gfx950.npz, the voice oracle's committed v_rcp_f32 model (VERDICT r5 #4;
    written on an MI355X by tools/rcp_dump.py): it decodes to the table its own sha256 names, every
    entry is within one ulp of the correctly rounded 1/x, and it has the exception counts measured
    in round 5: 897,675 mantissas of 2^23 one ulp off, 761,701 down and 135,974
    up.  The GPU tests compare the device with this table before using it (conftest rcp_table)."""
    import rcp_model
    tab = rcp_model.load()
    d = tab.astype(np.int64) - rcp_model.correctly_rounded().astype(np.int64)
    assert tab.shape == (1 << 23,) and np.abs(d).max() == 1
    assert int(np.count_nonzero(d)) == 897675
    assert int(np.count_nonzero(d == -1)) == 761701 and int(np.count_nonzero(d == 1)) == 135974
    assert rcp_model.decode(rcp_model.encode(tab)).tobytes() == tab.tobytes()
