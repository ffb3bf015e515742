"""GPU edges: the HIP kernels on signals and parameters at the edge of fp32, against the CPU oracle.

What test_gpu_parity.py leaves out: every run there feeds uniform noise in [-0.5, 0.5) through
parameters from the interior of their ranges.  Here
  - signals: subnormal, decaying into silence, loud enough to overflow, single NaN / +-Inf samples
    in a few instances, -0.0 and constants, through every effect kind;
  - parameters: every corner of the setters' ranges, and values pushed past the clamps;
  - containment: the floats next to the caller's buffers are neither written nor used.
Every comparison is helpers.same_bits_or_nan: +-Inf, +-0 and subnormals exact, the NaN masks equal,
NaN sign and payload not compared (x86 and the GPU generate different default NaNs).  Each signal
also states a condition on the ORACLE's output (a share of subnormal or non-finite samples), so
that no case passes without the edge it is about; the shares are printed (pytest -s).
The three fused kinds (platerack, voice_sample, synth) get the same questions in
tests/test_gpu_edges_fused.py.
"""
import numpy as np
import pytest

import oracle as O
from helpers import (EDGE_BLOCKS, EDGE_FRAMES, UNIFORM_PD_RUNS, bits_equal, chorus_params, dt_corner_params, dt_edge_params,
                     dt_reference_cases, edge_signals, fast_noise, first_mismatch, first_mismatch_or_nan,
                     fxrack_params, lr_hashes, nonfinite_share, poison_table, poisoned, same_bits_or_nan,
                     subnormal_share, voice_configs)
from test_gpu_parity import _chain_oracle, _fxrack_pair, _voice_run, engine, run_gpu, voice_bits_equal

pytestmark = pytest.mark.gpu

EFFECTS = ["dattorro", "chorus", "pitchshift", "chain", "fxrack"]
VOICES = ["voice", "voice_moog"]
# the @min / @max pairs of the chorus parameters (include/olfx.h OLFX_CH_*)
CH_BOUNDS = np.array([(0, 3), (0, 1), (0, 1), (0, 1), (0, 1), (0.08, 1), (0.01, 1), (4, 10)], np.float32)
RAGGED_4096 = [256] * 7 + [4, 12, 240, 2048]


def _params(kind, n, seed=40):
    """Seeded interior parameters of one kind; the rack runs all five topologies in one engine."""
    rng = np.random.default_rng(seed)
    if kind == "dattorro":
        return dt_edge_params(n, seed)
    if kind == "chorus":
        return chorus_params(rng, n)
    if kind == "pitchshift":
        return chorus_params(rng, n)[[0, 7]]
    if kind == "chain":
        return np.concatenate([chorus_params(rng, n), chorus_params(rng, n)[[0, 7]], dt_edge_params(n, seed)], 0)
    if kind == "fxrack0":
        return fxrack_params(rng, n)
    return np.concatenate([fxrack_params(rng, n), (np.arange(n) % 5)[None, :].astype(np.float32)], 0)


def _pair(kind, n, p):
    """(engine, oracle) with parameters p [fields][n]; oracle(x) -> the expected output, stateful
    like the engine.  The chain's oracle is the composed chorus -> pitch-shift -> reverb."""
    if kind in ("fxrack", "fxrack0"):
        e, ref = _fxrack_pair(n, p)
        return e, lambda x: ref.process(x, threads=8)
    e = engine(kind, n)
    e.set_params(0, p)
    if kind == "chain":
        c1, c2, d = _chain_oracle(n, p[:8], p[8:10], p[10:])
        return e, lambda x: d.process(c2.process(c1.process(x, threads=8), threads=8), threads=8)
    if kind == "dattorro":
        ref = O.Dattorro(n)
    else:
        ref = O.Chorus(n, mode=0 if kind == "chorus" else 1)
    names = {"pitchshift": ("pitch", "window")}.get(kind, range(p.shape[0]))
    for i in range(n):
        for f, name in enumerate(names):
            ref.set(i, name, float(p[f, i]))
    return e, lambda x: ref.process(x, threads=8)


def _check(y, yr):
    assert same_bits_or_nan(y, yr), first_mismatch_or_nan(y, yr)


# ------------------------------------------------------------------------------- signal edges
SIGNALS = ["subnormal", "burst", "loud100", "negzero", "ones", "alternating"]
# "fxrack" mixes the five topologies, which takes the kernel variant that serves standalone
# components; "fxrack0" is an engine of FxRack<2> instances only (topology 0), the other variant
RACKS = ["fxrack", "fxrack0"]
SIGNAL_CASES = ([(k, s) for k in EFFECTS + ["fxrack0"] for s in SIGNALS]
                + [("chorus", "loud127"), ("chain", "loud127")])


@pytest.mark.parametrize("n", [70, 72])
@pytest.mark.parametrize("kind,signal", SIGNAL_CASES)
def test_signal_edges(cuda, kind, signal, n):
    """Every effect kind on helpers.edge_signals, n = 70 (per-lane I/O, a partial 64-group, a partial
    32-instance chorus wave) and n = 72 (cooperative rows), ragged calls.  The oracle-side
    conditions, with the shares this file prints at n = 70 / n = 72:
      subnormal (x * 2^-130): at least half of the oracle's non-zero samples subnormal (measured: all
        of them, every kind) -- a flush to zero anywhere in a kernel shows as zeros against them;
      burst (300 frames, then exact zeros): chorus and rack decay into subnormals (lores~ and
        delay-feedback tails), at least 5 % of the non-zero samples (measured: chorus 21.1 / 17.2 %,
        rack 30.3 / 24.6 %, racks only 26.1 / 25.6 %);
      loud100 (x * 2^100): the rack's Svf overflows to Inf and NaN, at least 20 % of its samples
        (measured 30.0 / 30.5 %; racks only 50 %, all of channel 0, bound 10 %); the reverb and the
        pitch-shift stay finite;
      loud127 (x * 2^127, chorus and chain): at least 5 % non-finite (measured: chorus 14.1 / 7.8 %,
        chain 16.8 / 9.0 %);
      negzero, ones, alternating (+-1 per frame): bit-exact, the sign of zero counts."""
    x = edge_signals(fast_noise(n, EDGE_FRAMES, seed=40))[signal]
    e, oracle = _pair(kind, n, _params(kind, n))
    yr = oracle(x)
    sub, nonfin = subnormal_share(yr), nonfinite_share(yr)
    print(f"\n{kind} n={n} {signal}: oracle subnormal share of non-zero {100 * sub:.1f} %, "
          f"non-finite share {100 * nonfin:.1f} %")
    if signal == "subnormal":
        assert np.any(yr != 0) and sub >= 0.5
    if signal == "burst" and kind in ["chorus"] + RACKS:
        assert sub >= 0.05
    if signal == "loud100" and kind in RACKS:
        # of the racks alone only channel 0 can overflow (output channel 1 is 0): half the share
        assert nonfin >= (0.20 if kind == "fxrack" else 0.10)
        assert kind == "fxrack" or not np.any(yr[1])
    if signal == "loud100" and kind in ("dattorro", "pitchshift"):
        assert nonfin == 0
    if signal == "loud127":
        assert nonfin >= 0.05
    _check(run_gpu(e, x, EDGE_BLOCKS, cuda), yr)


@pytest.mark.parametrize("n", [70, 72])
@pytest.mark.parametrize("kind", EFFECTS + ["fxrack0"])
def test_poisoned_instances_stay_isolated(cuda, kind, n):
    """Single NaN / +Inf / -Inf input samples in instances 0, 5, 63, 64 and n-1 (the first and the
    last instance, both sides of a wave edge; helpers.poison_table): (a) the whole output matches the
    oracle; (b) every instance that was not poisoned is bit-identical to a second GPU run on the
    clean signal -- no lane reads a neighbour's sample, a junk slot or a partial sum of another
    instance, not even times a zero gain; (c) at least 4 of the 5 poisoned instances are non-finite
    in the oracle (the rack's topology 0 ignores input channel 1: 4 of 5 there, 5 of 5 elsewhere;
    in the engine of racks only, both instances poisoned on channel 1 alone stay clean, 3 of 5, and
    are then held to the clean run as well)."""
    x = fast_noise(n, EDGE_FRAMES, seed=40)
    xp = poisoned(x)
    p = _params(kind, n)
    e, oracle = _pair(kind, n, p)
    yr = oracle(xp)
    bad = sorted({i for _, _, i, _ in poison_table(n)})
    hit = sum(1 for i in bad if not np.all(np.isfinite(yr[:, :, i])))
    print(f"\n{kind} n={n} poisoned: {hit} of {len(bad)} poisoned instances non-finite in the oracle, "
          f"non-finite share {100 * nonfinite_share(yr):.1f} %")
    assert len(bad) == 5 and hit >= (3 if kind == "fxrack0" else 4)
    if kind == "fxrack0":
        bad = sorted({i for c, _, i, _ in poison_table(n) if c == 0})
    y = run_gpu(e, xp, EDGE_BLOCKS, cuda)
    _check(y, yr)
    e2, _ = _pair(kind, n, p)
    yc = run_gpu(e2, x, EDGE_BLOCKS, cuda)
    clean = np.setdiff1d(np.arange(n), bad)
    assert np.all(np.isfinite(yc))
    assert bits_equal(y[:, :, clean], yc[:, :, clean]), first_mismatch(y[:, :, clean], yc[:, :, clean])


# --------------------------------------------------- the reverb against the real reference's bits
@pytest.fixture(scope="module")
def reference_runs():
    import json
    import os
    with open(os.path.join(os.path.dirname(__file__), "golden", "dattorro_reference_runs.json")) as f:
        recorded = json.load(f)
    return {k: (p, x, recorded[k]["fnv1a64"]) for k, (p, x) in dt_reference_cases().items()}


@pytest.mark.parametrize("name", ["edge_params", "random_params", "corner_params", "edge_signal_subnormal",
                                  "edge_signal_loud100", "edge_signal_loud127", "edge_signal_burst",
                                  "edge_signal_negzero"] + UNIFORM_PD_RUNS)
def test_dattorro_equals_reference_hashes(cuda, reference_runs, name):
    """The GPU reverb held to the hashes the REAL reference build produced
    (tests/golden/dattorro_reference_runs.json; tests/test_oracle.py holds the CPU oracle to the
    same): the setter extremes (gains exactly 0 and 1, decay at both clamps), the random run over
    70,000 frames, the 128 corners, the all-finite edge signals at n = 8, and the runs with one
    pre-delay for all instances (dattorro_block_v5 at these sizes; tests/test_gpu_dattorro_v4.py holds
    dattorro_block_v4 to the same hashes)."""
    p, x, recorded = reference_runs[name]
    n, frames = x.shape[2], x.shape[1]
    e = engine("dattorro", n)
    e.set_params(0, p)
    if frames == EDGE_FRAMES:
        blocks = EDGE_BLOCKS
    else:
        blocks = [4096] * (frames // 4096) + ([frames % 4096] if frames % 4096 else [])
    y = run_gpu(e, x, blocks, cuda)
    assert np.all(np.isfinite(y))
    assert lr_hashes(y) == recorded


# --------------------------------------------------------------------------- parameter corners
def test_dattorro_corners(cuda):
    """The 128 corners {0, 1}^7 of the reverb's setters in one engine (pre-delays 0 and 4800 mixed:
    gather mode), ragged calls: bit-exact against the oracle, which is finite on every instance."""
    n = 128
    p = dt_corner_params()
    x = fast_noise(n, 4096, seed=4)
    e, oracle = _pair("dattorro", n, p)
    yr = oracle(x)
    assert np.all(np.isfinite(yr))
    _check(run_gpu(e, x, [256] * 8 + [4, 2044], cuda), yr)


def _chorus_corners():
    """[8][256] corner values and the same corners pushed 1.0 past their bounds."""
    bit = ((np.arange(256)[None, :] >> np.arange(8)[:, None]) & 1).astype(bool)
    lo, hi = CH_BOUNDS[:, :1], CH_BOUNDS[:, 1:]
    return np.where(bit, hi, lo).astype(np.float32), np.where(bit, hi + 1, lo - 1).astype(np.float32)


@pytest.mark.parametrize("kind", ["chorus", "pitchshift"])
def test_chorus_corners_and_clamps(cuda, kind):
    """The 256 corners of the eight @min / @max pairs (include/olfx.h); then the same engine after
    reset() with every value 1.0 past its bound, which RNBO clamps: the same bits, and both equal to
    the oracle (finite on every instance).  The pitch-shift takes the pitch and window columns."""
    n = 256
    p, past = _chorus_corners()
    if kind == "pitchshift":
        p, past = p[[0, 7]], past[[0, 7]]
    x = fast_noise(n, 4096, seed=6)
    e, oracle = _pair(kind, n, p)
    yr = oracle(x)
    assert np.all(np.isfinite(yr))
    y1 = run_gpu(e, x, RAGGED_4096, cuda)
    _check(y1, yr)
    e.reset()
    e.set_params(0, past)
    y2 = run_gpu(e, x, RAGGED_4096, cuda)
    assert bits_equal(y1, y2), first_mismatch(y1, y2)


def test_chain_corners(cuda):
    """256 chain instances, each of the 17 parameters at a random corner (chorus and pitch-shift
    @min / @max, the reverb's setters 0 / 1: pre-delay 0 or 4800 samples, both inside the range
    bad_value accepts): bit-exact against the composed oracle, finite on every instance."""
    n = 256
    rng = np.random.default_rng(17)
    bounds = np.concatenate([CH_BOUNDS, CH_BOUNDS[[0, 7]], np.tile(np.float32([0, 1]), (7, 1))], 0)
    p = np.where(rng.integers(0, 2, (17, n)) == 1, bounds[:, 1:], bounds[:, :1]).astype(np.float32)
    assert np.all(p[10] * np.float32(4800.0) < 65536.0)
    x = fast_noise(n, 4096, seed=17)
    e, oracle = _pair("chain", n, p)
    yr = oracle(x)
    assert np.all(np.isfinite(yr))
    _check(run_gpu(e, x, RAGGED_4096, cuda), yr)


# field -> CC of FxRack<2> (topology 0); the firmware topologies route per include/olfx.h
# OLFX_FR_TOPOLOGY: 1 takes the delay CCs 35-39, the reverb balance 34 and the voice-filter CCs 41-44
# (cutoff, resonance, type, drive) in place of 45-48, and no master volume; 2 the delay CCs; 3 the
# reverb balance; 4 the filter CCs 41-44
RACK_CC = {0: 35, 1: 36, 2: 39, 3: 37, 4: 38, 5: 34, 6: 45, 7: 46, 8: 48, 9: 47, 10: 7}
RACK_DELAY, RACK_FILTER = (0, 1, 2, 3, 4), (6, 7, 8, 9)


def _rack_route(topology, field):
    """The CC that reaches `field` of an instance with this topology, or None."""
    if topology == 0:
        return RACK_CC[field]
    if field in RACK_DELAY and topology in (1, 2):
        return RACK_CC[field]
    if field == 5 and topology in (1, 3):
        return RACK_CC[field]
    if field in RACK_FILTER and topology in (1, 4):
        return RACK_CC[field] - 45 + 41
    return None


def test_fxrack_corners_and_midi_extremes(cuda):
    """256 racks over all five topologies, fields 0-8 and the master volume each at a random end of
    what MIDI 0 / 127 map to (0 / 1, cutoffs 0 / 20000 Hz), every filter type: bit-exact against
    the oracle, finite on every instance.  The same corners driven through olfx_control with MIDI
    values 0 and 127, wherever the instance's topology takes the control, give the same bits."""
    import ol_dsp_amd as ofx
    n = 256
    rng = np.random.default_rng(23)
    ends = np.empty((11, 2), np.float32)
    for f, cc in RACK_CC.items():
        ends[f] = [ofx.control_map("fxrack", cc, v)[1] for v in (0, 127)]
    assert np.all(ends[[0, 1, 2, 4, 5, 7, 8, 10]] == [0.0, 1.0]) and np.all(ends[[3, 6]] == [0.0, 20000.0])
    pick = rng.integers(0, 2, (11, n))
    p = np.where(pick == 1, ends[:, 1:], ends[:, :1]).astype(np.float32)
    ftype = rng.integers(0, 5, n)
    p[9] = ftype
    topo = np.arange(n) % 5
    p = np.concatenate([p, topo[None, :].astype(np.float32)], 0)
    x = fast_noise(n, 4096, seed=23)
    e, ref = _fxrack_pair(n, p)
    yr = ref.process(x, threads=8)
    print(f"\nfxrack corners: largest oracle sample {np.abs(yr).max():.1f}")
    assert np.all(np.isfinite(yr))
    y = run_gpu(e, x, RAGGED_4096, cuda)
    _check(y, yr)
    # the control path: the topology first (it decides the routing), then one CC per field
    type_midi = {t: next(v for v in range(128) if ofx.control_map("fxrack", 47, v)[1] == t) for t in range(5)}
    e2 = engine("fxrack", n)
    e2.set_params("topology", p[11:])
    evs, direct = [], 0
    for i in range(n):
        for f in range(11):
            cc = _rack_route(int(topo[i]), f)
            if cc is None:
                e2.set_param(i, f, float(p[f, i]))
                direct += 1
            else:
                evs.append((i, cc, type_midi[int(ftype[i])] if f == 9 else 127 * int(pick[f, i])))
    e2.control(evs)
    assert len(evs) > 0.5 * 11 * n
    for f in range(12):
        assert [e2.get_param(i, f) for i in range(n)] == p[f].tolist(), f
    y2 = run_gpu(e2, x, RAGGED_4096, cuda)
    assert bits_equal(y, y2), first_mismatch(y, y2)


@pytest.mark.parametrize("kind", VOICES)
def test_voice_corners(cuda, rcp_table, kind):
    """256 voices, each of the 16 config fields at a random end of its range (cutoff 0 / 20000 Hz,
    the rest 0 / 1: resonance 1, zero-length envelope segments, amounts 0 and 1), notes from the
    ends of the MIDI range: NoteOn, 1,024 frames in ragged blocks, NoteOff, 1,024 frames, bit-exact
    against the oracle's kernel arithmetic.  The oracle is finite throughout and at least a third of
    the voices sound (measured: 50 % of the Svf voices, 37 % of the Moog voices; half of all voices
    have amp amount 0)."""
    n = 256
    rng = np.random.default_rng(33)
    cfg = rng.integers(0, 2, (16, n)).astype(np.float32)
    cfg[0] *= 20000.0
    notes = [int(v) for v in rng.choice([0, 1, 21, 60, 108, 127], n)]
    e = engine(kind, n)
    ref = O.Voice(n, moog=kind == "voice_moog", kernel_arith=True)
    e.set_params(0, cfg)
    for i in range(n):
        ref.config(i, cfg[:, i])
    ys, yrs = [], []
    for on in (1, 0):
        e.note_events([(i, on, notes[i]) for i in range(n)])
        for i in range(n):
            ref.note(i, bool(on), notes[i])
        ys += [_voice_run(e, b, cuda) for b in (256, 4, 100, 300, 364)]
        yrs.append(ref.process(1024))
    y, yr = np.concatenate(ys, 1), np.concatenate(yrs, 1)
    sounding = float(np.mean(np.any(yr[0] != 0, axis=0)))
    print(f"\n{kind} corners: {100 * sounding:.0f} % of the oracle's voices non-silent")
    assert np.all(np.isfinite(yr)) and sounding >= 1 / 3
    assert voice_bits_equal(y, yr), first_mismatch(y, yr)


# --------------------------------------------------------------------------------- containment
GUARD = 64
SENTINEL = 0x7FC5A5A5                      # a quiet NaN with a recognisable payload


def _guarded_torch(count, offset, cuda):
    """(whole int32 buffer, float view of `count` floats): 64 guard floats on each side (one more
    in front with offset 1, which takes the view off 16-byte alignment), all sentinel."""
    import torch
    buf = torch.full((GUARD + offset + count + GUARD,), SENTINEL, dtype=torch.int32, device=cuda)
    view = buf.view(torch.float32)[GUARD + offset:GUARD + offset + count]
    assert (view.data_ptr() % 16 == 0) == (offset == 0)
    return buf, view


def _guarded_numpy(count, offset):
    buf = np.full(GUARD + offset + count + GUARD, SENTINEL, np.int32)
    return buf, buf.view(np.float32)[GUARD + offset:GUARD + offset + count]


def _assert_contained(buf, offset, count):
    """The guards still hold the sentinel and every float between them was overwritten."""
    bits = buf.cpu().numpy() if hasattr(buf, "cpu") else buf
    lo = GUARD + offset
    assert np.all(bits[:lo] == SENTINEL), "write in front of out"
    assert np.all(bits[lo + count:] == SENTINEL), "write past the end of out"
    assert not np.any(bits[lo:lo + count] == SENTINEL), "output floats left unwritten"


def _contain_setup(kind, n):
    """(engine, oracle(x or frame count)) for any kind; voices sound (NoteOn) and stay finite."""
    if kind in VOICES:
        rng = np.random.default_rng(31)
        cfg = voice_configs(rng, n)
        cfg[2] *= 0.25                       # moderate Svf drive: finite, so the sentinel NaN is unmistakable
        e = engine(kind, n)
        ref = O.Voice(n, moog=kind == "voice_moog", kernel_arith=True)
        e.set_params(0, cfg)
        e.note_events([(i, 1, 40 + i % 50) for i in range(n)])
        for i in range(n):
            ref.config(i, cfg[:, i])
            ref.note(i, True, 40 + i % 50)
        return e, lambda x: ref.process(x.shape[1])
    return _pair(kind, n, _params(kind, n))


CONTAIN_CALLS = [4, 20, 260]


@pytest.mark.parametrize("n", [1, 63, 70, 72])
@pytest.mark.parametrize("kind", EFFECTS + ["fxrack0"] + VOICES)
def test_device_buffers_contained(cuda, rcp_table, kind, n):
    """in and out are views into larger device tensors, 64 guard floats on each side, guards and
    output filled with a NaN sentinel; calls of 4, 20 and 260 frames, once with 16-byte aligned
    views and once offset by one float (the per-lane I/O path).  The output guards' bits are
    unchanged, every output float was overwritten, and the result equals the oracle -- so no guard
    float around the input (NaN) was used either.  All accesses stay inside the test's tensors."""
    import torch
    voice = kind in VOICES
    x = fast_noise(n, sum(CONTAIN_CALLS), seed=n)
    for offset in (0, 1):
        e, oracle = _contain_setup(kind, n)
        ich, och = e.info.in_channels, e.info.out_channels
        yr = oracle(x)
        outs, f0 = [], 0
        for b in CONTAIN_CALLS:
            obuf, oview = _guarded_torch(och * b * n, offset, cuda)
            xin = None
            if not voice:
                _, iview = _guarded_torch(ich * b * n, offset, cuda)
                xin = iview.view(ich, b, n)
                xin.copy_(torch.from_numpy(np.ascontiguousarray(x[:, f0:f0 + b])))
            e.process(xin, out=oview.view(och, b, n))
            torch.cuda.synchronize()
            _assert_contained(obuf, offset, och * b * n)
            outs.append(oview.view(och, b, n).cpu().numpy())
            f0 += b
        y = np.concatenate(outs, 1)
        if voice:
            assert np.all(np.isfinite(yr)) and voice_bits_equal(y, yr), first_mismatch(y, yr)
        else:
            _check(y, yr)


@pytest.mark.parametrize("kind", EFFECTS + ["fxrack0"] + VOICES)
def test_host_buffers_contained(cuda, rcp_table, kind):
    """The same through OLFX_IO_HOST: numpy views into larger arrays with sentinel guards."""
    n = 70
    voice = kind in VOICES
    x = fast_noise(n, sum(CONTAIN_CALLS), seed=n)
    for offset in (0, 1):
        e, oracle = _contain_setup(kind, n)
        ich, och = e.info.in_channels, e.info.out_channels
        yr = oracle(x)
        outs, f0 = [], 0
        for b in CONTAIN_CALLS:
            obuf, oview = _guarded_numpy(och * b * n, offset)
            xin = None
            if not voice:
                _, iview = _guarded_numpy(ich * b * n, offset)
                xin = iview.reshape(ich, b, n)
                xin[...] = x[:, f0:f0 + b]
            out = oview.reshape(och, b, n)
            assert e.process(xin, out=out) is out and np.shares_memory(out, obuf)
            _assert_contained(obuf, offset, och * b * n)
            outs.append(out.copy())
            f0 += b
        y = np.concatenate(outs, 1)
        if voice:
            assert np.all(np.isfinite(yr)) and voice_bits_equal(y, yr), first_mismatch(y, yr)
        else:
            _check(y, yr)


@pytest.mark.parametrize("sizes", [[8], [4, 12, 0, 8, 20], [1, 7, 0, 12, 3]])
def test_mix_buffers_contained(cuda, sizes):
    """olfx_mix over 509 frames (the four-frame step and its scalar tail) with sentinel guards
    around bus_out and around the voice samples, buses that are runs of 4 voices (voice_mix_v4) and
    runs that are not (voice_mix_v2), aligned and offset by one float, device and host: the guards
    keep their bits and the buses equal Polyvoice's in-order adds into a non-zero bus buffer."""
    import torch
    n, frames = 300, 509
    rng = np.random.default_rng(37)
    buses, v, k = [], 0, 0
    while v < n:
        m = min(sizes[k % len(sizes)], n - v)
        buses.append(list(range(v, v + m)))
        v += m
        k += 1
    e = engine("voice", n)
    e.mix_config(buses)
    nb = len(buses)
    voices = rng.standard_normal((frames, n)).astype(np.float32)
    init = rng.standard_normal((frames, nb)).astype(np.float32)
    want = O.mix_ref(voices, buses, init)
    for offset in (0, 1):
        _, vview = _guarded_torch(frames * n, offset, cuda)
        vview.copy_(torch.from_numpy(voices.ravel()))
        bbuf, bview = _guarded_torch(frames * nb, offset, cuda)
        bview.copy_(torch.from_numpy(init.ravel()))
        e.mix(vview.view(1, frames, n), bview.view(frames, nb))
        torch.cuda.synchronize()
        _assert_contained(bbuf, offset, frames * nb)
        assert bits_equal(bview.view(frames, nb).cpu().numpy(), want)
        _, hv = _guarded_numpy(frames * n, offset)
        hv[:] = voices.ravel()
        hbuf, hb = _guarded_numpy(frames * nb, offset)
        hb[:] = init.ravel()
        e.mix(hv.reshape(1, frames, n), hb.reshape(frames, nb))
        _assert_contained(hbuf, offset, frames * nb)
        assert bits_equal(hb.reshape(frames, nb), want)
