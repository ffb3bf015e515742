"""The references of tests/edge_fused_cases.py alone, on the CPU: every case that
tests/test_gpu_edges_fused.py runs on the engine gives a reference with the edge the case is about --
the subnormal and non-finite shares, the poisoned instances non-finite and their neighbours finite,
the corners finite and audible, the containment runs finite, the other sample rates different from
48 kHz.  A condition that fails here means the case builder is wrong, not the bound."""
import numpy as np
import pytest

import edge_fused_cases as C
import synth_ref as SYN
from helpers import same_bits_or_nan
from test_gpu_sampler import assignments


@pytest.fixture(scope="module", autouse=True)
def rcp():
    SYN.install_rcp()
    yield
    SYN.remove_rcp()


# ----------------------------------------------------------------------------------- A. plate rack
@pytest.mark.parametrize("n", C.PLATE_N)
@pytest.mark.parametrize("signal", C.PLATE_SIGNALS)
def test_plate_signals(signal, n):
    p, x = C.plate_signal_case(n, signal)
    assert np.all(np.isfinite(x))
    C.plate_signal_condition(n, signal, C.plate_reference(p, x))


@pytest.mark.parametrize("n", C.PLATE_N)
def test_plate_poisoned(n):
    """All five poisoned instances non-finite, every other instance as on the clean input and finite."""
    p, x, xp, bad = C.plate_poison_case(n)
    yr = C.plate_reference(p, xp)
    C.plate_poison_condition(n, yr, bad)
    yc = C.plate_reference(p, x)
    clean = np.setdiff1d(np.arange(n), bad)
    assert np.all(np.isfinite(yc)) and same_bits_or_nan(yr[:, :, clean], yc[:, :, clean])


def test_plate_corners():
    n, p, x = C.plate_corner_case()
    assert set(np.unique(p[:9])) <= {0.0, 1.0, 20000.0} and set(np.unique(p[9])) == {0.0, 1.0, 2.0, 3.0, 4.0}
    assert set(np.unique(p[10:])) == {0.0, 1.0} and x.shape == (2, 2048, n)
    C.plate_corner_condition(C.plate_reference(p, x))


@pytest.mark.parametrize("n", C.CONTAIN_N)
def test_plate_containment_runs_are_finite(n):
    C.finite_and_sounding(C.plate_reference(*C.plate_contain_case(n)))


@pytest.mark.parametrize("sr", C.RATES)
def test_plate_rates(sr):
    n, p, x = C.plate_rate_case(sr)
    assert x.shape == (2, 3000, 70)
    C.plate_rate_condition(sr, C.plate_reference(p, x, sr), C.plate_reference(p, x))


# --------------------------------------------------------------------------------- B. sample voice
@pytest.mark.parametrize("n", C.VOICE_N)
@pytest.mark.parametrize("name", C.BANKS)
def test_voice_banks(name, n):
    bank = C.edge_bank(name)
    assert all(np.all(np.isfinite(s)) for s in bank)
    C.voice_bank_condition(n, name, C.voice_reference(n, C.voice_config(n), bank, C.voice_script(n)))


@pytest.mark.parametrize("n", C.VOICE_N)
def test_voice_poisoned_bank(n):
    """The voices on a poisoned sample go non-finite; the others equal the clean-bank run."""
    cfg, script = C.voice_config(n), C.voice_script(n)
    yr = C.voice_reference(n, cfg, C.poisoned_bank(), script)
    C.voice_poison_condition(n, yr)
    yc = C.voice_reference(n, cfg, C.clean_bank(), script)
    _, clean = C.voice_poison_split(n)
    assert np.array_equal(yr[:, :, clean].view(np.uint32), yc[:, :, clean].view(np.uint32))


def test_voice_corners():
    n, cfg, script = C.voice_corner_case()
    assert set(np.unique(cfg)) == {0.0, 1.0, 20000.0}
    yr = C.voice_reference(n, cfg, C.clean_bank(), script)
    assert yr.shape == (1, 2048, n)
    C.voice_corner_condition(yr)


@pytest.mark.parametrize("n", C.CONTAIN_N)
def test_voice_containment_runs_are_finite(n):
    C.finite_and_sounding(C.voice_reference(n, C.voice_config(n), C.clean_bank(), C.voice_contain_script(n)))


@pytest.mark.parametrize("sr", C.RATES)
def test_voice_rates(sr):
    n = 70
    args = (n, C.voice_config(n), C.clean_bank(), C.voice_script(n))
    C.voice_rate_condition(C.voice_reference(*args, sample_rate=sr), C.voice_reference(*args))


def test_voice_cases_use_the_whole_bank():
    """Every sample of the bank, the four poisoned ones included, and OLFX_NO_SAMPLE are assigned at
    both sizes."""
    for n in C.VOICE_N:
        assert {r[1] for r in assignments(n)} == set(range(12)) | {None}


# ------------------------------------------------------------------------------------------ C. synth
@pytest.mark.parametrize("n,P", C.SYNTH_CORNER_SHAPES)
def test_synth_half_corners(n, P):
    script = C.synth_corner_script(n, P)
    p = script[0][1]
    at_corner = np.isin(p[:SYN.NV + 9], [0.0, 1.0, 20000.0])
    assert 0.4 < at_corner.mean() < 0.6                  # half the fields at an end of their range
    assert sum(s[1] for s in script if s[0] == "block") == 2048
    yr, ref = SYN.run_ref(script, n, P, threads=8)
    assert len(ref.trace) == 2 and np.all(ref.trace[0] != 0) and np.all(ref.trace[1][:, 0] == 0)
    C.synth_corner_condition(n, P, yr)


@pytest.mark.parametrize("n,P", C.SYNTH_CONTAIN_SHAPES)
def test_synth_containment_runs_are_finite(n, P):
    yr, _ = SYN.run_ref(C.synth_contain_script(n, P), n, P, threads=8)
    C.finite_and_sounding(yr)


@pytest.mark.parametrize("sr", C.RATES)
def test_synth_rates(sr):
    script, n = C.synth_rate_script(), C.SYNTH_RATE_N
    yr, _ = SYN.run_ref(script, n, 4, threads=8, sample_rate=sr)
    yr48, _ = SYN.run_ref(script, n, 4, threads=8)
    C.synth_rate_condition(yr, yr48)
