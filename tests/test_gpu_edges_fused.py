"""GPU edges of the three fused kinds: platerack_block_v1, sampler_block_v1 and synth_block_v1 on the
questions tests/test_gpu_edges.py puts to the older kernels -- flushes to zero, overflow, a NaN
crossing from one instance's queue column, mirrored padding lane or transposed ring column to a
neighbour's, every parameter corner, one float written outside `out`, a sample-rate constant left at
48000.  The cases, their references and the condition each reference must meet are
tests/edge_fused_cases.py (held on the CPU by tests/test_edge_fused_ref.py); every test here asserts
that condition again before it compares, and prints the shares (pytest -s).

Comparators: the plate rack against its unfused fp32 reference with helpers.same_bits_or_nan; the
sample voice and the synth against their kernel-arithmetic references with synth_ref.bits_equal (the
same finite mask, the same bits wherever the reference is finite).

The synth has no audio input and its setters refuse non-finite values, so it has no signal and no
poison case."""
import numpy as np
import pytest

import edge_fused_cases as C
import ol_dsp_amd as ofx
import sampler_ref as SMP
import synth_ref as SYN
from helpers import EDGE_BLOCKS, bits_equal, first_mismatch, first_mismatch_or_nan, same_bits_or_nan
from test_gpu_edges import CONTAIN_CALLS, _assert_contained, _guarded_numpy, _guarded_torch
from test_gpu_parity import engine, run_gpu
from test_gpu_sampler import Trio, assignments, cat
from test_gpu_synth import run_engine

pytestmark = pytest.mark.gpu


def _check(y, yr):
    assert same_bits_or_nan(y, yr), first_mismatch_or_nan(y, yr)


def _check_k(y, yr):
    assert SYN.bits_equal(y, yr), first_mismatch(y, yr)


def _contained_calls(e, x, n, offset, cuda, host):
    """CONTAIN_CALLS on views into larger buffers, 64 sentinel floats on each side of `in` (x, or
    None for a kind without input) and of `out`, 16-byte aligned (offset 0) or one float off: after
    every call the output's guards hold their bits and every output float was written.  Returns the
    output [och][frames][n]."""
    import torch
    och = e.info.out_channels
    outs, f0 = [], 0
    for b in CONTAIN_CALLS:
        xin = None
        if host:
            obuf, oview = _guarded_numpy(och * b * n, offset)
            out = oview.reshape(och, b, n)
            if x is not None:
                _, iview = _guarded_numpy(x.shape[0] * b * n, offset)
                xin = iview.reshape(x.shape[0], b, n)
                xin[...] = x[:, f0:f0 + b]
            assert e.process(xin, out=out) is out and np.shares_memory(out, obuf)
            got = out.copy()
        else:
            obuf, oview = _guarded_torch(och * b * n, offset, cuda)
            if x is not None:
                _, iview = _guarded_torch(x.shape[0] * b * n, offset, cuda)
                xin = iview.view(x.shape[0], b, n)
                xin.copy_(torch.from_numpy(np.ascontiguousarray(x[:, f0:f0 + b])))
            e.process(xin, out=oview.view(och, b, n))
            torch.cuda.synchronize()
            got = oview.view(och, b, n).cpu().numpy()
        _assert_contained(obuf, offset, och * b * n)
        outs.append(got)
        f0 += b
    return np.concatenate(outs, 1)


# ----------------------------------------------------------------------------------- A. plate rack
def _plate(n, p, sample_rate=48000.0):
    e = engine("platerack", n, sample_rate=sample_rate)
    e.set_params(0, p)
    return e


@pytest.mark.parametrize("n", C.PLATE_N)
@pytest.mark.parametrize("signal", C.PLATE_SIGNALS)
def test_plate_signal_edges(cuda, signal, n):
    """helpers.edge_signals through n = 70 (the last group's second delay wave has no instance and
    publishes zeros) and n = 100 (it has four), a partly filled first delay wave and padding lanes that
    mirror instance n-1 in the filter and plate waves; 3,072 frames in ragged calls.  Conditions on the
    reference (edge_fused_cases.plate_signal_condition), with the shares this file prints at n = 70 /
    n = 100: x 2^-130 all of the non-zero samples subnormal (a flush in the delay, the plate, the
    balance mix or the filter shows as zeros against them); x 2^100 50.0 / 50.0 % and x 2^127
    50.6 / 50.7 % non-finite, all of channel 0; the burst finite with a tail past frame 2000;
    -0.0, +1 and alternating +-1 bit for bit, the sign of zero included."""
    p, x = C.plate_signal_case(n, signal)
    yr = C.plate_reference(p, x)
    C.plate_signal_condition(n, signal, yr)
    e = _plate(n, p)
    y = run_gpu(e, x, EDGE_BLOCKS, cuda)
    assert e.kernel_name == "platerack_block_v1"
    _check(y, yr)


@pytest.mark.parametrize("n", C.PLATE_N)
def test_plate_poisoned_instances_stay_isolated(cuda, n):
    """Single NaN / +-Inf input samples in instances 0, 5, 63, 64 and n-1 (helpers.poison_table), each
    on a channel its topology reads: all five are non-finite in the reference; (a) the whole output
    equals the reference; (b) every other instance is bit-identical to a second GPU run on the clean
    input, which is finite -- no wave read a neighbour's queue column, a padding lane's copy of
    instance n-1 or the zeros of an empty wave into another instance, not even times a zero gain."""
    p, x, xp, bad = C.plate_poison_case(n)
    yr = C.plate_reference(p, xp)
    C.plate_poison_condition(n, yr, bad)
    y = run_gpu(_plate(n, p), xp, EDGE_BLOCKS, cuda)
    _check(y, yr)
    yc = run_gpu(_plate(n, p), x, EDGE_BLOCKS, cuda)
    clean = np.setdiff1d(np.arange(n), bad)
    assert np.all(np.isfinite(yc))
    assert bits_equal(y[:, :, clean], yc[:, :, clean]), first_mismatch(y[:, :, clean], yc[:, :, clean])


def test_plate_corners(cuda):
    """256 plate racks: the rack's fields at the ends MIDI 0 / 127 map to, every filter type, both
    topologies, the plate's setters from {0, 1}^7 (pre-delays 0 and 4800 in one group: gather mode).
    The reference is finite on every instance (largest sample 43.4); bit-exact."""
    n, p, x = C.plate_corner_case()
    yr = C.plate_reference(p, x)
    C.plate_corner_condition(yr)
    _check(run_gpu(_plate(n, p), x, C.PLATE_CORNER_BLOCKS, cuda), yr)


def _plate_contained(cuda, n, host):
    p, x = C.plate_contain_case(n)
    yr = C.plate_reference(p, x)
    C.finite_and_sounding(yr)
    for offset in (0, 1):
        _check(_contained_calls(_plate(n, p), x, n, offset, cuda, host), yr)


@pytest.mark.parametrize("n", C.CONTAIN_N)
def test_plate_device_buffers_contained(cuda, n):
    """_contained_calls around `in` and `out`, aligned and one float off (the per-lane I/O path), at
    n = 1, 63, 70, 72: guards intact, every output float written, the output equal to the (finite)
    reference -- so no guard float of `in` was used."""
    _plate_contained(cuda, n, host=False)


def test_plate_host_buffers_contained(cuda):
    """The same through host pointers at n = 70."""
    _plate_contained(cuda, 70, host=True)


@pytest.mark.parametrize("sr", C.RATES)
def test_plate_at_other_sample_rates(cuda, sr):
    """44.1 and 96 kHz (DelayFx's time scale and the Svf's frequency map follow the rate; the plate's
    delays are in samples): bit-exact against PlateRack(n, sample_rate=sr), whose output is finite,
    non-zero and not the 48 kHz reference's."""
    n, p, x = C.plate_rate_case(sr)
    yr = C.plate_reference(p, x, sr)
    C.plate_rate_condition(sr, yr, C.plate_reference(p, x))
    _check(run_gpu(_plate(n, p, sr), x, C.PLATE_RATE_BLOCKS, cuda), yr)


# --------------------------------------------------------------------------------- B. sample voice
class RateTrio(Trio):
    """test_gpu_sampler.Trio at another sample rate."""

    def __init__(self, n, cuda, sample_rate):
        self.n, self.cuda = n, cuda
        self.e = ofx.Engine("voice_sample", n, sample_rate=sample_rate)
        self.k = SMP.SamplerVoices(n, sample_rate=sample_rate, kernel_arith=True)
        self.u = SMP.SamplerVoices(n, sample_rate=sample_rate)
        self.refs = (self.k, self.u)


def _voices(t, cfg, bank, script):
    """The case on a Trio: (engine output, kernel-arithmetic reference)."""
    got, wk, _ = cat(C.drive_voices(t, cfg, bank, assignments(t.n), script))
    assert t.e.kernel_name == "sampler_block_v1"
    return got, wk


@pytest.mark.parametrize("n", C.VOICE_N)
@pytest.mark.parametrize("name", C.BANKS)
def test_voice_bank_edges(cuda, rcp_table, name, n):
    """The bank scaled by 2^-130, 2^100 and 2^127 (exact), all -0.0 and all +1, every sample length and
    loop mode of test_gpu_sampler.assignments, n = 70 and 72; NoteOn, 580 ragged frames, NoteOff, 256.
    On the NoteOn blocks the reference is 100 % subnormal where non-zero (x 2^-130: a flush between the
    bank load, the staging, the transposed ring and the Svf shows as zeros) and 92.7 / 92.9 %
    non-finite (x 2^100 and x 2^127)."""
    t = Trio(n, cuda, configure=False)
    got, wk = _voices(t, C.voice_config(n), C.edge_bank(name), C.voice_script(n))
    C.voice_bank_condition(n, name, wk)
    _check_k(got, wk)


@pytest.mark.parametrize("n", C.VOICE_N)
def test_voice_poisoned_bank_stays_in_its_voices(cuda, rcp_table, n):
    """Single NaN / +-Inf frames in four samples of the bank (lengths 1, 63, 256, 1000): the voices that
    play them go non-finite (28 of 29 at n = 70, 29 of 30 at 72; one loops inside sample 5 short of its
    frame 62); the output equals the reference; and every voice on another sample or on none (41 / 42)
    is finite and bit-identical to a GPU run with the clean bank.  A wrong column or ballot bit of the
    64 x 64 transposed ring write, or a gather off by a frame, leaks a neighbour's frame."""
    cfg, script = C.voice_config(n), C.voice_script(n)
    got, wk = _voices(Trio(n, cuda, configure=False), cfg, C.poisoned_bank(), script)
    C.voice_poison_condition(n, wk)
    _check_k(got, wk)
    clean_got, clean_wk = _voices(Trio(n, cuda, configure=False), cfg, C.clean_bank(), script)
    _, clean = C.voice_poison_split(n)
    assert np.all(np.isfinite(clean_got)) and np.all(np.isfinite(got[:, :, clean]))
    _check_k(clean_got, clean_wk)
    assert bits_equal(got[:, :, clean], clean_got[:, :, clean]), first_mismatch(got[:, :, clean], clean_got[:, :, clean])


def test_voice_sample_corners(cuda, rcp_table):
    """256 sample voices with test_voice_corners' configurations (every field at an end of its range),
    notes from the ends of the MIDI range: NoteOn, 1,024 ragged frames, NoteOff, 1,024 more.  The
    reference is finite and 48 % of its voices sound; bit-exact."""
    n, cfg, script = C.voice_corner_case()
    got, wk = _voices(Trio(n, cuda, configure=False), cfg, C.clean_bank(), script)
    C.voice_corner_condition(wk)
    _check_k(got, wk)


def _voices_contained(cuda, n, host):
    script = C.voice_contain_script(n)
    for offset in (0, 1):
        t = Trio(n, cuda, configure=False)
        C.drive_voices(t, C.voice_config(n), C.clean_bank(), assignments(n), script[:1])
        got = _contained_calls(t.e, None, n, offset, cuda, host)
        wk = np.concatenate([t.k.process(b) for b in CONTAIN_CALLS], 1)
        C.finite_and_sounding(wk)
        _check_k(got, wk)


@pytest.mark.parametrize("n", C.CONTAIN_N)
def test_voice_sample_device_buffers_contained(cuda, rcp_table, n):
    """_contained_calls with in = None and guards around `out`, every voice sounding (NoteOn)."""
    _voices_contained(cuda, n, host=False)


def test_voice_sample_host_buffers_contained(cuda, rcp_table):
    _voices_contained(cuda, 70, host=True)


@pytest.mark.parametrize("sr", C.RATES)
def test_voice_sample_at_other_sample_rates(cuda, rcp_table, sr):
    """44.1 and 96 kHz: bit-exact against SamplerVoices(n, sample_rate=sr, kernel_arith=True), which
    differs from the 48 kHz reference (the envelopes' and the Svf's rates; the cursor steps one frame
    per output frame whatever the rate)."""
    n = 70
    cfg, script = C.voice_config(n), C.voice_script(n)
    got, wk = _voices(RateTrio(n, cuda, sr), cfg, C.clean_bank(), script)
    C.voice_rate_condition(wk, C.voice_reference(n, cfg, C.clean_bank(), script))
    _check_k(got, wk)


# ------------------------------------------------------------------------------------------ C. synth
@pytest.mark.parametrize("n,P", C.SYNTH_CORNER_SHAPES)
def test_synth_half_corners(cuda, rcp_table, n, P):
    """256 instruments of 4 voices and 70 of 8: each of the 28 fields at its corner with probability
    1/2, else at an interior value; notes from the ends and the middle of the MIDI range on every voice,
    1,024 ragged frames, a NoteOff of each instrument's first note, 1,024 more.  The reference is finite
    with both channels non-zero on 49 % / 61 % of the instruments; bit-exact, and Engine.playing equals
    the rule's table after both event steps."""
    script = C.synth_corner_script(n, P)
    yr, ref = SYN.run_ref(script, n, P, threads=8)
    C.synth_corner_condition(n, P, yr)
    y, _ = run_engine(script, n, P, cuda, trace=ref.trace)
    _check_k(y, yr)


def _synth_contained(cuda, n, P, host):
    script = C.synth_contain_script(n, P)
    yr, _ = SYN.run_ref(script, n, P, threads=8)
    C.finite_and_sounding(yr)
    for offset in (0, 1):
        e = ofx.Engine("synth", n, voices=P)
        e.set_params(0, script[0][1])
        e.note_events(script[1][1])
        y = _contained_calls(e, None, n, offset, cuda, host)
        assert e.kernel_name == "synth_block_v1"
        _check_k(y, yr)


@pytest.mark.parametrize("n,P", C.SYNTH_CONTAIN_SHAPES)
def test_synth_device_buffers_contained(cuda, rcp_table, n, P):
    """_contained_calls with in = None and guards around the two output planes: P = 4 at n = 1, 63, 70,
    72, and P = 8 (the wave that runs two voices) at n = 70."""
    _synth_contained(cuda, n, P, host=False)


def test_synth_host_buffers_contained(cuda, rcp_table):
    _synth_contained(cuda, 70, 4, host=True)


@pytest.mark.parametrize("sr", C.RATES)
def test_synth_at_other_sample_rates(cuda, rcp_table, sr):
    """44.1 and 96 kHz, 33 instruments of 4 voices on synth_ref's ragged_frames script: the reference is
    finite with both channels non-zero on every instrument and is not the 48 kHz one; bit-exact."""
    script, n = C.synth_rate_script(), C.SYNTH_RATE_N
    yr, _ = SYN.run_ref(script, n, 4, threads=8, sample_rate=sr)
    C.synth_rate_condition(yr, SYN.run_ref(script, n, 4, threads=8)[0])
    y, _ = run_engine(script, n, 4, cuda, e=ofx.Engine("synth", n, voices=4, sample_rate=sr))
    _check_k(y, yr)
