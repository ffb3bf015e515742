"""The edge cases of the three fused kinds -- platerack, voice_sample, synth -- as data: inputs,
parameters, banks and scripts, with each case's reference and the condition that reference must meet.

tests/test_edge_fused_ref.py runs every reference alone on the CPU and asserts its condition;
tests/test_gpu_edges_fused.py runs the same cases on the engine and asserts the same condition before
it compares, so no case passes on the GPU without the edge it is about.  The references are
  plate rack     platerack_ref.PlateRack (the unfused fp32 composition), helpers.same_bits_or_nan;
  sample voice   sampler_ref.SamplerVoices(kernel_arith=True), synth_ref.bits_equal;
  synth          synth_ref.Synth, synth_ref.bits_equal.
The last two need the committed v_rcp_f32 table installed (the GPU tests' rcp_table fixture, or
synth_ref.install_rcp() / remove_rcp() on the CPU).
"""
from __future__ import annotations

import numpy as np

import platerack_ref as PR
import sampler_ref as SMP
import synth_ref as SYN
from helpers import (EDGE_BLOCKS, EDGE_FRAMES, edge_signals, fast_noise, nonfinite_share, poison_table, poisoned,
                     subnormal_share)
from ol_dsp_amd import workload
from test_gpu_edges import CONTAIN_CALLS
from test_gpu_platerack import PRE, TOPO, params
from test_gpu_sampler import LENGTHS, NOTE_OFF, NOTE_ON, assignments

RATES = [44100.0, 96000.0]
RAGGED_1024 = [256, 4, 100, 300, 364]
CONTAIN_FRAMES = sum(CONTAIN_CALLS)


def _say(text: str) -> None:
    print("\n" + text)


def _sounding(y: np.ndarray) -> np.ndarray:
    """[channels][n]: the instance has a non-zero sample on the channel."""
    return np.any(y != 0, axis=1)


def _rack_corners(rng: np.random.Generator, n: int):
    """[11][n]: the rack's fields 0-8 and 10 at a random end of what MIDI 0 / 127 map to (0 / 1, the
    two cutoffs 0 / 20000 Hz) and a random filter type 0..4 in row 9, drawn as
    test_gpu_edges.test_fxrack_corners_and_midi_extremes draws them."""
    ends = np.tile(np.float32([0.0, 1.0]), (11, 1))
    ends[[3, 6]] = [0.0, 20000.0]
    pick = rng.integers(0, 2, (11, n))
    p = np.where(pick == 1, ends[:, 1:], ends[:, :1]).astype(np.float32)
    p[9] = rng.integers(0, 5, n)
    return p


def _voice_corners(rng: np.random.Generator, n: int) -> np.ndarray:
    """[16][n] as test_gpu_edges.test_voice_corners: every field 0 / 1, the cutoff 0 / 20000 Hz."""
    cfg = rng.integers(0, 2, (16, n)).astype(np.float32)
    cfg[0] *= 20000.0
    return cfg


# ----------------------------------------------------------------------------------- A. plate rack
PLATE_N = [70, 100]          # 70: the last group's D1 wave has no instance; 100: it has four
PLATE_SIGNALS = ["subnormal", "burst", "loud100", "loud127", "negzero", "ones", "alternating"]
PLATE_CORNER_BLOCKS = [256, 4, 20, 1024, 300, 444]
PLATE_RATE_BLOCKS = [256, 4, 60, 1024, 300, 1356]
CONTAIN_N = [1, 63, 70, 72]


def plate_params(n: int) -> np.ndarray:
    """test_gpu_platerack.params(n, 40) with pre-delays of at most 96 samples.  The workload's (up to
    4800) hold the input out of the tank for longer than these runs: a NaN fed at frame 1000 under a
    pre-delay of 4295 leaves the reference finite for all 3072 frames."""
    p = params(n, 40)
    p[PRE] = np.random.default_rng(40).uniform(0, 0.02, n)
    return p


def plate_reference(p: np.ndarray, x: np.ndarray, sample_rate: float = 48000.0) -> np.ndarray:
    ref = PR.PlateRack(x.shape[2], sample_rate=sample_rate)
    ref.set_params(p)
    return ref.process(x, threads=8)


def plate_signal_case(n: int, signal: str):
    return plate_params(n), edge_signals(fast_noise(n, EDGE_FRAMES, seed=40))[signal]


def plate_signal_condition(n: int, signal: str, yr: np.ndarray) -> None:
    """subnormal: non-zero, at least half of the non-zero samples subnormal (measured 100 %);
    loud100 / loud127: at least 40 % non-finite (measured 50.0 % and 50.2-50.7 %, all of channel 0);
    burst: finite and non-zero after frame 2000, the plate's tail (subnormal share measured 0, none
    claimed); ones, alternating: finite and non-zero; negzero: the comparison alone."""
    sub, nonfin = subnormal_share(yr), nonfinite_share(yr)
    _say(f"platerack n={n} {signal}: reference subnormal share of non-zero {100 * sub:.1f} %, "
         f"non-finite share {100 * nonfin:.1f} %")
    if signal == "subnormal":
        assert np.any(yr != 0) and sub >= 0.5
    if signal in ("loud100", "loud127"):
        assert nonfin >= 0.40
    if signal == "burst":
        assert nonfin == 0 and np.any(yr[:, 2000:] != 0)
    if signal in ("ones", "alternating"):
        assert nonfin == 0 and np.any(yr != 0)


def plate_poison_case(n: int):
    """(params, clean input, poisoned input, the poisoned instances).  Topology 1 (the firmware path:
    channel 1 is a copy of channel 0) on instances 0 and 63, poisoned on channel 0; topology 0 on
    5, 64 and n-1, whose poison sits on channel 1, which topology 1 ignores."""
    p = plate_params(n)
    p[TOPO, [0, 63]] = 1.0
    p[TOPO, [5, 64, n - 1]] = 0.0
    x = fast_noise(n, EDGE_FRAMES, seed=40)
    return p, x, poisoned(x), sorted({i for _, _, i, _ in poison_table(n)})


def plate_poison_condition(n: int, yr: np.ndarray, bad) -> None:
    hit = sum(1 for i in bad if not np.all(np.isfinite(yr[:, :, i])))
    _say(f"platerack n={n} poisoned: {hit} of {len(bad)} poisoned instances non-finite in the reference, "
         f"non-finite share {100 * nonfinite_share(yr):.1f} %")
    assert len(bad) == 5 and hit == 5


def plate_corner_case():
    """(n, params, input): 256 instances; the rack's fields at the MIDI ends, every filter type,
    topology i % 2, the plate's seven setters from {0, 1}^7 (pre-delays 0 and 4800 in one group:
    gather mode)."""
    n = 256
    rng = np.random.default_rng(23)
    rack = _rack_corners(rng, n)
    topo = (np.arange(n) % 2)[None, :].astype(np.float32)
    plate = rng.integers(0, 2, (7, n)).astype(np.float32)
    p = np.concatenate([rack, topo, plate], 0)
    assert np.all(p[PRE] * np.float32(4800.0) < 65536.0) and {0.0, 1.0} == set(p[PRE, :64].tolist())
    return n, p, fast_noise(n, sum(PLATE_CORNER_BLOCKS), seed=23)


def plate_corner_condition(yr: np.ndarray) -> None:
    _say(f"platerack corners: largest reference sample {np.abs(yr).max():.1f}")
    assert np.all(np.isfinite(yr)) and np.any(yr != 0)


def plate_contain_case(n: int):
    return plate_params(n), fast_noise(n, CONTAIN_FRAMES, seed=n)


def plate_rate_case(sr: float):
    n = 70
    return n, plate_params(n), fast_noise(n, sum(PLATE_RATE_BLOCKS), seed=int(sr) % 1000)


def plate_rate_condition(sr: float, yr: np.ndarray, yr48: np.ndarray) -> None:
    """Finite and non-zero, and not what the 48 kHz reference gives: the rate cannot be ignored."""
    assert np.all(np.isfinite(yr)) and np.any(yr[0] != 0) and np.any(yr[1] != 0)
    assert np.any(yr.view(np.uint32) != yr48.view(np.uint32))


# --------------------------------------------------------------------------------- B. sample voice
VOICE_N = [70, 72]           # one voice past a workgroup, a partial last group, n % 4 both ways
BANKS = ["subnormal", "loud100", "loud127", "negzero", "ones"]
ON_BLOCKS = [256, 4, 20, 300]
ON_FRAMES = sum(ON_BLOCKS)
POISON_FRAMES = [(0, 0, np.nan), (5, 62, -np.inf), (9, 0, np.inf), (11, 5, np.nan)]   # (sample, frame, value)


def clean_bank():
    """test_gpu_sampler's bank."""
    return workload.sample_bank(LENGTHS, seed=11)


def edge_bank(name: str):
    f = np.float32
    scale = {"subnormal": f(2.0 ** -130), "loud100": f(2.0 ** 100), "loud127": f(2.0 ** 127)}
    if name in scale:
        return [s * scale[name] for s in clean_bank()]
    return [np.full_like(s, {"negzero": -0.0, "ones": 1.0}[name]) for s in clean_bank()]


def poisoned_bank():
    bank = [s.copy() for s in clean_bank()]
    for k, frame, v in POISON_FRAMES:
        assert frame < LENGTHS[k]
        bank[k][frame] = v
    return bank


class RefVoices:
    """The kernel-arithmetic reference alone behind test_gpu_sampler.Trio's surface."""

    def __init__(self, n: int, sample_rate: float = 48000.0):
        self.n = n
        self.k = SMP.SamplerVoices(n, sample_rate=sample_rate, kernel_arith=True)

    def config(self, p):
        for i in range(self.n):
            self.k.config(i, p[:, i])

    def bank(self, samples):
        self.k.sample_bank(samples)

    def voices(self, recs):
        self.k.sample_voices(recs)

    def events(self, evs):
        self.k.events(evs)

    def run(self, frames):
        return self.k.process(frames)


def voice_notes(n: int):
    return [40 + i % 50 for i in range(n)]


def voice_script(n: int, notes=None, on=ON_BLOCKS, off=(256,)):
    """NoteOn on every voice, the blocks of `on`, NoteOff on every voice, the blocks of `off`."""
    notes = voice_notes(n) if notes is None else notes
    return ([("events", [(i, NOTE_ON, notes[i]) for i in range(n)])] + [("block", b) for b in on]
            + [("events", [(i, NOTE_OFF, notes[i]) for i in range(n)])] + [("block", b) for b in off])


def voice_config(n: int) -> np.ndarray:
    return workload.instance_params("voice_sample", 0, n, 3)


def drive_voices(t, cfg, bank, recs, script) -> list:
    """The case on a Trio or a RefVoices: what each block's run() returned, in order."""
    t.config(cfg)
    t.bank(bank)
    t.voices(recs)
    out = []
    for step in script:
        if step[0] == "events":
            t.events(step[1])
        else:
            out.append(t.run(step[1]))
    return out


def voice_reference(n: int, cfg, bank, script, sample_rate: float = 48000.0) -> np.ndarray:
    return np.concatenate(drive_voices(RefVoices(n, sample_rate), cfg, bank, assignments(n), script), 1)


def voice_bank_condition(n: int, name: str, yr: np.ndarray) -> None:
    """On the NoteOn blocks: x 2^-130 at least half of the non-zero samples subnormal (measured
    100 %: a flush anywhere between the bank load, the transposed ring and the Svf shows as zeros);
    x 2^100 and x 2^127 at least 50 % non-finite (measured 92.7 % for both)."""
    on = yr[:, :ON_FRAMES]
    sub, nonfin = subnormal_share(on), nonfinite_share(on)
    _say(f"voice_sample n={n} bank {name}: reference subnormal share of non-zero {100 * sub:.1f} %, "
         f"non-finite share {100 * nonfin:.1f} %")
    if name == "subnormal":
        assert np.any(on != 0) and sub >= 0.5
    if name in ("loud100", "loud127"):
        assert nonfin >= 0.5


def voice_poison_split(n: int):
    """(voices assigned one of the four poisoned samples, every other voice)."""
    hot = {k for k, _, _ in POISON_FRAMES}
    bad = [r[0] for r in assignments(n) if r[1] in hot]
    return bad, [i for i in range(n) if i not in bad]


def voice_poison_condition(n: int, yr: np.ndarray) -> None:
    """At least 80 % of the voices that play a poisoned sample go non-finite (measured 28 of 29 at
    n = 70: one voice loops inside sample 5 without reaching frame 62); every other voice is finite."""
    bad, clean = voice_poison_split(n)
    hit = sum(1 for i in bad if not np.all(np.isfinite(yr[:, :, i])))
    _say(f"voice_sample n={n} poisoned bank: {hit} of {len(bad)} voices on a poisoned sample non-finite in the "
         f"reference, {len(clean)} voices on another sample or none")
    assert bad and hit >= 0.8 * len(bad)
    assert clean and np.all(np.isfinite(yr[:, :, clean]))


def voice_corner_case():
    """(n, configurations, script): test_voice_corners' draw; NoteOn, 1024 ragged frames, NoteOff, the
    same again."""
    n = 256
    rng = np.random.default_rng(33)
    cfg = _voice_corners(rng, n)
    notes = [int(v) for v in rng.choice([0, 1, 21, 60, 108, 127], n)]
    return n, cfg, voice_script(n, notes, RAGGED_1024, RAGGED_1024)


def voice_corner_condition(yr: np.ndarray) -> None:
    sounding = float(np.mean(_sounding(yr)[0]))
    _say(f"voice_sample corners: {100 * sounding:.0f} % of the reference's voices non-silent")
    assert np.all(np.isfinite(yr)) and sounding >= 1 / 3


def voice_contain_script(n: int):
    return [("events", [(i, NOTE_ON, voice_notes(n)[i]) for i in range(n)])] + [("block", b) for b in CONTAIN_CALLS]


def finite_and_sounding(yr: np.ndarray) -> None:
    """The containment runs: finite, so that the NaN sentinel is unmistakable, and not silent."""
    assert np.all(np.isfinite(yr)) and np.all(np.any(yr != 0, axis=(1, 2)))


def voice_rate_condition(yr: np.ndarray, yr48: np.ndarray) -> None:
    assert np.all(np.isfinite(yr)) and np.any(yr != 0)
    assert np.any(yr.view(np.uint32) != yr48.view(np.uint32))


# ------------------------------------------------------------------------------------------ C. synth
SYNTH_CORNER_SHAPES = [(256, 4), (70, 8)]
SYNTH_CONTAIN_SHAPES = [(1, 4), (63, 4), (70, 4), (72, 4), (70, 8)]       # P = 8: the wave that runs two voices
SYNTH_RATE_N = 33
FTYPE = SYN.NV + 9


def synth_corner_script(n: int, P: int):
    """Each of the 28 fields of each instrument at its corner value with probability 1/2 (voice fields
    as test_voice_corners, rack fields as the plate rack's corners, topology 1), else at the interior
    value of synth_ref.params(n, 35); the filter type is the corner matrix's integer.  (A full-corner
    draw leaves 10 % of the instruments audible: amp amount 0 and delay balance 1 with a one-second
    delay each silence half of them.)  Every voice gets a NoteOn from the ends and the middle of the
    MIDI range; 1024 ragged frames; a NoteOff of each instrument's first note; 1024 more."""
    rng = np.random.default_rng(35)
    corner = np.concatenate([_voice_corners(rng, n), _rack_corners(rng, n), np.ones((1, n), np.float32)], 0)
    interior = SYN.params(n, 35)
    assert corner.shape == interior.shape == (28, n)
    p = np.where(rng.random((28, n)) < 0.5, corner, interior).astype(np.float32)
    p[FTYPE] = corner[FTYPE]
    assert np.all(p[SYN.TOPOLOGY] == 1.0)
    notes = rng.choice([1, 21, 60, 108, 127], (n, P))
    s = [("params", p), ("events", [(i, SYN.EV_NOTE_ON, int(notes[i, v])) for i in range(n) for v in range(P)]),
         ("check_playing",)]
    s += [("block", b) for b in RAGGED_1024]
    s += [("events", [(i, SYN.EV_NOTE_OFF, int(notes[i, 0])) for i in range(n)]), ("check_playing",)]
    s += [("block", b) for b in RAGGED_1024]
    return s


def synth_corner_condition(n: int, P: int, yr: np.ndarray) -> None:
    """Finite, and both channels non-zero on at least a third of the instruments."""
    both = float(np.mean(np.all(_sounding(yr), axis=0)))
    _say(f"synth n={n} P={P} half-corners: both channels non-zero on {100 * both:.0f} % of the reference's "
         f"instruments, largest sample {np.abs(yr).max():.1f}")
    assert np.all(np.isfinite(yr)) and both >= 1 / 3


def synth_contain_script(n: int, P: int):
    return [("params", SYN.params(n, 5)), ("events", SYN.notes_on(n, P))] + [("block", b) for b in CONTAIN_CALLS]


def synth_rate_script():
    return SYN.script_ragged_frames(SYNTH_RATE_N)


def synth_rate_condition(yr: np.ndarray, yr48: np.ndarray) -> None:
    SYN.condition(yr)
    assert np.any(yr.view(np.uint32) != yr48.view(np.uint32))
