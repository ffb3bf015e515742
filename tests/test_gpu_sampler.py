"""OLFX_KIND_VOICE_SAMPLE (sampler_block_v1: sample playback -> Svf -> amp envelope) on the GPU against
tests/sampler_ref: bit-exact in its kernel arithmetic (with the committed v_rcp_f32 table), within
1e-5 of max(|ref|, rms) of its unfused arithmetic (the voice tests' tolerance, test_gpu_parity.py).

One bank for every test: seeded noise in [-0.5, 0.5), samples of 1, 3, 7, 8, 9, 63, 64, 65, 255,
256, 257 and 1000 frames, so later samples start at odd offsets in the caller's array and every
sample is shorter than, equal to or a little longer than the kernel's 64-frame fetch window."""
import numpy as np
import pytest

import ol_dsp_amd as ofx
import oracle as O
import sampler_ref as SR
from helpers import rel_err
from ol_dsp_amd import workload
from test_gpu_parity import VOICE_TOL

pytestmark = pytest.mark.gpu

LENGTHS = [1, 3, 7, 8, 9, 63, 64, 65, 255, 256, 257, 1000]
NOTE_OFF, NOTE_ON, GATE_ON, GATE_OFF, SET_FREQ = 0, 1, 2, 3, 4


@pytest.fixture(scope="module")
def bank():
    b = workload.sample_bank(LENGTHS, seed=11)
    assert all(x.min() >= -0.5 and x.max() <= 0.5 for x in b)
    return b


def loop_modes(L):
    """OneShot and the eight configurations of tests/golden/sample_reference_runs.json (recorded on a
    5-frame sample), scaled to an L-frame sample: (play_mode, loop_start, loop_end)."""
    return [(0, 0, 0), (1, 0, 0), (1, 0, max(L - 1, 0)), (1, L // 5, 3 * L // 5), (1, 2 * L // 5, L + 2),
            (1, L + 4, 0), (1, 3 * L // 5, L // 5), (1, 2 * L // 5, 2 * L // 5), (0, 3, 2)]


def assignments(n):
    """Round-robin over the bank and OLFX_NO_SAMPLE, the modes of loop_modes() cycling at another
    period; loops of 1, 2, 7, 8 and 9 frames forced onto the first and the last voices (on the
    1000-frame sample: frames a .. a + m - 1 play per turn with loop_start = a, loop_end = a + m - 1)."""
    recs = []
    for i in range(n):
        k = i % (len(LENGTHS) + 1)
        if k == len(LENGTHS):
            recs.append((i, None))
            continue
        mode, ls, le = loop_modes(LENGTHS[k])[(i // 2) % 9]
        recs.append((i, k, mode, ls, le))
    forced = [1, 2, 7, 8, 9]
    for j, m in enumerate(forced):
        for i in {j, n - 1 - j}:
            if 0 <= i < n:
                a = 100 + 61 * j
                recs[i] = (i, 11, 1, a, a + m - 1)
    return recs


class Trio:
    """The engine and the helper in both arithmetics, driven alike."""

    def __init__(self, n, cuda, seed=3, configure=True):
        self.n, self.cuda = n, cuda
        self.e = ofx.Engine("voice_sample", n)
        self.k = SR.SamplerVoices(n, kernel_arith=True)
        self.u = SR.SamplerVoices(n)
        self.refs = (self.k, self.u)
        if configure:
            self.config(workload.instance_params("voice_sample", 0, n, seed))

    def config(self, p):
        self.e.set_params(0, p)
        for r in self.refs:
            for i in range(self.n):
                r.config(i, p[:, i])

    def bank(self, samples):
        self.e.sample_bank(samples)
        for r in self.refs:
            r.sample_bank(samples)

    def voices(self, recs):
        self.e.sample_voices(recs)
        for r in self.refs:
            r.sample_voices(recs)

    def events(self, evs):
        self.e.voice_events(evs)
        for r in self.refs:
            r.events(evs)

    def reset(self):
        self.e.reset()
        for r in self.refs:
            r.reset()

    def run(self, frames):
        import torch
        out = torch.full((1, frames, self.n), 7.0, device=self.cuda)      # poisoned: every word is written
        self.e.process(None, out=out)
        return out.cpu().numpy(), self.k.process(frames), self.u.process(frames)


def check(got, want_k, want_u):
    assert np.isfinite(want_k).all() and np.isfinite(got).all()
    bad = np.argwhere(got.view(np.uint32) != want_k.view(np.uint32))
    assert len(bad) == 0, (len(bad), bad[:4], got[tuple(bad[0])], want_k[tuple(bad[0])])
    err = rel_err(got, want_u)
    print(f"rel err vs the unfused arithmetic: {err:.3e}")
    assert err <= VOICE_TOL


def cat(parts):
    return tuple(np.concatenate([p[j] for p in parts], 1) for j in range(3))


# ------------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("n", [1, 33, 65, 130])
def test_ragged_voices(cuda, rcp_table, bank, n):
    """A partly filled wave, one voice past a workgroup, two workgroups and more; three 256-frame
    blocks.  Voices i % 5 == 3 are never triggered."""
    t = Trio(n, cuda)
    t.bank(bank)
    recs = assignments(n)
    t.voices(recs)
    trig = [i for i in range(n) if i % 5 != 3]
    t.events([(i, NOTE_ON, 40 + i % 50) for i in trig])
    got, wk, wu = cat([t.run(256) for _ in range(3)])
    check(got, wk, wu)
    silent = [i for i in range(n) if i not in trig or recs[i][1] is None]
    assert not got[0][:, silent].any()
    sounding = [i for i in trig if recs[i][1] is not None]
    assert sounding and all(got[0][:, i].any() for i in sounding)
    assert t.e.kernel_name == "sampler_block_v1"


# ------------------------------------------------------------------------------------------ 5
def test_ragged_frames(cuda, rcp_table, bank):
    """Blocks of 4, 20, 36, 256 and 12 frames: samples end and loops turn inside a chunk, at a chunk
    edge (8), at a window edge (64) and at a block edge; the last window of a block is partial."""
    n = 65
    t = Trio(n, cuda, seed=4)
    t.bank(bank)
    t.voices(assignments(n))
    t.events([(i, NOTE_ON if i % 2 else GATE_ON, 60) for i in range(n)])
    got, wk, wu = cat([t.run(b) for b in [4, 20, 36, 256, 12]])
    check(got, wk, wu)
    assert got.any()


# ------------------------------------------------------------------------------------------ 6
def test_events(cuda, rcp_table, bank):
    """NoteOn; NoteOff mid-sample (zeros enter the filter while the amp envelope releases); NoteOn
    again (seeks to 0); GateOff then GateOn (no retrigger); NoteOn + NoteOff at one boundary (cursor
    0, paused, envelopes retriggered); a loop-point change (cursor kept) and a reassignment (fresh
    Sample) between blocks."""
    n = 40
    t = Trio(n, cuda, seed=6)
    t.bank(bank)
    t.voices([(i, 11 if i % 3 else 9, i % 2, 50, 600 if i % 3 else 200) for i in range(n)])
    every = range(n)
    parts = []
    t.events([(i, NOTE_ON, 50 + i) for i in every]);                    parts.append(t.run(256))
    t.events([(i, NOTE_OFF, 50 + i) for i in every if i % 2 == 0]);     parts.append(t.run(256))
    t.events([(i, NOTE_ON, 62) for i in every if i % 4 == 0]);          parts.append(t.run(256))
    t.events([(i, GATE_OFF) for i in every]);                           parts.append(t.run(64))
    t.events([(i, GATE_ON) for i in every]);                            parts.append(t.run(256))
    t.events([e for i in every for e in ((i, NOTE_ON, 70), (i, NOTE_OFF, 70))])
    parts.append(t.run(128))
    t.events([(i, GATE_ON) for i in every]);                            parts.append(t.run(128))
    # loop points change under a running cursor; every fifth voice gets another sample (fresh: silent
    # until its next gate), every seventh loses its sample
    t.voices([(i, 11 if i % 3 else 9, 1, 10, 90) for i in every if i % 5 and i % 7])
    t.voices([(i, 7) for i in every if i % 5 == 0])
    t.voices([(i, None) for i in every if i % 7 == 0])
    parts.append(t.run(256))
    t.events([(i, NOTE_ON, 55) for i in every]);                        parts.append(t.run(256))
    got, wk, wu = cat(parts)
    check(got, wk, wu)
    # the boundary with NoteOn + NoteOff: the source is paused, so only the filter's tail is heard
    src = SR.SamplerVoices(1)
    src.sample_bank(bank)
    src.sample_voices([(0, 11)])
    src.events([(0, NOTE_ON, 70), (0, NOTE_OFF, 70)])
    assert not src.source(0, 64).any()


def test_event_storm(cuda, rcp_table, bank):
    """40 blocks of 64 frames; before each, random gate calls and SetFrequency on random voices (several
    per voice at one boundary, more than four voices per workgroup: the overflow list) and now and then
    new Sample settings."""
    n = 70
    rng = np.random.default_rng(8)
    t = Trio(n, cuda, seed=8)
    t.bank(bank)
    t.voices(assignments(n))
    parts = []
    for b in range(40):
        if b % 6 == 5:
            recs = []
            for i in rng.choice(n, 9, replace=False):
                k = int(rng.integers(0, len(LENGTHS) + 1))
                if k == len(LENGTHS):
                    recs.append((int(i), None))
                else:
                    mode, ls, le = loop_modes(LENGTHS[k])[int(rng.integers(0, 9))]
                    recs.append((int(i), k, mode, ls, le))
            t.voices(recs)
        evs = []
        for _ in range(int(rng.integers(0, 30))):
            ty = int(rng.integers(0, 5))
            evs.append((int(rng.integers(0, n)), ty, int(rng.integers(30, 90)), float(rng.uniform(50, 2000))))
        t.events(evs)
        parts.append(t.run(64))
    got, wk, wu = cat(parts)
    check(got, wk, wu)
    assert got.any()


# ------------------------------------------------------------------------------------------ 7
def test_bank_lifecycle(cuda, rcp_table):
    """A 70,000-frame one-shot played through and past its end (the cursor crosses 65,536); a smaller
    bank uploaded over it (assignments drop as specified, every Sample fresh: the source is silent
    until retriggered); olfx_reset keeps the bank and the assignments and leaves every voice fresh."""
    n = 3
    long_bank = workload.sample_bank([70000, 100, 50], seed=12)
    t = Trio(n, cuda, seed=9)
    t.bank(long_bank)
    t.voices([(0, 0), (1, 2, 1, 5, 40), (2, 1)])
    t.events([(i, NOTE_ON, 60) for i in range(n)])
    blocks = [256] * 274 + [120]                      # 70,264 frames
    parts = [t.run(b) for b in blocks]
    got = cat(parts)[0]
    assert got[0][69000:70000, 0].any()
    # fewer samples: index 2 is gone (voice 1 becomes unassigned), 0 and 1 stay valid over new data
    small = workload.sample_bank([300, 100], seed=13)
    t.bank(small)
    parts.append(t.run(256))                          # nothing plays: only the filters' tails
    probe = SR.SamplerVoices(n)
    probe.sample_bank(long_bank)
    probe.sample_voices([(0, 0), (1, 2, 1, 5, 40), (2, 1)])
    probe.events([(i, NOTE_ON, 60) for i in range(n)])
    probe.sample_bank(small)
    assert not any(probe.source(i, 64).any() for i in range(n))
    t.events([(i, NOTE_ON, 60) for i in range(n)])
    parts += [t.run(256), t.run(256)]
    got = cat(parts[-2:])[0]
    assert got[0][:, 0].any() and got[0][:, 2].any()
    # the whole run against the helper (the tolerance is relative to each voice's rms over the run, as in
    # the voice tests: a filter tail dying away after the bank change is compared on that scale)
    check(*cat(parts))
    # a record that names the dropped index is refused and changes nothing
    with pytest.raises(ofx.OlfxError):
        t.e.sample_voices([(0, 1), (1, 2)])
    # reset: default parameters, zeroed state, fresh Samples -- exactly 0 until triggered; the bank and
    # the assignments are kept
    t.reset()
    got, wk, wu = t.run(64)
    assert not got.any() and not wk.any()
    t.events([(i, GATE_ON) for i in range(n)])
    parts = [t.run(256), t.run(256)]
    got = cat(parts)[0]
    assert got[0][:, 0].any() and got[0][:, 2].any() and not got[0][:, 1].any()
    # no bank at all: the source is silent whatever the gate
    t.bank([])
    t.events([(i, NOTE_ON, 60) for i in range(n)])
    parts.append(t.run(64))
    check(*cat(parts))


# ------------------------------------------------------------------------------------------ 8
def test_buses(cuda, rcp_table, bank):
    """olfx_mix over a 16-voice kit in two buses: bit-exact against O.mix_ref over the helper's voices."""
    import torch
    n = 16
    t = Trio(n, cuda, seed=10)
    t.bank(bank)
    t.voices([(i, (5 + i) % len(LENGTHS), i % 2, 3, 40) for i in range(n)])
    buses = [[0, 3, 5, 7, 9, 11, 13, 15, 1], [2, 4, 6, 8, 10, 12, 14]]
    t.e.mix_config(buses)
    t.events([(i, NOTE_ON, 48 + i) for i in range(n)])
    frames = 256
    out = torch.empty((1, frames, n), device=cuda)
    t.e.process(None, out=out)
    mixed = t.e.mix(out).cpu().numpy()
    wk = t.k.process(frames)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), wk.view(np.uint32))
    want = O.mix_ref(wk, buses)
    assert np.array_equal(mixed.view(np.uint32), want.view(np.uint32))
    assert mixed.any()
