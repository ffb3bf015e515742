"""tests/sampler_ref (the CPU reference of the sample-playback voice) pinned on both sides: its bare
Sample stream to the runs recorded from the reference's own Sample.cpp
(tests/golden/sample_reference_runs.json), and its voice -- Adsr, setters, Svf, in both arithmetics --
to the frozen oracle/voice_ref.c, bit for bit, through a case where the two sound sources coincide: a
constant 0.5 sample against the oscillator at 0 Hz (phase and increment 0, polyBLEP 0: the saw is
exactly the DC 0.5)."""
import json
import os

import numpy as np
import pytest

import oracle as O
import sampler_ref as SR
from ol_dsp_amd import workload

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def runs():
    with open(os.path.join(ROOT, "tests", "golden", "sample_reference_runs.json")) as f:
        return json.load(f)


def one_voice(sample, mode=SR.ONESHOT, ls=0, le=0):
    v = SR.SamplerVoices(1)
    v.sample_bank([np.asarray(sample, np.float32)])
    v.sample_voices([(0, 0, mode, ls, le)])
    return v


def test_source_reproduces_the_reference_runs(runs):
    assert len(runs["runs"]) == 8 and runs["sample"] == [1, 2, 3, 4, 5] and runs["ticks"] == 14
    for r in runs["runs"]:
        v = one_voice(runs["sample"], r["mode"], r["loop_start"], r["loop_end"])
        v.seek(0, 0)
        v.play(0)
        got = v.source(0, runs["ticks"])
        assert got.tolist() == [float(x) for x in r["stream"]], (r, got.tolist())


def test_source_pause_gate_and_loop_points():
    # a fresh Sample does not play
    v = one_voice([1, 2, 3, 4, 5])
    assert v.source(0, 3).tolist() == [0, 0, 0]
    # Pause mid-sample gives zeros and keeps the cursor; Play goes on from it
    v.event(0, 2)                                   # GateOn: Seek(0), Play()
    assert v.source(0, 2).tolist() == [1, 2]
    v.pause(0)
    assert v.source(0, 3).tolist() == [0, 0, 0]
    v.play(0)
    assert v.source(0, 2).tolist() == [3, 4]
    # GateOn restarts at frame 0; GateOff pauses; NoteOn restarts too
    v.event(0, 2)
    assert v.source(0, 3).tolist() == [1, 2, 3]
    v.event(0, 3)
    assert v.source(0, 2).tolist() == [0, 0]
    v.event(0, 1, 60)
    assert v.source(0, 7).tolist() == [1, 2, 3, 4, 5, 0, 0]
    # a loop-point change without a seek keeps the cursor: playing 1 2 3, then Loop 1..3 goes on at 4
    v = one_voice([1, 2, 3, 4, 5])
    v.event(0, 2)
    assert v.source(0, 3).tolist() == [1, 2, 3]
    v.sample_voices([(0, 0, SR.LOOP, 1, 3)])
    assert v.source(0, 6).tolist() == [4, 2, 3, 4, 2, 3]
    # another index is a fresh Sample: not playing, cursor 0
    v.sample_bank([np.float32([1, 2, 3]), np.float32([7, 8, 9])])
    v.sample_voices([(0, 0)])
    v.event(0, 2)
    assert v.source(0, 2).tolist() == [1, 2]
    v.sample_voices([(0, 1)])
    assert v.source(0, 2).tolist() == [0, 0]
    v.play(0)
    assert v.source(0, 4).tolist() == [7, 8, 9, 0]
    # no sample: nothing, whatever the gate
    v.sample_voices([(0, None)])
    v.event(0, 2)
    assert v.source(0, 3).tolist() == [0, 0, 0]


@pytest.mark.parametrize("kernel_arith", [False, True])
@pytest.mark.parametrize("trigger", ["gate_on", "note_on_freq0"])
def test_voice_equals_the_frozen_oracle_at_dc(kernel_arith, trigger):
    """8 voices, workload parameters (resonance, drive, envelope times), a 4,096-frame sample of 0.5,
    OneShot; 2,000 frames with a second NoteOn (+ SetFrequency 0) at frame 1,000; no gate-off (after
    one the oscillator keeps sounding and a paused sample does not).  Every frame, bit for bit."""
    n, frames = 8, 2000
    p = workload.instance_params("voice", 0, n, seed=5)
    osc = O.Voice(n, kernel_arith=kernel_arith)
    smp = SR.SamplerVoices(n, kernel_arith=kernel_arith)
    smp.sample_bank([np.full(4096, 0.5, np.float32)])
    smp.sample_voices([(i, 0) for i in range(n)])
    for i in range(n):
        osc.config(i, p[:, i])
        smp.config(i, p[:, i])

    def start(first):
        for i in range(n):
            for b in (osc, smp):
                if trigger == "gate_on" and first:
                    b.event(i, 2)
                else:
                    b.event(i, 1, 40 + i)
                    b.event(i, 4, 0, 0.0)           # SetFrequency(0) at the same boundary
    start(True)
    want = [osc.process(1000)]
    got = [smp.process(1000)]
    start(False)
    want.append(osc.process(frames - 1000))
    got.append(smp.process(frames - 1000))
    want, got = np.concatenate(want, 1), np.concatenate(got, 1)
    assert np.isfinite(want).all() and np.abs(want).max() > 1e-3
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), \
        np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:4]
