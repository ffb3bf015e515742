"""OLFX_KIND_SYNTH (synth_block_v1: P MoogFilter voices -> Polyvoice sum -> DelayFx<1> -> stub reverb
-> FilterFx<2> in one launch) on the GPU, bit-exact against tests/synth_ref.py -- the existing oracles
composed: O.Voice in the kernels' arithmetic, O.mix_ref, O.FxRack at topology 1 -- and against the
three launches it replaces.  Small ragged shapes: a partly filled group and an empty second delay wave
(n = 1, 33), two and three groups (65, 130), one voice, the odd count past four and the maximum (the
wave that runs two voices), chunks of 4 .. 16 frames, every line delay at which the delay stage's
window takes another position.  The grid is one workgroup per 64 instruments (not persistent), so
there is no back-to-back-groups case.

Every test asserts of its reference that it is finite for every instrument and that both channels are
non-zero for every instrument (synth_ref.condition; tests/test_synth_ref.py checks the same scripts on
the CPU)."""
import numpy as np
import pytest

import ol_dsp_amd as ofx
import synth_ref as SR
from helpers import first_mismatch
from ol_dsp_amd import _lib, workload

pytestmark = pytest.mark.gpu


def process(e, frames, cuda):
    import torch
    out = torch.empty((2, frames, e.n), device=cuda)
    e.process(None, out=out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def run_engine(script, n, voices, cuda, trace=None, e=None):
    """The script on a synth engine: ([2][frames][n], the engine).  At a ("check_playing",) step
    Engine.playing of every instrument must equal the rule's table (trace, from synth_ref.run_ref)."""
    if e is None:
        e = ofx.Engine("synth", n, voices=voices)
    assert e.kernel_name == "synth_block_v1" and e.voices == voices
    out, checks = [], 0
    for step in script:
        if step[0] == "params":
            e.set_params(0, step[1])
        elif step[0] == "set":
            e.set_param(step[1], step[2], step[3])
        elif step[0] == "events":
            e.note_events([(i, t, note) for i, t, note in step[1]])
        elif step[0] == "block":
            out.append(process(e, step[1], cuda))
        elif step[0] == "check_playing" and trace is not None:
            got = np.array([e.playing(i) for i in range(n)])
            assert np.array_equal(got, trace[checks]), (checks, np.argwhere(got != trace[checks])[:4])
            checks += 1
    assert trace is None or checks == len(trace)
    return np.concatenate(out, 1), e


def compare(name, cuda):
    script, n, voices = SR.GPU_SCRIPTS[name]()
    yr, ref = SR.run_ref(script, n, voices, threads=8)
    SR.condition(yr)
    y, e = run_engine(script, n, voices, cuda, trace=ref.trace)
    assert SR.bits_equal(y, yr), first_mismatch(y, yr)
    return y, e, ref


@pytest.mark.parametrize("n", [1, 33, 65, 130])
def test_ragged_instances(cuda, rcp_table, n):
    compare(f"ragged_instances_{n}", cuda)


@pytest.mark.parametrize("voices", [1, 2, 5, 8])
def test_voices_per_instrument(cuda, rcp_table, voices):
    compare(f"voices_{voices}", cuda)


def test_ragged_frames(cuda, rcp_table):
    """Blocks of 4, 20, 36, 256 and 12 frames with note events between them."""
    compare("ragged_frames", cuda)


def test_delay_lines(cuda, rcp_table):
    """The line delays 0, 1, 15, 16, 17, 24000 and 47999 on the first and last instruments."""
    script, n, _ = SR.GPU_SCRIPTS["delay_lines"]()
    d = (script[0][1][SR.RACK_TIME] * np.float32(48000.0)).astype(np.int64)
    assert set(SR.LINE_DELAYS) <= set(d[:7].tolist()) and set(SR.LINE_DELAYS) <= set(d[-7:].tolist())
    compare("delay_lines", cuda)


def test_allocation_storm(cuda, rcp_table):
    """Random NOTE_ON / NOTE_OFF / GATE_* per instrument and block, a fifth note into full instruments,
    note 0: Engine.playing equals the rule's table after every block's events, the output is bit-exact
    over about 6,000 frames."""
    y, e, ref = compare("storm", cuda)
    assert y.shape[1] >= 6000 and len(ref.trace) > 20
    e.voice_events([(0, _lib.EV_SET_FREQUENCY, 0, 440.0)])      # accepted, does nothing
    assert e.playing(0) == ref.playing[0].tolist()


def test_firmware_setup(cuda, rcp_table):
    """The firmware's own set-up (main.cpp:114-128 before Init at :149-154): its control list as member
    writes without Update (olfx_set_member with the values olfx_synth_control_map gives), a NoteOn, a
    block against oracle voices configured by init_members; then olfx_update (the first Update() ends
    Init's component defaults) and a block against the same members through config; then one of the
    list's controls through olfx_control (handleMidi's route once the firmware runs)."""
    n, B = 3, 512
    controls = [(5, 48), (41, 0), (42, 0), (74, 0), (75, 100), (76, 0), (77, 24), (73, 127),
                (108, 0), (109, 127), (110, 127), (111, 100), (114, 100), (7, 80)]
    e = ofx.Engine("synth", n)
    ref = SR.Synth(n)
    members = SR.defaults()[:SR.NV].copy()
    names = ofx.PARAMS[ofx.KIND_SYNTH]
    for cc, value in controls:
        # voice.UpdateMidiControl only: the list never reaches delay_fx, reverb_fx or filter_fx
        hits = [(f, v) for f, v in ofx.synth_control_map(cc, value) if not f.startswith("rack_")]
        assert len(hits) == 1                                    # every control of the list is a voice control
        f, v = hits[0]
        if f == "update_only":                                   # osc_1_mix: no modelled member
            continue
        for i in range(n):
            assert e.lib.olfx_set_member(e.handle, i, names.index(f), float(v)) == 0
        members[names.index(f)] = v
    for i in range(n):
        ref.init_members(i, members)
        assert e.get_param(i, "portamento") == np.float32(ofx.control_map("voice_moog", 5, 48)[1])
    notes = [(i, SR.EV_NOTE_ON, 50 + 7 * i) for i in range(n)]
    e.note_events(notes)
    for ev in notes:
        ref.event(*ev)
    y0, yr0 = process(e, B, cuda), ref.process(B)
    e.update()
    for i in range(n):
        ref.update(i)
    y1, yr1 = process(e, B, cuda), ref.process(B)
    e.control([(1, 75, 60.0)])                                   # CC_ENV_FILT_D on a running instrument
    f, v = ofx.synth_control_map(75, 60.0)[0]
    ref.set(1, f, v)
    y2, yr2 = process(e, B, cuda), ref.process(B)
    y, yr = np.concatenate([y0, y1, y2], 1), np.concatenate([yr0, yr1, yr2], 1)
    SR.condition(yr)
    assert SR.bits_equal(y, yr), first_mismatch(y, yr)


def test_control_moves_both_filters(cuda, rcp_table):
    """A CC-41 event moves the voice filter and FILTER_CUTOFF; a hardware-source one too."""
    n, B = 5, 256
    p = SR.params(n, 5)
    script = [("params", p), ("events", SR.notes_on(n, 4))]
    e = ofx.Engine("synth", n)
    ref = SR.Synth(n)
    ref.set_params(p)
    e.set_params(0, p)
    e.note_events(SR.notes_on(n, 4))
    for ev in script[1][1]:
        ref.event(*ev)
    ys, yrs = [process(e, B, cuda)], [ref.process(B)]
    for inst, value, source in ((1, 90.0, "midi"), (3, 0.4, "hw")):
        e.control([(inst, 41, value, source)])
        hits = ofx.synth_control_map(41, value, source)
        assert [f for f, _ in hits] == ["filter_cutoff", "rack_filter_cutoff"]
        for f, v in hits:
            ref.set(inst, f, v)
            assert e.get_param(inst, f) == np.float32(v)
    ys.append(process(e, B, cuda))
    yrs.append(ref.process(B))
    y, yr = np.concatenate(ys, 1), np.concatenate(yrs, 1)
    SR.condition(yr)
    assert SR.bits_equal(y, yr), first_mismatch(y, yr)
    with pytest.raises(ofx.OlfxError):
        e.set_param(0, "rack_topology", 0.0)
    assert e.get_param(0, "rack_topology") == 1.0


def test_param_change_and_reset(cuda, rcp_table):
    """A parameter change lands at the next block; after olfx_reset a second run reproduces the first
    (Playing() cleared, the rack ring and its clock at zero, defaults again)."""
    script, n, voices = SR.GPU_SCRIPTS["param_change"]()
    y, e, ref = compare("param_change", cuda)
    yr_same, _ = SR.run_ref([s for s in script if s[0] != "set"], n, voices)
    assert SR.bits_equal(y[:, :256], yr_same[:, :256]) and not SR.bits_equal(y[:, 256:], yr_same[:, 256:])
    e.reset()
    assert e.frames_processed == 0 and e.playing(0) == [0, 0, 0, 0]
    assert e.get_param(0, "rack_topology") == 1.0
    y2, _ = run_engine(script, n, voices, cuda, e=e)
    assert SR.bits_equal(y2, y), first_mismatch(y2, y)
    host = ofx.Engine("synth", n)                                # host-pointer I/O equals device-pointer I/O
    host.set_params(0, script[0][1])
    host.note_events([(i, t, note) for i, t, note in script[1][1]])
    yh = host.process(None, out=np.empty((2, 256, n), np.float32))
    assert SR.bits_equal(yh, y[:, :256]), first_mismatch(yh, y[:, :256])


def test_composed_engines(cuda):
    """130 instruments of 4 voices against the three launches the kind replaces -- a voice_moog engine
    of 520 voices (voice p * 130 + i), olfx_mix into 130 buses, an fxrack engine at topology 1 -- driven
    with the same parameters and the same routed events: bit-identical, no oracle involved."""
    import torch
    n, P, B = 130, 4, 256
    p = SR.params(n, 6)
    synth = ofx.Engine("synth", n)
    voice = ofx.Engine("voice_moog", P * n)
    rack = ofx.Engine("fxrack", n)
    poly = ofx.Polyvoice(voice, [[q * n + i for q in range(P)] for i in range(n)])
    synth.set_params(0, p)
    voice.set_params(0, np.tile(p[:SR.NV], (1, P)))
    rack.set_params(0, p[SR.NV:])
    rng = np.random.default_rng(6)
    ys, yc = [], []
    for b, frames in enumerate([B, 20, B, B]):
        evs = SR.notes_on(n, P) if b == 0 else [
            (int(i), int(rng.choice([0, 1])), int(rng.integers(36, 97))) for i in np.flatnonzero(rng.random(n) < 0.5)]
        if b == 2:
            evs += [(i, 0, int(workload.voice_notes(0, n * P)[P * i])) for i in range(n)]
        synth.note_events(evs)
        for i, t, note in evs:
            (poly.note_on if t == 1 else poly.note_off)(i, note)
        ys.append(process(synth, frames, cuda))
        vo = torch.empty((1, frames, P * n), device=cuda)
        x = torch.zeros((2, frames, n), device=cuda)
        bus = poly.process(vo, x[0])                             # the sum into the rack's input channel 0
        assert bus.data_ptr() == x.data_ptr()
        yc.append(rack.process(x).cpu().numpy())
        got = np.array([synth.playing(i) for i in range(n)])
        assert np.array_equal(got, poly.playing.reshape(P, n).T)
    y, yc = np.concatenate(ys, 1), np.concatenate(yc, 1)
    assert np.isfinite(yc).all() and np.all(np.any(yc != 0, axis=1))
    assert np.array_equal(y.view(np.uint32), yc.view(np.uint32)), first_mismatch(y, yc)
