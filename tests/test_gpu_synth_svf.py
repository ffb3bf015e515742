"""OLFX_KIND_SYNTH_SVF (synth_svf_block_v1: P SvfFilter voices -> Polyvoice sum -> the rack at each
instrument's topology, 0 or 1, in one launch) on the GPU, bit-exact against tests/synth_svf_ref.py -- the
existing oracles composed: O.Voice(moog=False) in voice_block_v5's arithmetic, O.mix_ref, O.FxRack on
(mono, 0) -- and against the three launches it replaces.  Small ragged shapes as tests/test_gpu_synth.py:
a partly filled group and an empty second delay wave (n = 1, 33), two and three groups (65, 130), one
voice, the odd count past four and the maximum (the wave that runs two voices), chunks of 4 .. 16 frames,
every line delay at which the delay stage's window takes another position; every script draws each
instrument's topology from {0, 1}, and one puts both in every lane pair of the delay waves and switches
some between blocks.

Every test asserts of its reference what synth_svf_ref.condition states (finite; channel 0 non-zero for
every instrument; channel 1 non-zero at topology 1, all +-0 at topology 0) before it compares;
tests/test_synth_svf_ref.py checks the same scripts on the CPU."""
import numpy as np
import pytest

import ol_dsp_amd as ofx
import synth_ref as SR
import synth_svf_ref as SV
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
    """The script on an Svf-synth engine: ([2][frames][n], the engine).  At a ("check_playing",) step
    Engine.playing of every instrument must equal the rule's table (trace, from synth_svf_ref.run_ref)."""
    if e is None:
        e = ofx.Engine("synth_svf", n, voices=voices)
    assert e.kernel_name == "synth_svf_block_v1" and e.voices == voices
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
    script, n, voices = SV.GPU_SCRIPTS[name]()
    yr, ref = SV.run_ref(script, n, voices, threads=8)
    SV.condition(yr, ref.topology_of_frames())
    y, e = run_engine(script, n, voices, cuda, trace=ref.trace)
    assert SV.bits_equal(y, yr), first_mismatch(y, yr)
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
    script, n, _ = SV.GPU_SCRIPTS["delay_lines"]()
    d = (script[0][1][SR.RACK_TIME] * np.float32(48000.0)).astype(np.int64)
    assert set(SR.LINE_DELAYS) <= set(d[:7].tolist()) and set(SR.LINE_DELAYS) <= set(d[-7:].tolist())
    compare("delay_lines", cuda)


def test_topology_mix(cuda, rcp_table):
    """70 instruments, even ones at topology 0 and odd ones at 1 (both in every lane pair of the delay
    waves), master volumes 0.25 .. 1.6 and none of them 1; between the blocks eight instruments switch
    0 -> 1 and 1 -> 0 and two of them back.  A switch lands at the next block boundary."""
    y, e, ref = compare("topology_mix", cuda)
    topo = ref.topology_of_frames()
    assert np.any(topo[0] != topo[300]) and np.any(topo[300] != topo[400])
    assert [e.get_param(i, "rack_topology") for i in (0, 1, 32, 69)] == [0.0, 0.0, 1.0, 1.0]
    # the master is live at topology 0: an instrument there is not its topology-1 self
    script, n, voices = SV.GPU_SCRIPTS["topology_mix"]()
    p1 = script[0][1].copy()
    p1[SV.TOPOLOGY] = 1.0
    y1, _ = run_engine([("params", p1)] + script[1:3], n, voices, cuda)
    assert SV.bits_equal(y1[:, :256, 1::2], y[:, :256, 1::2])
    assert np.all(np.any(y1[0, :256, 0::2].view(np.uint32) != y[0, :256, 0::2].view(np.uint32), axis=0))


def test_allocation_storm(cuda, rcp_table):
    """Random NOTE_ON / NOTE_OFF / GATE_* per instrument and block, a fifth note into full instruments,
    note 0: Engine.playing equals the rule's table after every block's events, the output is bit-exact
    over about 2,000 frames."""
    y, e, ref = compare("storm", cuda)
    assert 2000 <= y.shape[1] < 2300 and len(ref.trace) > 8
    e.voice_events([(0, _lib.EV_SET_FREQUENCY, 0, 440.0)])      # accepted, does nothing
    assert e.playing(0) == ref.playing[0].tolist()


def test_param_change_and_reset(cuda, rcp_table):
    """A parameter change lands at the next block; after olfx_reset a second run reproduces the first
    (Playing() cleared, the rack ring and its clock at zero, defaults again: topology 1); host-pointer
    I/O equals device-pointer I/O."""
    script, n, voices = SV.GPU_SCRIPTS["param_change"]()
    y, e, ref = compare("param_change", cuda)
    yr_same, _ = SV.run_ref([s for s in script if s[0] != "set"], n, voices)
    assert SV.bits_equal(y[:, :256], yr_same[:, :256]) and not SV.bits_equal(y[:, 256:], yr_same[:, 256:])
    e.reset()
    assert e.frames_processed == 0 and e.playing(0) == [0, 0, 0, 0]
    assert all(e.get_param(i, "rack_topology") == 1.0 for i in range(n))
    y2, _ = run_engine(script, n, voices, cuda, e=e)
    assert SV.bits_equal(y2, y), first_mismatch(y2, y)
    host = ofx.Engine("synth_svf", n)
    host.set_params(0, script[0][1])
    host.note_events([(i, t, note) for i, t, note in script[1][1]])
    yh = host.process(None, out=np.empty((2, 256, n), np.float32))
    assert SV.bits_equal(yh, y[:, :256]), first_mismatch(yh, y[:, :256])


def test_refused_topologies_change_nothing(cuda):
    e = ofx.Engine("synth_svf", 3)
    e.set_param(1, "rack_topology", 0.0)
    for bad in (2.0, -1.0, 0.5):
        with pytest.raises(ofx.OlfxError):
            e.set_param(1, "rack_topology", bad)
    assert [e.get_param(i, "rack_topology") for i in range(3)] == [1.0, 0.0, 1.0]
    m = ofx.Engine("synth", 3)
    with pytest.raises(ofx.OlfxError):
        m.set_param(1, "rack_topology", 0.0)
    assert m.get_param(1, "rack_topology") == 1.0 and m.kernel_name == "synth_block_v1"


def test_controls_follow_the_topology(cuda, rcp_table):
    """Instruments 0, 2, 4 at topology 0 and 1, 3 at topology 1.  At topology 1 one CC-41 event moves both
    filters (MIDI and hardware source); at topology 0 the same event moves the voice filter only, and the
    rack part follows the fxrack's topology-0 mapping: CC 45 drives FILTER_CUTOFF, CC 7 the voices' amount
    and the master volume.  Checked through get_param and, bit-exact, through the output."""
    n, B = 5, 256
    p = SV.params(n, 5)
    p[SV.TOPOLOGY] = [0, 1, 0, 1, 0]
    e = ofx.Engine("synth_svf", n)
    ref = SV.Synth(n)
    ref.set_params(p)
    e.set_params(0, p)
    e.note_events(SV.notes_on(n, 4))
    for ev in SV.notes_on(n, 4):
        ref.event(*ev)
    ys, yrs = [process(e, B, cuda)], [ref.process(B)]
    events = [(1, 41, 90.0, "midi", ["filter_cutoff", "rack_filter_cutoff"]),
              (3, 41, 0.4, "hw", ["filter_cutoff", "rack_filter_cutoff"]),
              (0, 41, 90.0, "midi", ["filter_cutoff"]),
              (2, 45, 70.0, "midi", ["rack_filter_cutoff"]),
              (3, 45, 70.0, "midi", []),
              (4, 7, 100.0, "midi", ["amp_env_amount", "rack_master_volume"]),
              (1, 7, 100.0, "midi", ["amp_env_amount"])]
    for inst, cc, value, source, fields in events:
        topo = int(p[SV.TOPOLOGY, inst])
        before = {f: e.get_param(inst, f) for f in ofx.PARAMS[ofx.KIND_SYNTH_SVF]}
        e.control([(inst, cc, value, source)])
        hits = ofx.synth_control_map(cc, value, source, kind="synth_svf", topology=topo)
        assert [f for f, _ in hits] == fields, (inst, cc)
        rack_cc = cc + 4 if topo == 1 and 41 <= cc <= 44 else cc
        for f, v in hits:
            ref.set(inst, f, v)
            assert e.get_param(inst, f) == np.float32(v)
            if f.startswith("rack_"):                           # the fxrack's own mapping at this topology
                assert (f[5:], v) == ofx.control_map("fxrack", rack_cc, value, source)
            else:
                assert (f, v) == ofx.control_map("voice", cc, value, source)
        for f, was in before.items():
            assert f in fields or e.get_param(inst, f) == was, (inst, cc, f)
    ys.append(process(e, B, cuda))
    yrs.append(ref.process(B))
    y, yr = np.concatenate(ys, 1), np.concatenate(yrs, 1)
    SV.condition(yr, ref.topology_of_frames())
    assert SV.bits_equal(y, yr), first_mismatch(y, yr)
    assert np.any(y[:, B:, 4].view(np.uint32) != run_unchanged(p, cuda, B)[:, B:, 4].view(np.uint32))


def run_unchanged(p, cuda, B):
    """The controls test's two blocks with no control event between them."""
    n = p.shape[1]
    e = ofx.Engine("synth_svf", n)
    e.set_params(0, p)
    e.note_events(SV.notes_on(n, 4))
    return np.concatenate([process(e, B, cuda), process(e, B, cuda)], 1)


def test_composed_engines(cuda):
    """130 instruments of 4 voices against the three launches the kind replaces -- a voice engine of 520
    voices (voice p * 130 + i), olfx_mix into 130 buses, an fxrack engine with the instruments' topologies
    -- driven with the same parameters and the same routed events over blocks of 256, 20, 256 and 256
    frames: bit-identical, no oracle involved."""
    import torch
    n, P, B = 130, 4, 256
    p = SV.params(n, 6)
    assert set(np.unique(p[SV.TOPOLOGY])) == {0.0, 1.0}
    synth = ofx.Engine("synth_svf", n)
    voice = ofx.Engine("voice", P * n)
    rack = ofx.Engine("fxrack", n)
    assert (voice.kernel_name, rack.kernel_name) == ("voice_block_v5", "fxrack_block_v3")
    poly = ofx.Polyvoice(voice, [[q * n + i for q in range(P)] for i in range(n)])
    synth.set_params(0, p)
    voice.set_params(0, np.tile(p[:SV.NV], (1, P)))
    rack.set_params(0, p[SV.NV:])
    rng = np.random.default_rng(6)
    ys, yc = [], []
    for b, frames in enumerate([B, 20, B, B]):
        evs = SV.notes_on(n, P) if b == 0 else [
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
    topo = np.tile(p[SV.TOPOLOGY][None, :], (y.shape[1], 1))
    SV.condition(yc, topo)
    assert np.array_equal(y.view(np.uint32), yc.view(np.uint32)), first_mismatch(y, yc)
