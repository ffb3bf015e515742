"""OLFX_KIND_DRUMKIT (drumkit_block_v1: P sample voices with their own configs and Samples -> VoiceMap sum by
ascending note -> the rack at each kit's topology, one launch) on the GPU, bit-exact against tests/drumkit_ref.py
-- the existing references composed: sampler_ref.SamplerVoices in sampler_block_v1's arithmetic, O.mix_ref,
O.FxRack on (sum, 0) -- and against the three launches it replaces.  Small ragged shapes: a partly filled group
and an empty second delay wave (n = 1, 33), two and three groups (65, 130); one voice, the first wave with two
voices, the maximum (P = 1, 2, 5, 8); blocks of 4 .. 256 frames; samples shorter than, equal to and longer than
the 16-frame chunk, every loop configuration of the sampler's tests and loops of 1 .. 17 frames; map changes
between blocks; both topologies in every lane pair of the delay waves.

Every test asserts of its reference what drumkit_ref.condition states before it compares;
tests/test_drumkit_ref.py checks the same scripts on the CPU."""
import numpy as np
import pytest

import drumkit_ref as DK
import ol_dsp_amd as ofx
from helpers import first_mismatch
from ol_dsp_amd import _lib, workload

pytestmark = pytest.mark.gpu


def process(e, frames, cuda):
    import torch
    out = torch.full((2, frames, e.n), 7.0, device=cuda)        # poisoned: every word is written
    e.process(None, out=out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def apply(e, step, voices):
    """One non-block step of a drumkit_ref script on the engine."""
    op = step[0]
    if op == "params":
        e.set_params(0, step[1])
    elif op == "set":
        e.set_param(step[1], step[2], step[3])
    elif op == "bank":
        e.sample_bank(step[1])
    elif op == "samples":
        e.sample_voices([(kit * voices + slot, *rest) for kit, slot, *rest in step[1]])
    elif op == "map":
        e.drumkit_map(step[1])
    elif op == "events":
        e.note_events(step[1])
    elif op == "control":
        e.control(step[1])
    elif op == "reset":
        e.reset()
    else:
        raise ValueError(op)


def run_engine(script, n, voices, cuda, trace=None, e=None):
    """The script on a drum-kit engine: ([2][frames][n], the engine).  At a ("check_playing",) step
    Engine.playing of every kit must equal the reference's table."""
    if e is None:
        e = ofx.Engine("drumkit", n, voices=voices)
    assert e.kernel_name == "drumkit_block_v1" and e.voices == voices
    out, checks = [], 0
    for step in script:
        if step[0] == "block":
            out.append(process(e, step[1], cuda))
        elif step[0] == "check_playing":
            if trace is not None:
                got = np.array([e.playing(i) for i in range(n)])
                assert np.array_equal(got, trace[checks]), (checks, np.argwhere(got != trace[checks])[:4])
                checks += 1
        else:
            apply(e, step, voices)
    assert trace is None or checks == len(trace)
    return np.concatenate(out, 1), e


def compare(name, cuda):
    script, n, voices = DK.GPU_SCRIPTS[name]()
    yr, ref = DK.run_ref(script, n, voices, threads=8)
    DK.condition(yr, ref)
    y, e = run_engine(script, n, voices, cuda, trace=ref.trace)
    assert DK.bits_equal(y, yr), first_mismatch(y, yr)
    return y, e, ref, script


@pytest.mark.parametrize("n", [1, 33, 65, 130])
def test_ragged_instances(cuda, rcp_table, n):
    compare(f"ragged_instances_{n}", cuda)


@pytest.mark.parametrize("voices", [1, 2, 5, 8])
def test_voices_per_kit(cuda, rcp_table, voices):
    y, e, _, _ = compare(f"voices_{voices}", cuda)
    assert e.algorithmic_bytes_per_frame == 24 + 4 * voices and e.algorithmic_read_bytes_per_frame == 8 + 4 * voices


def test_ragged_frames(cuda, rcp_table):
    """Blocks of 4, 20, 36, 256 and 12 frames with retriggers, releases and a note nobody sits at between them."""
    compare("ragged_frames", cuda)


def test_sum_order(cuda, rcp_table):
    """70 kits of 5 voices, 67 of them with a note order that is not their slot order (and, by condition(),
    audibly so): a kernel that summed in slot order fails here."""
    _, _, ref, _ = compare("sum_order", cuda)
    assert sum(o != sorted(o) for o in ref.log[0][2]) == 67


def test_map_changes_between_blocks(cuda, rcp_table):
    """Swap, unmap, displace, a channel repointed with a control following it, a kit mapped late and a kit
    whose map stays empty (it sums nothing: +0.0f into the rack)."""
    y, e, ref, _ = compare("map_changes", cuda)
    assert not ref.order(6) and not y[:, :, 6].any()
    assert not y[:, :356, 5].any() and y[0, 612:, 5].any()
    with pytest.raises(ofx.OlfxError):                           # voice 1 of kit 0 at a second note: nothing changes
        e.drumkit_map([(0, None, 0, 1)])
    y2 = process(e, 64, cuda)
    assert DK.bits_equal(y2, ref.process(64))


def test_topology_mix(cuda, rcp_table):
    _, e, ref, _ = compare("topology_mix", cuda)
    assert [e.get_param(i, "rack_topology") for i in (0, 1, 32, 69)] == [0.0, 0.0, 1.0, 1.0]
    with pytest.raises(ofx.OlfxError):
        e.set_param(1, "rack_topology", 2.0)
    assert e.get_param(1, "rack_topology") == 0.0


def test_params_and_controls(cuda, rcp_table):
    """Per-voice parameters and controls by channel; the fields a control moved are the addressed slot's."""
    script, n, P = DK.GPU_SCRIPTS["params_and_controls"]()
    y, e, ref, _ = compare("params_and_controls", cuda)
    for i in (0, 1, n - 1):
        for f in range(DK.NPARAMS):
            if f >= DK.RACK0 or f // DK.NV < P:
                assert e.get_param(i, f) == ref.p[f, i], (i, f)
    assert e.get_param(0, "v1_filter_cutoff") == np.float32(ofx.control_map("voice_sample", 41, 80.0)[1])
    # without the control step the last block differs
    y0, _ = run_engine([s for s in script if s[0] != "control"], n, P, cuda)
    assert DK.bits_equal(y0[:, :512], y[:, :512]) and not DK.bits_equal(y0[:, 512:], y[:, 512:])


def test_note_storm(cuda, rcp_table):
    """About 2,000 frames of random NOTE_ON / NOTE_OFF at mapped and unmapped notes; Engine.playing equals the
    reference's table after every block's events; gate and frequency events are refused."""
    y, e, ref, _ = compare("storm", cuda)
    assert 2000 <= y.shape[1] < 2300 and len(ref.trace) > 8
    for bad in ((0, _lib.EV_GATE_ON, 60), (0, _lib.EV_GATE_OFF, 60), (0, _lib.EV_SET_FREQUENCY, 0, 440.0)):
        with pytest.raises(ofx.OlfxError):
            e.voice_events([bad])
    assert e.playing(0) == ref.playing[0].tolist()


def test_reset_and_bank_replacement(cuda, rcp_table):
    """After olfx_reset (the map, the bank and the assignments stay) a second run reproduces the first; a smaller
    bank drops the assignments it lacks; host-pointer I/O equals device-pointer I/O."""
    script, n, P = DK.GPU_SCRIPTS["reset_and_bank"]()
    y, e, _, _ = compare("reset_and_bank", cuda)
    assert DK.bits_equal(y[:, :356], y[:, 356:712]), first_mismatch(y[:, :356], y[:, 356:712])
    host = ofx.Engine("drumkit", n, voices=P)
    for step in script[:5]:
        apply(host, step, P)
    yh = host.process(None, out=np.empty((2, 256, n), np.float32))
    assert DK.bits_equal(yh, y[:, :256]), first_mismatch(yh, y[:, :256])


def test_long_oneshot_crosses_65536(cuda, rcp_table):
    y, _, _, _ = compare("long_oneshot", cuda)
    assert y[0, 69000:70000, 0].any()


def test_composed_engines(cuda):
    """130 kits of 4 voices against the three launches the kind replaces -- a voice_sample engine of 520 voices
    (voice p * 130 + i) with each voice's own parameters, olfx_mix with one bus per kit listing its mapped voices
    by ascending note, an fxrack engine at the kits' topologies: bit-identical, no oracle involved."""
    import torch
    n, P = 130, 4
    script = DK.script_sum_order(n, P)
    p, bank, recs, kmap, evs = (s[1] for s in script[:5])
    kit = ofx.Engine("drumkit", n, voices=P)
    voice = ofx.Engine("voice_sample", P * n)
    rack = ofx.Engine("fxrack", n)
    assert (voice.kernel_name, rack.kernel_name) == ("sampler_block_v1", "fxrack_block_v3")
    for step in script[:5]:
        apply(kit, step, P)
    voice.set_params(0, np.concatenate([p[q * DK.NV:(q + 1) * DK.NV] for q in range(P)], 1))
    rack.set_params(0, p[DK.RACK0:])
    voice.sample_bank(bank)
    voice.sample_voices([(slot * n + k, *rest) for k, slot, *rest in recs])
    note_at = {(k, note): v for k, _, note, v in kmap}
    order = [[v * n + k for note in range(128) for v in [note_at.get((k, note))] if v is not None] for k in range(n)]
    assert sum(o != sorted(o) for o in order) > n // 2
    voice.mix_config(order)
    voice.note_events([(note_at[(k, note)] * n + k, t, note) for k, t, note in evs])
    ys, yc = [], []
    for frames in (256, 20, 256):
        ys.append(process(kit, frames, cuda))
        vo = torch.empty((1, frames, P * n), device=cuda)
        x = torch.zeros((2, frames, n), device=cuda)
        voice.process(None, out=vo)
        bus = voice.mix(vo, x[0])
        assert bus.data_ptr() == x.data_ptr()
        yc.append(rack.process(x).cpu().numpy())
    y, yc = np.concatenate(ys, 1), np.concatenate(yc, 1)
    assert np.isfinite(yc).all() and yc[0].any(axis=0).all()
    assert np.array_equal(y.view(np.uint32), yc.view(np.uint32)), first_mismatch(y, yc)
