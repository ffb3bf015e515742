"""OLFX_KIND_PLATERACK (platerack_block_v1: delay -> Dattorro plate -> filter in one launch) on the
GPU, bit-exact against tests/platerack_ref.py -- the existing oracles composed: O.FxRack's DelayFx
and FilterFx alone around the reference's own verb.cpp build.  Small ragged shapes: a partly filled
wave, a delay wave with no instance at all (n = 1, 33, 65: the group's second half is empty or one
instance), two groups and more (65, 130), chunks of 4 .. 16 frames, every line delay at which the
delay stage's window takes another position, both of the engine's clocks across their turns."""
import ctypes

import numpy as np
import pytest

import ol_dsp_amd as ofx
import platerack_ref as PR
from helpers import bits_equal, fast_noise, first_mismatch
from ol_dsp_amd import _lib, workload
from test_gpu_parity import engine, run_gpu

pytestmark = pytest.mark.gpu

LINE_DELAYS = [0, 1, 15, 16, 17, 24000, 47999]        # DelayLine delay_ D (integer part)
TIME, TOPO, FTYPE = 0, 11, 9                            # OLFX_FR_* fields
PRE = 12                                                # OLFX_PR_VERB0 + OLFX_DT_PREDELAY


def delay_time(d):
    """OLFX_FR_DELAY_TIME whose line delay is d samples and a half: (d + 0.5) / 48000, checked to
    give d back through the setter's int(scale(time, 0, 1, 0, 48000, 1))."""
    t = np.float32((d + 0.5) / 48000.0)
    assert int(t * np.float32(48000.0)) == d
    return t


def params(n, seed):
    """[19][n]: the section 8d ranges (workload.RANGES: rack fields, plate fields with pre-delays
    0..1, filter type 0..4), topology drawn from {0, 1}, and the line delays of LINE_DELAYS forced
    onto the first and the last instances."""
    p = workload.instance_params("platerack", 0, n, seed)
    rng = np.random.default_rng(seed)
    p[TOPO] = rng.integers(0, 2, n).astype(np.float32)
    for k, d in enumerate(LINE_DELAYS):
        p[TIME, k % n] = delay_time(d)
        p[TIME, (n - 1 - k) % n] = delay_time(LINE_DELAYS[-1 - k])
    assert set(np.unique(p[FTYPE])) <= {0.0, 1.0, 2.0, 3.0, 4.0}
    return p


def pair(n, p):
    e = engine("platerack", n)
    assert e.kernel_name == "platerack_block_v1"
    ref = PR.PlateRack(n)
    if p is not None:
        e.set_params(0, p)
        ref.set_params(p)
    return e, ref


@pytest.mark.parametrize("n", [1, 33, 65, 130])
def test_ragged_instances(cuda, n):
    p = params(n, 100 + n)
    if n >= 7:
        d = (p[TIME] * np.float32(48000.0)).astype(np.int64)
        assert set(LINE_DELAYS) <= set(d.tolist())
        assert {0.0, 1.0} <= set(p[TOPO].tolist())
    x = fast_noise(n, 768, seed=n)
    e, ref = pair(n, p)
    y = run_gpu(e, x, [256] * 3, cuda)
    yr = np.concatenate([ref.process(x[:, f:f + 256], threads=4) for f in (0, 256, 512)], 1)
    assert bits_equal(y, yr), first_mismatch(y, yr)
    assert np.any(y[0] != 0)
    fw = p[TOPO] == 1.0
    assert np.all(y[1][:, ~fw] == 0) and (not fw.any() or np.any(y[1][:, fw] != 0))


def test_ragged_frames(cuda):
    n, blocks = 65, [4, 20, 36, 256, 12]
    p = params(n, 7)
    x = fast_noise(n, sum(blocks), seed=8)
    e, ref = pair(n, p)
    y = run_gpu(e, x, blocks, cuda)
    yr = ref.process(x, threads=4)
    assert bits_equal(y, yr), first_mismatch(y, yr)


def test_groups_back_to_back(cuda):
    """More groups than workgroups -- the one path a small engine cannot reach: a workgroup runs
    two or three 64-instance groups back to back, its queues and counters running on across them
    and every role starting over on the next group's instances; the last group is ragged (37 of 64).
    Blocks of 256, 20 and 256 frames; sampled instances of the first, middle and last groups of
    several workgroups against the helper."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = cus * 64 * 2 + 37
    idx = np.array(sorted({0, 31, 32, 63, 64, cus * 64 - 1, cus * 64, cus * 64 + 65, 2 * cus * 64 - 1,
                           2 * cus * 64, 2 * cus * 64 + 17, n - 1}), np.int64)
    p = workload.instance_params("platerack", 0, n, 5)
    p[TOPO] = np.random.default_rng(5).integers(0, 2, n).astype(np.float32)
    for k, i in enumerate(idx):
        p[TIME, i] = delay_time(LINE_DELAYS[k % len(LINE_DELAYS)])
    xs = workload.noise_torch(0, n, 256, 2, cuda, blocks=2)
    xs = [xs[0], xs[1][:, :20].contiguous(), xs[1]]
    e = engine("platerack", n)
    e.set_params(0, p)
    y = torch.cat([e.process(x) for x in xs], 1)
    assert torch.isfinite(y).all()
    ref = PR.PlateRack(len(idx))
    ref.set_params(np.ascontiguousarray(p[:, idx]))
    yr = np.concatenate([ref.process(np.ascontiguousarray(x[:, :, idx].cpu().numpy())) for x in xs], 1)
    yg = y[:, :, idx].cpu().numpy()
    assert bits_equal(yg, yr), first_mismatch(yg, yr)


def test_both_clocks(cuda):
    """70,000 frames in 256-frame blocks and the tail: the rack ring wraps at 48,000 (one instance
    reads at D = 47999, one at 0: the sample written 48,000 frames before), the plate's modulation
    turns at t = 32768 and its 16-bit clock wraps at 65,536."""
    n, frames = 5, 70000
    p = params(n, 9)
    p[TIME, 0], p[TIME, 1] = delay_time(47999), delay_time(0)
    p[1] = np.minimum(p[1], 0.6)                        # feedback: a bounded tail over 70,000 frames
    x = fast_noise(n, frames, seed=10)
    blocks = [256] * (frames // 256) + [frames % 256]
    assert blocks[-1] % 4 == 0 and sum(blocks) == frames
    e, ref = pair(n, p)
    y = run_gpu(e, x, blocks, cuda)
    yr = ref.process(x, threads=5)
    assert bits_equal(y, yr), first_mismatch(y, yr)
    assert np.any(y[0, 66000:] != 0) and np.isfinite(y).all()


def test_control_storm(cuda):
    """Between blocks: the reverb CC table (MIDI and hardware), delay / filter / volume CCs, the two
    update-only controls, one pre-delay change and one topology flip.  The helper gets the mapped
    values (ofx.control_map, pure host code)."""
    n, B = 8, 256
    p = params(n, 11)
    p[TOPO] = 0.0
    p[TOPO, 5] = 1.0
    x = fast_noise(n, 5 * B, seed=12)
    e, ref = pair(n, p)
    names = ofx.PARAMS[ofx.KIND_PLATERACK]
    rng = np.random.default_rng(13)
    reverb_ccs = [32, 53, 54, 56, 55, 34, 33, 52, 50]

    def send(inst, cc, value, source, as_cc=None):
        e.control([(inst, cc, value, source)])
        m = ofx.control_map("platerack", cc if as_cc is None else as_cc, value, source)
        assert m is not None
        if m[0] != "update_only":
            ref.set(inst, names.index(m[0]), m[1])
            assert e.get_param(inst, m[0]) == np.float32(m[1])

    ys, yr = [], []
    for b in range(5):
        if b == 1:
            for k, cc in enumerate(reverb_ccs):          # every reverb CC, both sources, topology 0 and 1
                send(k % 4, cc, float(rng.integers(10, 118)), "midi")
                send(4 + k % 4, cc, float(rng.uniform(0.1, 0.9)), "hw")
        if b == 2:
            for cc in (35, 36, 39, 37, 38):              # delay CCs (37, 38: MIDI only)
                send(1, cc, float(rng.integers(5, 100)), "midi")
            for cc in (45, 46, 48, 7):                   # rack filter and master volume, topology 0
                send(2, cc, float(rng.integers(5, 100)), "midi")
            send(2, 47, 70.0, "midi")                    # filter type
            send(5, 41, 50.0, "midi", as_cc=45)          # topology 1: the voice-filter CC drives filter1
            before = e.get_param(5, "master_volume")
            e.control([(5, 7, 100.0), (5, 45, 3.0)])     # ... and CC 7 / 45 reach nothing
            assert e.get_param(5, "master_volume") == before
        if b == 3:
            e.set_param(3, "verb_pre_delay", 0.77)       # lands at this block boundary
            ref.set(3, "verb_pre_delay", 0.77)
            e.set_param(6, "topology", 1.0)              # FxRack<2> -> the firmware callback
            ref.set(6, "topology", 1.0)
            e.set_param(5, "topology", 0.0)
            ref.set(5, "topology", 0.0)
        xb = np.ascontiguousarray(x[:, b * B:(b + 1) * B])
        ys.append(run_gpu(e, xb, [B], cuda))
        yr.append(ref.process(xb, threads=4))
    y, yr = np.concatenate(ys, 1), np.concatenate(yr, 1)
    assert bits_equal(y, yr), first_mismatch(y, yr)
    with pytest.raises(ofx.OlfxError):
        e.set_param(0, "topology", 2.0)
    with pytest.raises(ofx.OlfxError):
        e.set_param(0, "verb_pre_delay", 14.0)


def test_reset_and_host_io(cuda):
    """olfx_reset followed by a run equals a fresh engine (defaults again, both clocks at 0), and
    host-pointer I/O equals device-pointer I/O."""
    n = 37
    p = params(n, 15)
    x = fast_noise(n, 600, seed=16)
    e, _ = pair(n, p)
    run_gpu(e, fast_noise(n, 1000, seed=17), [256, 256, 256, 232], cuda)
    e.reset()
    assert e.frames_processed == 0
    e.set_params(0, p)
    fresh, ref = pair(n, p)
    y = run_gpu(e, x, [256, 256, 88], cuda)
    yf = run_gpu(fresh, x, [256, 256, 88], cuda)
    assert bits_equal(y, yf), first_mismatch(y, yf)
    yr = ref.process(x, threads=4)
    assert bits_equal(yf, yr), first_mismatch(yf, yr)
    host, _ = pair(n, p)
    yh = np.concatenate([host.process(np.ascontiguousarray(x[:, a:b])) for a, b in ((0, 256), (256, 512), (512, 600))], 1)
    assert bits_equal(yh, yf), first_mismatch(yh, yf)
    # a reset engine without parameters is a default engine
    e.reset()
    d, dref = pair(n, None)
    y0, y1 = run_gpu(e, x, [600], cuda), run_gpu(d, x, [600], cuda)
    assert bits_equal(y0, y1) and bits_equal(y1, dref.process(x, threads=4))


def test_sample_objects_one_block_late(cuda):
    """Two olfx_sample objects of the kind, 600 frames, frame-major: the engine's output one block
    (256 frames) late."""
    lib = ofx.load()
    n, B, T = 2, 256, 600
    p = params(n, 19)
    x = fast_noise(n, T, seed=20)
    assert lib.olfx_sample_pool_config(0, B) == 0
    objs = []
    for i in range(n):
        h = ctypes.c_void_p()
        assert lib.olfx_sample_create(_lib.KIND_PLATERACK, 48000.0, ctypes.byref(h)) == 0
        for f in range(p.shape[0]):
            assert lib.olfx_sample_set_param(h, f, float(p[f, i])) == 0
        objs.append(h)
    assert lib.olfx_sample_latency(objs[0]) == B
    y = np.zeros((2, T, n), np.float32)
    fin, fout = (ctypes.c_float * 2)(), (ctypes.c_float * 2)()
    for t in range(T):
        for i, h in enumerate(objs):
            fin[0], fin[1] = float(x[0, t, i]), float(x[1, t, i])
            assert lib.olfx_sample_process(h, fin, fout) == 0, (t, i)
            y[0, t, i], y[1, t, i] = fout[0], fout[1]
    assert lib.olfx_sample_generation_size(objs[0]) == n
    for h in objs:
        assert lib.olfx_sample_destroy(h) == 0
    e, ref = pair(n, p)
    ye = run_gpu(e, x[:, :512], [B, B], cuda)
    assert not np.any(y[:, :B])
    assert bits_equal(y[:, B:], ye[:, :T - B]), first_mismatch(y[:, B:], ye[:, :T - B])
    yr = np.concatenate([ref.process(x[:, :B]), ref.process(x[:, B:512])], 1)
    assert bits_equal(ye, yr), first_mismatch(ye, yr)
