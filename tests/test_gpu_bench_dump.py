"""bench.py --dump-outputs: the arrays written are what a caller of the timed path receives after
the last timed step, bit for bit, and a plain run does the headline's work only."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_is_the_last_timed_block(cuda, tmp_path):
    """A plain chorus run of W + K = 1 + 3 blocks over a two-block input pool, 20,000 instances (a
    40 MB output: past DUMP_BYTES, so a sample of the instance columns is kept): out.npy equals the
    same columns of the fourth block of an engine fed the same workload in this process."""
    import torch

    import bench
    import ol_dsp_amd as ofx
    from ol_dsp_amd.workload import instance_params, noise_torch

    n, B, W, K = 20000, 256, 1, 3
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "chorus",
           "--instances", str(n), "--steps", str(K), "--warmup", str(W), "--leg-warmup", "0",
           "--pool-bytes", "1e8", "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-4000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert res["steps"] == K and res["warmup"] == W and res["frames"] == n * B * K
    assert res["reps"]["n"] == 1 and "also" not in res and res["parity"] is None and res["cpu_baseline"] is None
    assert res["ms_per_step"] > 0 and abs(res["value"] - res["frames"] / (res["ms_per_step"] * K / 1e3)) <= 1e-6 * res["value"]
    assert sorted(os.listdir(tmp_path)) == ["out.npy"]
    got = np.load(tmp_path / "out.npy")
    keep = bench.DUMP_BYTES // (2 * B * 4)
    assert keep < n and got.dtype == np.float32 and got.shape == (2, B, keep)
    assert got.nbytes <= 64e6 and res["dump_outputs"]["out"]["shape"] == [2, B, keep]

    pool = noise_torch(0, n, B, 2, cuda, blocks=2)
    eng = ofx.Engine("chorus", n, sample_rate=48000.0, block=B)
    eng.set_params(0, instance_params("chorus", 0, n))
    for k in range(W + K):
        y = eng.process(pool[k % 2])
    torch.cuda.synchronize()
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(n, keep, replace=False))
    want = y.cpu().numpy()[:, :, idx]
    eng.close()
    assert np.isfinite(want).all() and np.abs(want).max() > 0
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
