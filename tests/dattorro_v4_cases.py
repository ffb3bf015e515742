"""dattorro_block_v4 at small, ragged shapes: the cases, and the process that runs them.

The engine picks dattorro_block_v4 only for 2 x 64 x CUs instances and more, so the small-shape reverb
tests (test_gpu_parity.py, test_gpu_edges.py) run dattorro_block_v5.  OLFX_DT_V4=1 forces v4 for
uniform pre-delays at any size; the library reads it once per process, so these cases run in a child
process that tests/test_gpu_dattorro_v4.py starts with the variable set:

    OLFX_DT_V4=1 python tests/dattorro_v4_cases.py --report out.json     # every case, in order
    python tests/dattorro_v4_cases.py --list                             # the case names

The report maps case -> {"ok", "detail", "kernels"} (the kernel names the engine reported).  A
mismatch (AssertionError) is recorded and the run goes on; any other exception (an OLFX_E_HIP, an
illegal access) ends the run there, the cases after it are reported as not run, nothing is retried.
Every comparison is bit for bit against O.Dattorro (same_bits_or_nan on the edge signals), and every
case asserts the kernel name after its first block (before it the name is not meaningful).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, os.path.join(ROOT, "oracle"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import oracle as O  # noqa: E402
from helpers import (EDGE_BLOCKS, EDGE_FRAMES, UNIFORM_PD_RUNS, bits_equal, dt_corner_params,  # noqa: E402
                     dt_edge_params, dt_params, dt_reference_cases, edge_signals, fast_noise, first_mismatch,
                     first_mismatch_or_nan, lr_hashes, noise_block, nonfinite_share, poison_table, poisoned,
                     predelay_value, run_dattorro, same_bits_or_nan, subnormal_share)
from test_gpu_edges import (CONTAIN_CALLS, SIGNALS, _assert_contained, _guarded_numpy,  # noqa: E402
                            _guarded_torch)
from test_gpu_parity import _tiny_blocks, engine, run_gpu  # noqa: E402

V4, V5 = "dattorro_block_v4", "dattorro_block_v5"
CUDA = None           # torch.device, set by main()
KERNELS: list = []    # the names the running case has seen, in order, repeats dropped
LONG_BLOCKS = [60] + [4096] * 16 + [3900, 504]          # 70,000 frames; 4,096: a launch re-reads its writes
SWEEP_BLOCKS = [256, 4, 1028, 60]
EDGE_PD = 3           # the edge cases' one pre-delay, in samples: PreTap's register path


def _name(e, want=V4):
    k = e.kernel_name
    if KERNELS[-1:] != [k]:
        KERNELS.append(k)
    assert k == want, f"the engine ran {k}, not {want}"


def _run(e, x, blocks, want=V4):
    """run_gpu, with the network's name checked after the first block."""
    y = run_gpu(e, x[:, :blocks[0]], blocks[:1], CUDA)
    _name(e, want)
    if len(blocks) > 1:
        y = np.concatenate([y, run_gpu(e, x[:, blocks[0]:], blocks[1:], CUDA)], 1)
    return y


def _pair(n, p):
    e, ref = engine("dattorro", n), O.Dattorro(n)
    e.set_params(0, p)
    for i in range(n):
        for f in range(7):
            ref.set(i, f, float(p[f, i]))
    return e, ref


def _set_predelay(e, ref, pd):
    e.set_params("pre_delay", np.ascontiguousarray(pd[None, :], np.float32))
    for i in range(len(pd)):
        ref.set(i, 0, float(pd[i]))


def _exact(y, yr):
    assert bits_equal(y, yr), first_mismatch(y, yr)


def _golden():
    with open(os.path.join(HERE, "golden", "golden.json")) as f:
        return json.load(f)


# ------------------------------------------------------------- a. the real reference's fixtures
def ref_impulse():
    e = engine("dattorro", 1)
    x = np.zeros((2, 48000, 1), np.float32)
    x[:, 0, 0] = 1.0
    y = _run(e, x, [256] * 187 + [128])
    first = np.load(os.path.join(HERE, "golden", "dattorro_impulse_4096.npy"))
    _exact(y[:, :4096, 0], first)
    assert lr_hashes(y) == [_golden()["dattorro_impulse"]["fnv1a64"]]


def ref_noise_10s():
    g = _golden()["dattorro_noise_10s"]
    x1 = O.xorshift_noise(g["seed"], g["frames"])
    y = _run(engine("dattorro", 1), np.stack([x1, x1])[:, :, None], [4096] * 117 + [768])
    assert lr_hashes(y) == [g["fnv1a64"]]


def ref_sweep(k):
    g = _golden()["dattorro_sweep"][k]
    e = engine("dattorro", g["n"])
    e.set_params(0, np.asarray(g["params"], np.float32))
    x = noise_block(g["n"], g["frames"], g["input_base"])
    frames = g["frames"]
    y = _run(e, x, [256] * (frames // 256) + ([frames % 256] if frames % 256 else []))
    assert lr_hashes(y) == g["fnv1a64"], g["pre_delay"]


def ref_run(name):
    """A uniform-pre-delay run recorded from the reference build (dattorro_reference_runs.json)."""
    with open(os.path.join(HERE, "golden", "dattorro_reference_runs.json")) as f:
        recorded = json.load(f)[name]["fnv1a64"]
    p, x = dt_reference_cases()[name]
    e = engine("dattorro", x.shape[2])
    e.set_params(0, p)
    y = _run(e, x, LONG_BLOCKS if x.shape[1] == 70000 else SWEEP_BLOCKS + [700])
    assert np.all(np.isfinite(y))
    assert lr_hashes(y) == recorded


# ------------------------------------------------------------------------------ b. ragged n
def ragged(n):
    p = dt_params(np.random.default_rng(n), n, 0.1)
    x = fast_noise(n, 1536, seed=n)
    e, ref = _pair(n, p)
    _exact(_run(e, x, [256, 512, 4, 764]), ref.process(x, threads=8))


# ------------------------------------------------------------------------------ c. long run
def long_run(n, d):
    """70,000 frames: ModTap's extra-step reloads at the turn (t = 32768) and the uint16 wrap, calls
    off the 16-position rows, 4,096-frame launches (the 1,024-position rings re-read in the launch)."""
    p = dt_params(np.random.default_rng(85), n, 0.0)
    p[0] = predelay_value(d)
    x = fast_noise(n, 70000, seed=85)
    e, ref = _pair(n, p)
    _exact(_run(e, x, LONG_BLOCKS), ref.process(x, threads=8))


# ----------------------------------------------------------------- d. uniform pre-delay sweep
def predelay_sweep():
    """One engine, every instance set to d samples between calls: PreTap's register selects (0..8),
    the first ring delays, the block and ring edges and past them.  Uniform -> uniform: v4 throughout."""
    n = 70
    rng = np.random.default_rng(82)
    e, ref = _pair(n, dt_params(rng, n, 0.2))
    ys, yrs = [], []
    for k, d in enumerate([0, 1, 2, 3, 4, 5, 7, 8, 9, 10, 255, 256, 257, 4799, 4800, 8191, 8192, 8193, 65535]):
        _set_predelay(e, ref, np.full(n, predelay_value(d)))
        x = fast_noise(n, sum(SWEEP_BLOCKS), seed=820 + k)
        ys.append(_run(e, x, SWEEP_BLOCKS))
        yrs.append(ref.process(x, threads=8))
    y, yr = np.concatenate(ys, 1), np.concatenate(yrs, 1)
    _exact(y, yr)


# ---------------------------------------------------------------- e. layout conversions, small n
def layout_switches(n):
    """dattorro_pre_layout at an n off its 256-thread blocks, on a ring that has wrapped (9,220
    frames before the first switch), each switch right after a 4- or 60-frame call (t0 off the
    16-position rows): uniform -> per instance -> uniform -> per instance, then reset()."""
    rng = np.random.default_rng(83 + n)
    p = dt_params(rng, n, 0.2)
    e, ref = _pair(n, p)
    far = np.arange(8150, 8192)
    edge = np.concatenate([np.array([0, 1, 2, 3, 4, 7, 8, 255, 256, 257, 4800, 8191, 8193], np.float64) / 4800,
                           (far + 0.5) / 4800]).astype(np.float32)
    assert np.array_equal((edge[-len(far):] * np.float32(4800.0)).astype(np.uint16), far) and len(edge) <= n
    ys, yrs = [], []
    for step, (blocks, want) in enumerate([([4096, 4096, 1024, 4], V4), (SWEEP_BLOCKS, V5), (SWEEP_BLOCKS, V4),
                                           (SWEEP_BLOCKS, V5)]):
        if want == V5:
            pd = rng.uniform(0, 1, n).astype(np.float32)
            pd[:len(edge)] = edge
            _set_predelay(e, ref, pd)
        elif step:
            _set_predelay(e, ref, np.full(n, 0.05, np.float32))
        x = fast_noise(n, sum(blocks), seed=830 + step)
        ys.append(_run(e, x, blocks, want))
        yrs.append(ref.process(x, threads=8))
    y, yr = np.concatenate(ys, 1), np.concatenate(yrs, 1)
    _exact(y, yr)
    e.reset()
    e.set_params(0, p)
    x = fast_noise(n, 512, seed=99)
    _exact(_run(e, x, [512]), run_dattorro(O.Dattorro(n), p, x))


# ------------------------------------------------------------------------------ f. fp32 edges
def _edge_params(n):
    p = dt_edge_params(n)
    p[0] = predelay_value(EDGE_PD)
    return p


def _same(y, yr):
    assert same_bits_or_nan(y, yr), first_mismatch_or_nan(y, yr)


def edge_signal(signal, n):
    """test_gpu_edges.test_signal_edges' reverb rows on v4, with its oracle-side conditions; loud127
    (x * 2^127): the oracle stays finite and peaks above 2^126, within a factor 4 of overflow."""
    x = edge_signals(fast_noise(n, EDGE_FRAMES, seed=40))[signal]
    e, ref = _pair(n, _edge_params(n))
    yr = ref.process(x, threads=8)
    sub, nonfin = subnormal_share(yr), nonfinite_share(yr)
    print(f"dattorro v4 n={n} {signal}: oracle subnormal share of non-zero {100 * sub:.1f} %, "
          f"non-finite share {100 * nonfin:.1f} %, peak {np.abs(yr[np.isfinite(yr)]).max():.3g}")
    if signal == "subnormal":
        assert np.any(yr != 0) and sub >= 0.5
    if signal == "loud100":
        assert nonfin == 0
    if signal == "loud127":
        assert nonfin == 0 and np.abs(yr).max() >= 2.0 ** 126
    _same(_run(e, x, EDGE_BLOCKS), yr)


def poisoned_instances(n):
    x = fast_noise(n, EDGE_FRAMES, seed=40)
    xp = poisoned(x)
    p = _edge_params(n)
    e, ref = _pair(n, p)
    yr = ref.process(xp, threads=8)
    bad = sorted({i for _, _, i, _ in poison_table(n)})
    assert len(bad) == 5 and all(not np.all(np.isfinite(yr[:, :, i])) for i in bad)
    y = _run(e, xp, EDGE_BLOCKS)
    _same(y, yr)
    yc = _run(_pair(n, p)[0], x, EDGE_BLOCKS)
    clean = np.setdiff1d(np.arange(n), bad)
    assert np.all(np.isfinite(yc))
    _exact(y[:, :, clean], yc[:, :, clean])


def corners(pre_delay):
    """The 128 corners of the setters with one pre-delay for all: 0 samples, then 4800."""
    n = 128
    p = dt_corner_params()
    p[0] = pre_delay
    x = fast_noise(n, 4096, seed=4)
    e, ref = _pair(n, p)
    yr = ref.process(x, threads=8)
    assert np.all(np.isfinite(yr))
    _same(_run(e, x, [256] * 8 + [4, 2044]), yr)


# ----------------------------------------------------------------------------- g. containment
def contained(n, host):
    """test_gpu_edges' guarded buffers: 64 NaN guard floats on each side of in and out, aligned and
    offset by one float, calls of 4, 20 and 260 frames, device or host buffers."""
    import torch
    x = fast_noise(n, sum(CONTAIN_CALLS), seed=n)
    for offset in (0, 1):
        e, ref = _pair(n, _edge_params(n))
        yr = ref.process(x, threads=8)
        outs, f0 = [], 0
        for b in CONTAIN_CALLS:
            if host:
                obuf, oview = _guarded_numpy(2 * b * n, offset)
                xin = _guarded_numpy(2 * b * n, offset)[1].reshape(2, b, n)
                xin[...] = x[:, f0:f0 + b]
                out = oview.reshape(2, b, n)
                assert e.process(xin, out=out) is out and np.shares_memory(out, obuf)
            else:
                obuf, oview = _guarded_torch(2 * b * n, offset, CUDA)
                xin = _guarded_torch(2 * b * n, offset, CUDA)[1].view(2, b, n)
                xin.copy_(torch.from_numpy(np.ascontiguousarray(x[:, f0:f0 + b])))
                e.process(xin, out=oview.view(2, b, n))
                torch.cuda.synchronize()
                out = oview.view(2, b, n).cpu().numpy()
            if not f0:
                _name(e)
            _assert_contained(obuf, offset, 2 * b * n)
            outs.append(out.copy())
            f0 += b
        _same(np.concatenate(outs, 1), yr)


# ------------------------------------------------------------------------- h. small API cases
def host_io_equals_device_io():
    n = 100
    x = fast_noise(n, 512, seed=5)
    e1, e2 = engine("dattorro", n), engine("dattorro", n)
    yd = _run(e1, x, [512])
    yh = e2.process(x)
    _name(e2)
    _exact(yd, yh)


def tiny_blocks(n):
    rng = np.random.default_rng(1000 + n)
    x = fast_noise(n, 3000, seed=n + 7)
    blocks = _tiny_blocks(rng, 3000)
    p = dt_params(rng, n, 0.0)
    p[0] = predelay_value(int(rng.integers(0, 49)))
    e, ref = _pair(n, p)
    _exact(_run(e, x, blocks), ref.process(x, threads=8))


def param_change():
    n = 40
    x = fast_noise(n, 1024, seed=4)
    rng = np.random.default_rng(4)
    p1, p2 = dt_params(rng, n, 0.0), dt_params(rng, n, 0.0)
    e, ref = _pair(n, p1)
    ya, yra = _run(e, x[:, :512], [512]), ref.process(x[:, :512])
    e.set_params(1, p2[1:])
    for i in range(n):
        for f in range(1, 7):
            ref.set(i, f, float(p2[f, i]))
    yb, yrb = _run(e, x[:, 512:], [512]), ref.process(x[:, 512:])
    _exact(np.concatenate([ya, yb], 1), np.concatenate([yra, yrb], 1))


def _cases() -> dict:
    c = {"ref_impulse": ref_impulse, "ref_noise_10s": ref_noise_10s}
    for k in range(4):
        c[f"ref_sweep_{k}"] = lambda k=k: ref_sweep(k)
    for name in UNIFORM_PD_RUNS:
        c["ref_" + name] = lambda name=name: ref_run(name)
    for n in (1, 63, 70, 72, 300):
        c[f"ragged_n{n}"] = lambda n=n: ragged(n)
    for n in (70, 72):
        for d in (37, 8191):
            c[f"long_run_n{n}_pd{d}"] = lambda n=n, d=d: long_run(n, d)
    c["predelay_sweep"] = predelay_sweep
    for n in (70, 96, 300):
        c[f"layout_switches_n{n}"] = lambda n=n: layout_switches(n)
    for n in (70, 72):
        for s in SIGNALS + ["loud127"]:
            c[f"edge_{s}_n{n}"] = lambda s=s, n=n: edge_signal(s, n)
        c[f"poisoned_n{n}"] = lambda n=n: poisoned_instances(n)
    c["corners_pd0"] = lambda: corners(0.0)
    c["corners_pd4800"] = lambda: corners(1.0)
    for n in (1, 63, 70, 72):
        c[f"contained_device_n{n}"] = lambda n=n: contained(n, host=False)
        c[f"contained_host_n{n}"] = lambda n=n: contained(n, host=True)
    c["host_io_equals_device_io"] = host_io_equals_device_io
    for n in (1, 70):
        c[f"tiny_blocks_n{n}"] = lambda n=n: tiny_blocks(n)
    c["param_change"] = param_change
    return c


CASES = _cases()


def main(argv=None) -> int:
    global CUDA
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--list", action="store_true", help="print the case names and exit")
    ap.add_argument("--report", default="dattorro_v4_report.json", help="where the JSON report goes")
    args = ap.parse_args(argv)
    if args.list:
        print("\n".join(CASES))
        return 0
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU is visible")
    CUDA = torch.device("cuda:0")
    print(f"OLFX_DT_V4={os.environ.get('OLFX_DT_V4')!r}", flush=True)
    report, ended = {}, None
    t_all = time.perf_counter()
    for name, fn in CASES.items():
        if ended:
            report[name] = {"ok": False, "detail": f"not run: {ended}", "kernels": []}
            continue
        KERNELS.clear()
        t0 = time.perf_counter()
        try:
            fn()
            ok, detail = True, ""
        except AssertionError as err:
            ok, detail = False, f"mismatch: {err}"
        except Exception as err:       # a HIP error or anything else unexpected: launch nothing more
            ok, detail = False, f"{type(err).__name__}: {err}"
            ended = f"the run ended at {name} ({detail})"
        report[name] = {"ok": ok, "detail": detail, "kernels": list(KERNELS)}
        print(f"{name}: {'ok' if ok else 'FAILED ' + detail} {report[name]['kernels']} "
              f"{time.perf_counter() - t0:.2f} s", flush=True)
    with open(args.report, "w") as f:
        json.dump(report, f, indent=1)
    print(f"{sum(r['ok'] for r in report.values())} of {len(report)} cases ok, "
          f"{time.perf_counter() - t_all:.1f} s", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
