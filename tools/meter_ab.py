#!/usr/bin/env python3
"""The level meter (meter_block_v1) against the rates this GPU sustains: both modes, both lane layouts.

  envelope: olfx_process with an output (4 B in + 4 B out per signal-frame): compare with bw_probe's copy row;
  summary:  olfx_process with out = NULL (4 B in): compare with bw_probe's read row;
  scalar:   one signal per lane, the default;
  quad:     four adjacent instances per lane where n % 4 == 0 and the planes are 16-B aligned (OLFX_MT_QUAD=1,
            read once per process: each layout runs in a process of its own).

Device events around `--steps` launches per region after `--warmup` launches, the median of `--reps` regions.  The
inputs (and the envelope outputs) rotate through pools larger than the Infinity Cache, so every launch streams
from HBM.  One JSON line per run; `--all` runs the four (layout, size) cells as child processes, then
tools/bw_probe where it has been built, and writes the lot to `--out`.

  python tools/meter_ab.py [--instances 65536] [--block 256] [--layout scalar|quad]
  python tools/meter_ab.py --all --out profiles/meter_ab.json
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
POOL_BYTES = 320 << 20            # more than the 256 MB Infinity Cache


def one(args):
    os.environ["OLFX_MT_QUAD"] = "0" if args.layout == "scalar" else "1"     # ahead of the first launch
    import torch

    import ol_dsp_amd as ofx
    if not torch.cuda.is_available():
        sys.exit("meter_ab: no GPU (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    n, B = args.instances, args.block
    block_bytes = 2 * B * n * 4
    pool = max(2, -(-POOL_BYTES // block_bytes) + 1)
    xs = [torch.rand((2, B, n), device=dev) - 0.5 for _ in range(pool)]
    ys = [torch.empty((2, B, n), device=dev) for _ in range(pool)]
    e = ofx.Engine("meter", n, block=B)
    k = [0]

    def envelope():
        k[0] = (k[0] + 1) % pool
        e.process(xs[k[0]], out=ys[k[0]])

    def summary():
        k[0] = (k[0] + 1) % pool
        e.meter(xs[k[0]])

    def region(run):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(args.steps):
            run()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) * 1e3 / args.steps           # us per launch

    res = {"instances": n, "block": B, "layout": args.layout, "steps": args.steps, "reps": args.reps,
           "warmup": args.warmup, "pool_buffers": pool, "kernel": e.kernel_name, "lib": os.path.basename(ofx.LIB_PATH),
           "algorithmic_bytes_per_frame": e.algorithmic_bytes_per_frame}
    for name, run, bytes_per_launch in (("envelope", envelope, 2 * block_bytes), ("summary", summary, block_bytes)):
        for _ in range(args.warmup):
            run()
        us = [region(run) for _ in range(args.reps)]
        med = statistics.median(us)
        res[name] = {"us_per_launch_median": med, "us_per_launch": us, "bytes_per_launch": bytes_per_launch,
                     "TBs": bytes_per_launch / (med * 1e-6) / 1e12}
    lv = e.levels(0, 4)
    res["levels_finite"] = bool(all(map(lambda a: bool((a == a).all()), lv.values())))
    print(json.dumps(res))


def probe():
    """bw_probe's read and copy rows (GB/s), or None where the program has not been built."""
    exe = os.path.join(ROOT, "tools", "bw_probe")
    if not os.path.exists(exe):
        return None
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600).stdout
    rows = {m.group(1): float(m.group(2)) for m in re.finditer(r"^(\w+)\s+R\d+ W\d+\s+([\d.]+) GB/s", out, re.M)}
    return {"read_GBs": rows.get("read"), "copy_GBs": rows.get("copy"), "rows": rows}


def everything(args):
    cells = []
    for n in (65536, 16384):
        for layout in ("quad", "scalar"):
            cmd = [sys.executable, os.path.abspath(__file__), "--instances", str(n), "--block", str(args.block), "--layout", layout,
                   "--steps", str(args.steps), "--reps", str(args.reps), "--warmup", str(args.warmup)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
            if r.returncode:
                sys.exit(f"meter_ab: {' '.join(cmd)} failed:\n{r.stdout}{r.stderr}")
            cells.append(json.loads(r.stdout.strip().splitlines()[-1]))
            print(json.dumps(cells[-1]), flush=True)
    res = {"cells": cells, "bw_probe": probe()}
    if res["bw_probe"] and res["bw_probe"]["copy_GBs"] and res["bw_probe"]["read_GBs"]:
        for c in cells:
            c["envelope"]["of_probe_copy"] = c["envelope"]["TBs"] * 1e3 / res["bw_probe"]["copy_GBs"]
            c["summary"]["of_probe_read"] = c["summary"]["TBs"] * 1e3 / res["bw_probe"]["read_GBs"]
    print(json.dumps(res["bw_probe"]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=65536)
    ap.add_argument("--block", type=int, default=256)
    ap.add_argument("--layout", choices=["quad", "scalar"], default="scalar")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--all", action="store_true", help="both layouts at 65,536 and 16,384 instances, then tools/bw_probe")
    ap.add_argument("--out", default="", help="with --all: the JSON file to write")
    args = ap.parse_args()
    everything(args) if args.all else one(args)


if __name__ == "__main__":
    main()
