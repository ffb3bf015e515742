#!/usr/bin/env python3
"""The plate rack's fused kernel against the cheapest path a user had before it.

  fused:    one OLFX_KIND_PLATERACK engine (platerack_block_v1), one launch per block;
  separate: an OLFX_KIND_FXRACK engine (fxrack_block_v3) into an OLFX_KIND_DATTORRO engine with
            per-instance pre-delays (the row-layout dattorro_block_v5), two launches per block and the
            rack's output through HBM -- and still without the balance mix against the plate.
Both get the same inputs and the same per-instance parameters (workload.RANGES["platerack"]: the
rack's fields, the plate's with pre-delays drawn from 0..1).  Device events around `--steps` blocks
per window, after a warm-up of each path; `--reps` windows per path, alternating the two paths in
one process.  Prints one JSON line (medians, ranges, B/frame figures at 8 TB/s).

  python tools/platerack_ab.py [--instances 16384] [--block 256] [--steps 50] [--reps 5]
  python tools/platerack_ab.py --only fused --steps 10      # untimed, for a rocprofv3 --pmc run
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12       # B/s, MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=16384)
    ap.add_argument("--block", type=int, default=256)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=["fused", "separate"], help="run one path untimed (profiler runs)")
    args = ap.parse_args()

    import torch

    import ol_dsp_amd as ofx
    from ol_dsp_amd import workload
    if not torch.cuda.is_available():
        sys.exit("platerack_ab: no GPU (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    n, B = args.instances, args.block
    p = workload.instance_params("platerack", 0, n)
    n_rack = len(ofx.PARAMS[ofx.KIND_FXRACK])
    xs = workload.noise_torch(0, n, B, 2, dev, blocks=4)
    out = torch.empty((2, B, n), device=dev)

    paths = {}
    if args.only != "separate":
        fused = ofx.Engine("platerack", n, block=B)
        fused.set_params(0, p)
        paths["fused"] = lambda k: fused.process(xs[k % 4], out=out)
    if args.only != "fused":
        rack, verb = ofx.Engine("fxrack", n, block=B), ofx.Engine("dattorro", n, block=B)
        rack.set_params(0, p[:n_rack])
        verb.set_params(0, p[n_rack:])
        mid = torch.empty((2, B, n), device=dev)

        def separate(k):
            rack.process(xs[k % 4], out=mid)
            verb.process(mid, out=out)
        paths["separate"] = separate

    def window(run, steps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for k in range(steps):
            run(k)
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) * 1e3 / steps           # us per block

    for run in paths.values():
        window(run, args.warmup)
    if args.only:
        window(paths[args.only], args.steps)
        print(json.dumps({"only": args.only, "instances": n, "block": B, "steps": args.steps}))
        return
    kernels = {"fused": fused.kernel_name, "separate": [rack.kernel_name, verb.kernel_name]}
    us = {name: [] for name in paths}
    for _ in range(args.reps):
        for name, run in paths.items():                     # alternating
            us[name].append(window(run, args.steps))
    res = {"instances": n, "block": B, "steps": args.steps, "reps": args.reps, "kernels": kernels}
    frames = n * B
    for name, v in us.items():
        res[name] = {"us_per_block_median": statistics.median(v), "us_per_block_min": min(v),
                     "us_per_block_max": max(v), "us_per_block": v}
    med = res["fused"]["us_per_block_median"] * 1e-6
    rw, rd = fused.algorithmic_bytes_per_frame, fused.algorithmic_read_bytes_per_frame
    res["fused"].update({
        "algorithmic_bytes_per_frame": rw, "algorithmic_read_bytes_per_frame": rd,
        "rw_fraction_of_8TBs": rw * frames / med / HBM_PEAK,
        "read_fraction_of_8TBs": rd * frames / med / HBM_PEAK,
        "instance_frames_per_s": frames / med})
    res["fused_over_separate_median"] = res["fused"]["us_per_block_median"] / res["separate"]["us_per_block_median"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
