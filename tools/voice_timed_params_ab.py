#!/usr/bin/env python3
"""Parameter changes inside the block: one olfx_process with olfx_timed_params against one olfx_process per
parameter time.

tools/voice_timed_ab.py's shape -- 32,768 voices x 256 frames, every voice sounding -- with a cutoff change on 5 %
of the voices every block, rotating over the voices, spread over S distinct times, S in {1, 2, 4, 16}: change j of
the block sits at frame (j mod S) * (256 / S), so S = 1 is all at frame 0 (the unsegmented launch, a plain
set_param_list for either leg).  Per kind and S, two legs over the same schedule:

  timed: the block's changes through Engine.timed_params, one process call of 256 frames;
  split: per time, that time's changes through Engine.set_param_list and a process call up to the next time.

Device events around `--steps` blocks per region after `--warmup` blocks, the median (min - max) of `--reps` regions;
the per-block record arrays are prebuilt, so a step is the library calls alone.  One JSON line.

`--parent DIR` also runs the split leg on DIR's ol_dsp_amd, a build of the parent commit, in a child process of the
same run: the baseline (a tree without olfx_timed_params has no timed leg).

  python tools/voice_timed_params_ab.py [--kinds voice,voice_moog] [--segments 1,2,4,16] [--parent ../parent]
                                        [--out profiles/voice_timed_params_ab.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUTOFF = 0                               # OLFX_VC_FILTER_CUTOFF


def schedule(n, k, S, block):
    """Block k's changes as (frames, inst, values): every 20th voice, rotating, the cutoff stepping with the block."""
    import numpy as np
    inst = np.nonzero(np.arange(n) % 20 == k % 20)[0]
    frame = (np.arange(len(inst)) % S) * (block // S)
    value = (400.0 + 120.0 * ((inst + 7 * k) % 60)).astype(np.float32)        # inside the workload's own range
    return frame.astype(np.uint32), inst.astype(np.uint32), value


def measure(args, tree, legs):
    sys.path.insert(0, os.path.abspath(tree))
    import numpy as np
    import torch

    import ol_dsp_amd as ofx
    from ol_dsp_amd import workload
    if not torch.cuda.is_available():
        sys.exit("voice_timed_params_ab: no GPU (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    n, B = args.instances, args.block
    cells = []
    for kind in args.kinds.split(","):
        for S in (int(s) for s in args.segments.split(",")):
            assert B % S == 0 and (B // S) % 4 == 0
            for leg in legs:
                e = ofx.Engine(kind, n, block=B)
                e.set_params(0, workload.instance_params(kind, 0, n))
                e.note_events(e.make_events(np.arange(n), 1, workload.voice_notes(0, n)))
                out = torch.empty((1, B, n), device=dev)
                steps = []
                for k in range(20):
                    frame, inst, value = schedule(n, k, S, B)
                    if leg == "timed":
                        steps.append(e.make_timed_params(frame, inst, CUTOFF, value))
                    else:
                        cuts = sorted(set(frame.tolist())) + [B]
                        steps.append([(inst[frame == f0], value[frame == f0], out[:, f0:f1]) for f0, f1 in zip(cuts, cuts[1:])])
                k = [0]

                def step():
                    st = steps[k[0] % 20]
                    k[0] += 1
                    if leg == "timed":
                        e.timed_params(st)
                        e.process(None, out=out)
                    else:
                        for ii, vv, o in st:
                            e.set_param_list(CUTOFF, ii, vv)
                            e.process(None, out=o)

                def region():
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    for _ in range(args.steps):
                        step()
                    t1.record()
                    t1.synchronize()
                    return t0.elapsed_time(t1) * 1e3 / args.steps           # us per block

                for _ in range(args.warmup):
                    step()
                us = [region() for _ in range(args.reps)]
                cells.append({"kind": kind, "segments": S, "leg": leg, "us_per_block_median": statistics.median(us),
                              "us_per_block": us, "changes_per_block": int(len(schedule(n, 0, S, B)[1])),
                              "finite": bool(torch.isfinite(out).all().item())})
                print(json.dumps(cells[-1]), file=sys.stderr, flush=True)
                del e
    return {"lib": os.path.relpath(ofx.LIB_PATH, os.path.abspath(tree)), "cells": cells}       # inside its tree


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kinds", default="voice,voice_moog")
    ap.add_argument("--segments", default="1,2,4,16")
    ap.add_argument("--instances", type=int, default=32768)
    ap.add_argument("--block", type=int, default=256)
    ap.add_argument("--steps", type=int, default=80, help="blocks per timed region (a multiple of 20: whole rotations)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--parent", default="", help="a build of the parent commit: its split leg is the baseline")
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)      # the tree this child process measures
    ap.add_argument("--out", default="", help="also write the JSON record here")
    args = ap.parse_args()
    if args.child:                           # the baseline process: the split leg on another tree's library
        print(json.dumps(measure(args, args.child, ["split"])))
        return
    res = {"instances": args.instances, "block": args.block, "steps": args.steps, "reps": args.reps, "warmup": args.warmup}
    res.update(measure(args, ROOT, ["timed", "split"]))
    if args.parent:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", args.parent] + \
              [f"--{k}={getattr(args, k)}" for k in ("kinds", "segments", "instances", "block", "steps", "reps", "warmup")]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        sys.stderr.write(r.stderr)
        if r.returncode != 0:
            sys.exit("voice_timed_params_ab: the parent's leg failed")
        base = json.loads(r.stdout.strip().splitlines()[-1])
        res["parent_lib"] = base["lib"]
        res["cells"] += [dict(c, leg="split_parent") for c in base["cells"]]
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
