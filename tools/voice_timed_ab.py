#!/usr/bin/env python3
"""Note events inside the block: one olfx_process with olfx_timed_events against one olfx_process per event time.

bench.py's `voice_events` shape and event density -- 32,768 voices x 256 frames, NoteOn for 2.5 % and NoteOff
for 2.5 % of the voices every block, rotating over the voices -- with a block's events spread over S distinct
times, S in {1, 2, 4, 16, 64}: event j of the block sits at frame (j mod S) * (256 / S).  Per kind (the Svf
voice and the Moog voice) and S, two legs over the same schedule:

  timed: the block's events through Engine.timed_events, one process call of 256 frames;
  split: per event time, that time's events through Engine.note_events and a process call up to the next time.

Device events around `--steps` blocks per region after `--warmup` blocks, the median of `--reps` regions; the
per-block event arrays are prebuilt, so a step is the library calls alone.  One JSON line.

`--tree DIR` imports ol_dsp_amd from DIR, a build of another commit; one without olfx_timed_events runs the split
leg only (`--legs split`): the baseline.

  python tools/voice_timed_ab.py [--kinds voice,voice_moog] [--segments 1,2,4,16,64] [--out profiles/voice_timed_ab.json]
  python tools/voice_timed_ab.py --tree ../parent --legs split
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def schedule(n, k, S, block):
    """Block k's events as (frames, inst, type, note), bench.py's voice_events rotation."""
    import numpy as np
    gi = np.arange(n)
    notes = 36 + (gi * 7) % 61
    on = np.nonzero(gi % 40 == k % 40)[0]
    off = np.nonzero(gi % 40 == (k + 20) % 40)[0]
    inst = np.concatenate([on, off])
    typ = np.concatenate([np.ones(len(on), np.uint8), np.zeros(len(off), np.uint8)])
    note = np.concatenate([(notes[on] + 12 * (k & 1)) % 128, notes[off]])
    frame = (np.arange(len(inst)) % S) * (block // S)
    return frame.astype(np.uint32), inst, typ, note


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kinds", default="voice,voice_moog")
    ap.add_argument("--segments", default="1,2,4,16,64")
    ap.add_argument("--legs", default="timed,split")
    ap.add_argument("--instances", type=int, default=32768)
    ap.add_argument("--block", type=int, default=256)
    ap.add_argument("--steps", type=int, default=80, help="blocks per timed region (a multiple of 40: whole rotations)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--tree", default=ROOT, help="the tree whose ol_dsp_amd (and libolfx.so) is measured")
    ap.add_argument("--out", default="", help="also write the JSON record here")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import numpy as np
    import torch

    import ol_dsp_amd as ofx
    from ol_dsp_amd import workload
    if not torch.cuda.is_available():
        sys.exit("voice_timed_ab: no GPU (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    n, B = args.instances, args.block
    legs = args.legs.split(",")
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
                for k in range(40):
                    frame, inst, typ, note = schedule(n, k, S, B)
                    if leg == "timed":
                        steps.append(e.make_timed_events(frame, inst, typ, note))
                    else:
                        cuts = sorted(set(frame.tolist())) + [B]
                        steps.append([(e.make_events(inst[frame == f0], typ[frame == f0], note[frame == f0]), out[:, f0:f1])
                                      for f0, f1 in zip(cuts, cuts[1:])])
                k = [0]

                def step():
                    st = steps[k[0] % 40]
                    k[0] += 1
                    if leg == "timed":
                        e.timed_events(st)
                        e.process(None, out=out)
                    else:
                        for evs, o in st:
                            e.note_events(evs)
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
                              "us_per_block": us, "events_per_block": int(len(steps[0]) if leg == "timed" else
                                                                          sum(len(a) for a, _ in steps[0])),
                              "finite": bool(torch.isfinite(out).all().item())})
                print(json.dumps(cells[-1]), file=sys.stderr, flush=True)
                del e
    res = {"instances": n, "block": B, "steps": args.steps, "reps": args.reps, "warmup": args.warmup,
           "lib": os.path.relpath(ofx.LIB_PATH, ROOT), "cells": cells}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
