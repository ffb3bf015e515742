#!/usr/bin/env python3
"""Notes inside the block for the instrument kinds: one olfx_process with olfx_timed_notes against one olfx_process
per event time.

tools/synth_ab.py's shape -- 16,384 instruments x 256 frames, P = 4 -- for the synth, the Svf synth and the drum
kit, with bench.py's `voice_events` note density: every block 2.5 % of the instruments get a NoteOn and 2.5 % a
NoteOff, rotating over the instruments in 40 blocks.  Voices 0 .. P - 2 of every instrument hold a note throughout;
the rotating notes take and release the last voice (a kit: pad i mod P of kit i is retriggered and released; every
pad loops its one-second sample, so all voices keep reading the bank).  A block's notes are spread over S distinct
times, S in {1, 2, 4, 16}: note j of the block sits at frame (j mod S) * (256 / S).  Per kind and S, over the same
schedule:

  timed: the block's notes through Engine.timed_notes, one process call of 256 frames;
  split: per event time, that time's notes through Engine.note_events and a process call up to the next time.

Device events around `--steps` blocks per region after `--warmup` blocks, the median of `--reps` regions; the
per-block note arrays are prebuilt, so a step is the library calls alone.  One JSON line.

`--parent DIR` also runs the split leg on the build in DIR (a checkout of the parent commit, built), in a process of
its own in the same run: the baseline, under "parent".  `--tree DIR --legs split` is that run by hand.

  python tools/synth_timed_ab.py [--kinds synth,synth_svf,drumkit] [--segments 1,2,4,16] [--parent ../parent]
                                 [--out profiles/synth_timed_ab.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def schedule(n, P, k, S, block, kit):
    """Block k's notes as (frames, inst, type, note), bench.py's voice_events rotation over the instruments."""
    import numpy as np
    gi = np.arange(n)
    notes = 36 + gi % P if kit else 72 + (gi * 7) % 40
    on = np.nonzero(gi % 40 == k % 40)[0]
    off = np.nonzero(gi % 40 == (k + 20) % 40)[0]
    inst = np.concatenate([on, off])
    typ = np.concatenate([np.ones(len(on), np.uint8), np.zeros(len(off), np.uint8)])
    note = np.concatenate([notes[on], notes[off]])
    frame = (np.arange(len(inst)) % S) * (block // S)
    return frame.astype(np.uint32), inst, typ, note


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kinds", default="synth,synth_svf,drumkit")
    ap.add_argument("--segments", default="1,2,4,16")
    ap.add_argument("--legs", default="timed,split")
    ap.add_argument("--instances", type=int, default=16384)
    ap.add_argument("--voices", type=int, default=4)
    ap.add_argument("--block", type=int, default=256)
    ap.add_argument("--steps", type=int, default=80, help="blocks per timed region (a multiple of 40: whole rotations)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--tree", default=ROOT, help="the tree whose ol_dsp_amd (and libolfx.so) is measured")
    ap.add_argument("--parent", default="", help="a built checkout of the parent commit: its split leg, as the baseline")
    ap.add_argument("--out", default="", help="also write the JSON record here")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import numpy as np
    import torch

    import ol_dsp_amd as ofx
    from ol_dsp_amd import workload
    if not torch.cuda.is_available():
        sys.exit("synth_timed_ab: no GPU (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    n, P, B = args.instances, args.voices, args.block
    legs = args.legs.split(",")
    cells = []
    for kind in args.kinds.split(","):
        kit = kind == "drumkit"
        for S in (int(s) for s in args.segments.split(",")):
            assert B % S == 0 and (B // S) % 4 == 0
            for leg in legs:
                e = ofx.Engine(kind, n, block=B, voices=P)
                e.set_params(0, workload.instance_params(kind, 0, n))
                if kit:
                    e.sample_bank(workload.sample_bank([48000] * 128, seed=1))
                    e.sample_voices([(v, v % 128, 1) for v in range(n * P)])
                    e.drumkit_map([(i, q, 36 + q, q) for i in range(n) for q in range(P)])
                    held = range(P)
                else:
                    held = range(P - 1)
                for q in held:                                   # the notes that stay
                    e.note_events(e.make_events(np.arange(n), 1, 36 + q if kit else 40 + 7 * q + np.arange(n) % 5))
                out = torch.empty((2, B, n), device=dev)
                steps = []
                for k in range(40):
                    frame, inst, typ, note = schedule(n, P, k, S, B, kit)
                    if leg == "timed":
                        steps.append(e.make_timed_notes(frame, inst, typ, note))
                    else:
                        cuts = sorted(set(frame.tolist()) | {0}) + [B]
                        steps.append([(e.make_events(inst[frame == f0], typ[frame == f0], note[frame == f0]),
                                       torch.empty((2, f1 - f0, n), device=dev)) for f0, f1 in zip(cuts, cuts[1:])])
                k = [0]

                def step():
                    st = steps[k[0] % 40]
                    k[0] += 1
                    if leg == "timed":
                        e.timed_notes(st)
                        e.process(None, out=out)
                    else:
                        for evs, o in st:
                            if len(evs):
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
                last = out if leg == "timed" else steps[(k[0] - 1) % 40][-1][1]
                cells.append({"kind": kind, "segments": S, "leg": leg, "us_per_block_median": statistics.median(us),
                              "us_per_block": us, "notes_per_block": int(len(steps[0]) if leg == "timed" else
                                                                         sum(len(a) for a, _ in steps[0])),
                              "playing_0": e.playing(0), "finite": bool(torch.isfinite(last).all().item()),
                              "nonzero": bool((last != 0).any().item())})
                print(json.dumps(cells[-1]), file=sys.stderr, flush=True)
                del e
    res = {"instances": n, "voices": P, "block": B, "steps": args.steps, "reps": args.reps, "warmup": args.warmup,
           "device": torch.cuda.get_device_name(0), "lib": os.path.relpath(ofx.LIB_PATH, ROOT), "cells": cells}
    if args.parent:
        torch.cuda.synchronize()
        cmd = [sys.executable, os.path.abspath(__file__), "--tree", args.parent, "--legs", "split", "--kinds", args.kinds,
               "--segments", args.segments, "--instances", str(n), "--voices", str(P), "--block", str(B),
               "--steps", str(args.steps), "--reps", str(args.reps), "--warmup", str(args.warmup)]
        r = subprocess.run(cmd, capture_output=True, text=True, check=True)
        sys.stderr.write(r.stderr)
        res = {"this_change": res, "parent": json.loads(r.stdout.strip().splitlines()[-1])}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
