#!/usr/bin/env python3
"""Control changes inside the block for the instrument kinds: one olfx_process with olfx_timed_instrument_control
against one olfx_process per control time.

tools/synth_timed_ab.py's shape -- 16,384 instruments x 256 frames, P = 4, every voice sounding -- for the synth, the
Svf synth and the drum kit, with CC 41 (the voice filter's cutoff; on a synth at topology 1 the rack filter's too; on a
kit the voice on channel i mod P) on 5 % of the instruments every block, rotating over the instruments in 20 blocks,
spread over S distinct times, S in {1, 2, 4, 16}: change j of the block sits at frame (j mod S) * (256 / S), so S = 1
is all at frame 0 (the unsegmented launch for either leg).  Per kind and S, two legs over the same schedule:

  timed: the block's changes through olfx_timed_instrument_control, one process call of 256 frames;
  split: per time, that time's changes through olfx_control and a process call up to the next time.

`--boundary` adds, at S = 2, the same instruments' change as a parameter record at frame 128 in two forms: "inside", a
field the kernel changes at its frame (rack FILTER_CUTOFF), and "boundary", a field that ends the launch there (rack
DELAY_FEEDBACK): the difference is the extra launch.

Device events around `--steps` blocks per region after `--warmup` blocks, the median (min - max) of `--reps` regions;
the per-block record arrays are prebuilt ctypes arrays, so a step is the library calls alone.  One JSON line.

`--parent DIR` also runs the split leg on DIR's ol_dsp_amd, a build of the parent commit, in a child process of the
same run: the baseline (a tree without the timed calls has no timed leg).

  python tools/synth_timed_params_ab.py [--kinds synth,synth_svf,drumkit] [--segments 1,2,4,16] [--boundary]
                                        [--parent ../parent] [--out profiles/synth_timed_params_ab.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CC_CUTOFF = 41


def schedule(n, P, k, S, block):
    """Block k's changes as (frames, inst, channel, values): every 20th instrument, rotating, the value stepping."""
    import numpy as np
    inst = np.nonzero(np.arange(n) % 20 == k % 20)[0]
    frame = (np.arange(len(inst)) % S) * (block // S)
    value = (30.0 + (inst + 7 * k) % 55).astype(np.float32)                   # MIDI 30 .. 84: 540 Hz .. 7.1 kHz
    return frame.astype(np.uint32), inst.astype(np.uint32), (inst % P).astype(np.uint16), value


def measure(args, tree, legs):
    sys.path.insert(0, os.path.abspath(tree))
    import numpy as np
    import torch

    import ol_dsp_amd as ofx
    from ol_dsp_amd import _lib, workload
    if not torch.cuda.is_available():
        sys.exit("synth_timed_params_ab: no GPU (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    n, P, B = args.instances, args.voices, args.block

    def controls(frame, inst, chan, value, kit, timed):
        arr = ((_lib.TimedControl if timed else _lib.ControlEvent) * len(inst))()
        for j in range(len(inst)):
            ev = arr[j].ev if timed else arr[j]
            if timed:
                arr[j].frame = int(frame[j])
            ev.inst, ev.control, ev.source, ev.value = int(inst[j]), CC_CUTOFF, _lib.CTL_MIDI, float(value[j])
            ev.pad = int(chan[j]) if kit else 0
        return arr

    def engine(kind):
        kit = kind == "drumkit"
        e = ofx.Engine(kind, n, block=B, voices=P)
        e.set_params(0, workload.instance_params(kind, 0, n))
        if kit:
            e.sample_bank(workload.sample_bank([48000] * 128, seed=1))
            e.sample_voices([(v, v % 128, 1) for v in range(n * P)])
            e.drumkit_map([(i, q, 36 + q, q) for i in range(n) for q in range(P)])
        for q in range(P):                                           # every voice sounds
            e.note_events(e.make_events(np.arange(n), 1, 36 + q if kit else 40 + 7 * q + np.arange(n) % 5))
        return e

    def timeit(step, last):
        def region():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.steps):
                step()
            t1.record()
            t1.synchronize()
            return t0.elapsed_time(t1) * 1e3 / args.steps               # us per block
        for _ in range(args.warmup):
            step()
        us = [region() for _ in range(args.reps)]
        return {"us_per_block_median": statistics.median(us), "us_per_block": us,
                "finite": bool(torch.isfinite(last()).all().item()), "nonzero": bool((last() != 0).any().item())}

    cells = []
    for kind in args.kinds.split(","):
        kit = kind == "drumkit"
        for S in (int(s) for s in args.segments.split(",")):
            assert B % S == 0 and (B // S) % 4 == 0
            for leg in legs:
                e = engine(kind)
                out = torch.empty((2, B, n), device=dev)
                steps = []
                for k in range(20):
                    frame, inst, chan, value = schedule(n, P, k, S, B)
                    if leg == "timed":
                        steps.append(controls(frame, inst, chan, value, kit, True))
                    else:
                        cuts = sorted(set(frame.tolist()) | {0}) + [B]
                        steps.append([(controls(frame[frame == f0], inst[frame == f0], chan[frame == f0], value[frame == f0], kit, False),
                                       torch.empty((2, f1 - f0, n), device=dev)) for f0, f1 in zip(cuts, cuts[1:])])
                k = [0]

                def step():
                    st = steps[k[0] % 20]
                    k[0] += 1
                    if leg == "timed":
                        assert e.lib.olfx_timed_instrument_control(e.handle, st, len(st)) == 0
                        e.process(None, out=out)
                    else:
                        for arr, o in st:
                            if len(arr):
                                assert e.lib.olfx_control(e.handle, arr, len(arr)) == 0
                            e.process(None, out=o)

                cell = {"kind": kind, "segments": S, "leg": leg, "changes_per_block": int(len(schedule(n, P, 0, S, B)[1]))}
                cell.update(timeit(step, lambda: out if leg == "timed" else steps[(k[0] - 1) % 20][-1][1]))
                cells.append(cell)
                print(json.dumps(cell), file=sys.stderr, flush=True)
                del e
        if args.boundary and "timed" in legs:
            names = ofx.engine.PARAMS[ofx.engine.KIND_NAMES[kind]]
            for leg, field in (("inside", "rack_filter_cutoff"), ("boundary", "rack_delay_feedback")):
                e = engine(kind)
                out = torch.empty((2, B, n), device=dev)
                steps = []
                for k in range(20):
                    _, inst, _, value = schedule(n, P, k, 1, B)
                    v = 500.0 + 10.0 * value if leg == "inside" else 0.2 + value / 400.0
                    steps.append(e.make_timed_params(B // 2, inst, names.index(field), v))
                k = [0]

                def step():
                    e.timed_instrument_params(steps[k[0] % 20])
                    k[0] += 1
                    e.process(None, out=out)

                cell = {"kind": kind, "segments": 2, "leg": leg, "field": field, "changes_per_block": int(len(steps[0]))}
                cell.update(timeit(step, lambda: out))
                cells.append(cell)
                print(json.dumps(cell), file=sys.stderr, flush=True)
                del e
    return {"lib": os.path.relpath(ofx.LIB_PATH, os.path.abspath(tree)), "device": torch.cuda.get_device_name(0),
            "cells": cells}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kinds", default="synth,synth_svf,drumkit")
    ap.add_argument("--segments", default="1,2,4,16")
    ap.add_argument("--instances", type=int, default=16384)
    ap.add_argument("--voices", type=int, default=4)
    ap.add_argument("--block", type=int, default=256)
    ap.add_argument("--steps", type=int, default=80, help="blocks per timed region (a multiple of 20: whole rotations)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--boundary", action="store_true", help="at S = 2: a record inside the launch against one that ends it")
    ap.add_argument("--parent", default="", help="a build of the parent commit: its split leg is the baseline")
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)      # the tree this child process measures
    ap.add_argument("--out", default="", help="also write the JSON record here")
    args = ap.parse_args()
    if args.child:                           # the baseline process: the split leg on another tree's library
        print(json.dumps(measure(args, args.child, ["split"])))
        return
    res = {"instances": args.instances, "voices": args.voices, "block": args.block, "steps": args.steps, "reps": args.reps,
           "warmup": args.warmup}
    res.update(measure(args, ROOT, ["timed", "split"]))
    if args.parent:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", args.parent] + \
              [f"--{k}={getattr(args, k)}" for k in ("kinds", "segments", "instances", "voices", "block", "steps", "reps", "warmup")]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        sys.stderr.write(r.stderr)
        if r.returncode != 0:
            sys.exit("synth_timed_params_ab: the parent's leg failed")
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
