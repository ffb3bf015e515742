#!/usr/bin/env python3
"""The sample-playback voice against the saw voice it shares three of its four roles with.

  sampler: one OLFX_KIND_VOICE_SAMPLE engine (sampler_block_v1) over a bank of `--samples` samples of
           one second each, voice i on sample i % samples, a quarter of the voices looping their whole
           sample, NoteOn staggered over the warm-up blocks so the cursors are spread over the bank;
  saw:     an OLFX_KIND_VOICE engine (voice_block_v5) of the same size and parameters, NoteOn at the
           first block.
Device events around `--steps` blocks per window, after the warm-up; `--reps` windows per path,
alternating the two paths in one process.  Prints one JSON line (medians, ranges, the ratio, and the
bank read rate the sampler sustains).

  python tools/sampler_ab.py [--instances 32768] [--block 256] [--steps 20] [--reps 7]
  python tools/sampler_ab.py --only sampler --steps 10      # untimed, for a rocprofv3 --pmc run
  OLFX_LIB=build/ab/libolfx_lane.so python tools/sampler_ab.py --tag per_lane   # a variant build
      (make -C ol_dsp_amd/csrc OUT=../../build/ab/libolfx_lane.so OBJDIR=../../build/ab/obj_lane
       EXTRA=-DOLFX_SAMPLER_PER_LANE: every voice on the per-frame gather)
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=32768)
    ap.add_argument("--block", type=int, default=256)
    ap.add_argument("--samples", type=int, default=128)
    ap.add_argument("--sample-frames", type=int, default=48000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=32)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--tag", default="", help="label of the library under test (OLFX_LIB variant builds)")
    ap.add_argument("--only", choices=["sampler", "saw"], help="run one path untimed (profiler runs)")
    args = ap.parse_args()

    import torch

    import ol_dsp_amd as ofx
    from ol_dsp_amd import workload
    if not torch.cuda.is_available():
        sys.exit("sampler_ab: no GPU (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    n, B = args.instances, args.block
    p = workload.instance_params("voice_sample", 0, n)
    out = torch.empty((1, B, n), device=dev)
    notes = workload.voice_notes(0, n)

    smp = ofx.Engine("voice_sample", n, block=B)
    smp.set_params(0, p)
    smp.sample_bank(workload.sample_bank([args.sample_frames] * args.samples, seed=1))
    # a quarter loops (the whole sample: a turn per second), the rest are one-shots retriggered below
    smp.sample_voices([(i, i % args.samples, 1 if i % 4 == 0 else 0) for i in range(n)])
    saw = ofx.Engine("voice", n, block=B)
    saw.set_params(0, p)
    saw.note_events(ofx.Engine.make_events(range(n), 1, notes))

    # triggers staggered over the warm-up blocks: voice i starts at block i % warmup, so the cursors
    # of a workgroup's 64 voices are spread over warmup x block frames of their samples
    def warm_sampler():
        for k in range(args.warmup):
            idx = range(k, n, args.warmup)
            smp.note_events(ofx.Engine.make_events(idx, 1, notes[k::args.warmup]))
            smp.process(None, out=out)

    def warm_saw():
        for _ in range(args.warmup):
            saw.process(None, out=out)

    paths = {"sampler": lambda: smp.process(None, out=out), "saw": lambda: saw.process(None, out=out)}
    if args.only:
        paths = {args.only: paths[args.only]}

    def window(run, steps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(steps):
            run()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) * 1e3 / steps           # us per block

    if "sampler" in paths:
        warm_sampler()
    if "saw" in paths:
        warm_saw()
    if args.only:
        window(paths[args.only], args.steps)
        print(json.dumps({"only": args.only, "instances": n, "block": B, "steps": args.steps}))
        return
    # the whole run stays inside the one-shots' second: warmup + reps x steps blocks of B frames
    played = (args.warmup + args.reps * args.steps) * B
    us = {name: [] for name in paths}
    for _ in range(args.reps):
        for name, run in paths.items():                     # alternating
            us[name].append(window(run, args.steps))
    res = {"instances": n, "block": B, "steps": args.steps, "reps": args.reps, "tag": args.tag,
           "lib": os.path.basename(ofx.LIB_PATH), "samples": args.samples, "sample_frames": args.sample_frames,
           "frames_played": played, "one_shots_still_playing": played < args.sample_frames,
           "kernels": {"sampler": smp.kernel_name, "saw": saw.kernel_name}}
    for name, v in us.items():
        res[name] = {"us_per_block_median": statistics.median(v), "us_per_block_min": min(v),
                     "us_per_block_max": max(v), "us_per_block": v}
    med = res["sampler"]["us_per_block_median"] * 1e-6
    res["sampler"]["bank_read_TBs"] = 4.0 * n * B / med / 1e12
    res["sampler"]["algorithmic_bytes_per_frame"] = smp.algorithmic_bytes_per_frame
    res["sampler_over_saw_median"] = res["sampler"]["us_per_block_median"] / res["saw"]["us_per_block_median"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
