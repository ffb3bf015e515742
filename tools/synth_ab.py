#!/usr/bin/env python3
"""The synth's fused kernel against the three launches it replaces.

  fused:    one OLFX_KIND_SYNTH engine (synth_block_v1), one launch per block;
  composed: an OLFX_KIND_VOICE_MOOG engine of instances x voices voices (voice_block_v4), olfx_mix into
            one bus per instrument (voice_mix), an OLFX_KIND_FXRACK engine at topology 1
            (fxrack_block_v3): three launches per block, every voice sample and every bus sample
            through HBM (8 voices + 8 B per instrument-frame).
Both get the same per-instrument parameters (workload.RANGES["synth"]) and every voice a NoteOn before
the first block.  --kind synth_svf times the Svf synth instead: synth_svf_block_v1 against
voice_block_v5 (OLFX_KIND_VOICE) + voice_mix + fxrack_block_v3, with workload.RANGES["synth_svf"] and every
instrument's rack at --topology (0 or 1; the composed rack engine gets the same).  Device events around `--steps` blocks per window; at least 50 warm-up launches of
each path; `--reps` windows per path, the order of the two paths rotated from one repetition to the
next, in one process.  Prints one JSON line (medians, min-max, the verdict by the rule below, and
whether the two paths' last blocks -- the same block of the same stream -- agree bit for bit).

The verdict: "faster" only if the fused median lies below the composed median by more than the
larger of the two min-max spreads; "slower" by the same rule the other way; else "tie".

--kind drumkit times the drum kit: drumkit_block_v1 against sampler_block_v1 (OLFX_KIND_VOICE_SAMPLE, voice
i * P + q = voice q of kit i with that slot's own parameters) + voice_mix + fxrack_block_v3 at --topology, with
workload.RANGES["drumkit"], a bank of 128 one-second samples (voice v on sample v % 128, a quarter of the voices
looping their whole sample) and voice q of every kit at note 36 + q (the sum order is the slot order: the mix's
contiguous buses).  One-shots last a second, so both paths retrigger before every window, untimed and staggered over
eight blocks (the kits with i % 8 = k at block k): the cursors of a workgroup's voices stay spread over the bank.
OLFX_LIB=... --tag per_lane times a variant build (EXTRA=-DOLFX_DRUMKIT_PER_LANE: lane = voice gathers only).

  python tools/synth_ab.py [--instances 16384] [--voices 4] [--block 256] [--steps 50] [--reps 7]
  python tools/synth_ab.py --kind synth_svf --topology 0 [--voices 1|4|8]
  python tools/synth_ab.py --kind drumkit [--voices 1|4|8] [--topology 0|1] [--tag per_lane]
  python tools/synth_ab.py --only fused --steps 10      # untimed, for a rocprofv3 --pmc run
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
    ap.add_argument("--instances", type=int, default=16384)
    ap.add_argument("--voices", type=int, default=4)
    ap.add_argument("--block", type=int, default=256)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--kind", choices=["synth", "synth_svf", "drumkit"], default="synth")
    ap.add_argument("--tag", default="", help="label of the library under test (OLFX_LIB variant builds)")
    ap.add_argument("--topology", type=int, choices=[0, 1], default=1, help="synth_svf: every instrument's rack topology")
    ap.add_argument("--only", choices=["fused", "composed"], help="run one path untimed (profiler runs)")
    args = ap.parse_args()

    import numpy as np
    import torch

    import ol_dsp_amd as ofx
    from ol_dsp_amd import workload
    if not torch.cuda.is_available():
        sys.exit("synth_ab: no GPU (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    n, P, B = args.instances, args.voices, args.block
    svf = args.kind == "synth_svf"
    kit = args.kind == "drumkit"
    if args.topology != 1 and not (svf or kit):
        sys.exit("synth_ab: the Moog synth runs topology 1 only")
    p = workload.instance_params(args.kind, 0, n)
    nv = len(ofx.PARAMS[ofx.KIND_VOICE])
    rack0 = 8 * nv if kit else nv                            # the rack's fields follow the voices'
    p[rack0 + ofx.PARAMS[ofx.KIND_FXRACK].index("topology")] = float(args.topology)
    notes = workload.voice_notes(0, n * P).reshape(n, P)
    out = torch.empty((2, B, n), device=dev)
    out_c = torch.empty((2, B, n), device=dev)

    paths, retrigger = {}, {}
    stagger = 8
    if kit:
        bank = workload.sample_bank([48000] * 128, seed=1)
        voices_of = np.arange(n * P)                         # voice v = kit v // P, slot v % P, in both paths
        recs = [(int(v), int(v) % 128, 1 if v % 4 == 0 else 0) for v in voices_of]
        kits_of = [np.arange(k, n, stagger) for k in range(stagger)]
    if kit and args.only != "composed":
        fused = ofx.Engine("drumkit", n, block=B, voices=P)
        fused.set_params(0, p)
        fused.sample_bank(bank)
        fused.sample_voices(recs)
        fused.drumkit_map([(i, q, 36 + q, q) for i in range(n) for q in range(P)])
        ev_f = [np.concatenate([ofx.Engine.make_events(kits, 1, 36 + q) for q in range(P)]) for kits in kits_of]

        def retrigger_fused():
            for k in range(stagger):
                fused.note_events(ev_f[k])
                fused.process(None, out=out)
        paths["fused"], retrigger["fused"] = (lambda k: fused.process(None, out=out)), retrigger_fused
    if kit and args.only != "fused":
        voice, rack = ofx.Engine("voice_sample", n * P, block=B), ofx.Engine("fxrack", n, block=B)
        voice.set_params(0, np.ascontiguousarray(p[:8 * nv].reshape(8, nv, n)[:P].transpose(1, 2, 0)).reshape(nv, n * P))
        rack.set_params(0, p[rack0:])
        voice.sample_bank(bank)
        voice.sample_voices(recs)
        voice.mix_config([[i * P + q for q in range(P)] for i in range(n)])
        ev_c = [ofx.Engine.make_events((kits[:, None] * P + np.arange(P)[None, :]).T.reshape(-1), 1,
                                       np.repeat(36 + np.arange(P), len(kits))) for kits in kits_of]
        vo = torch.empty((1, B, n * P), device=dev)
        x = torch.zeros((2, B, n), device=dev)

        def composed_kit(k):
            voice.process(None, out=vo)
            x[0].zero_()                                     # the caller zeroes its frame (VoiceMap.h:64-73)
            voice.mix(vo, x[0])
            rack.process(x, out=out_c)

        def retrigger_composed():
            for k in range(stagger):
                voice.note_events(ev_c[k])
                composed_kit(k)
        paths["composed"], retrigger["composed"] = composed_kit, retrigger_composed
    if not kit and args.only != "composed":
        fused = ofx.Engine(args.kind, n, block=B, voices=P)
        fused.set_params(0, p)
        for q in range(P):                                   # voice q of every instrument
            fused.note_events(ofx.Engine.make_events(np.arange(n), 1, notes[:, q]))
        paths["fused"] = lambda k: fused.process(None, out=out)
    if not kit and args.only != "fused":
        voice, rack = ofx.Engine("voice" if svf else "voice_moog", n * P, block=B), ofx.Engine("fxrack", n, block=B)
        # voice i * P + q is voice q of instrument i: contiguous buses, the mix's fastest path (float4 runs)
        voice.set_params(0, np.repeat(p[:nv], P, axis=1))
        rack.set_params(0, p[nv:])
        voice.mix_config([[i * P + q for q in range(P)] for i in range(n)])
        voice.note_events(ofx.Engine.make_events(np.arange(n * P), 1, notes.reshape(-1)))
        vo = torch.empty((1, B, n * P), device=dev)
        x = torch.zeros((2, B, n), device=dev)

        def composed(k):
            voice.process(None, out=vo)
            x[0].zero_()                                     # the caller zeroes its frame (Polyvoice.h:28-33)
            voice.mix(vo, x[0])
            rack.process(x, out=out_c)
        paths["composed"] = composed

    def window(run, steps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for k in range(steps):
            run(k)
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) * 1e3 / steps           # us per block

    for name, run in paths.items():
        if name in retrigger:
            retrigger[name]()
        window(run, max(args.warmup, 50 if not args.only else 2))
    if args.only:
        if args.only in retrigger:
            retrigger[args.only]()
        window(paths[args.only], args.steps)
        print(json.dumps({"only": args.only, "kind": args.kind, "topology": args.topology, "instances": n, "voices": P, "block": B, "steps": args.steps}))
        return
    names = list(paths)
    us = {name: [] for name in names}
    for r in range(args.reps):
        for name in names[r % 2:] + names[:r % 2]:          # rotated
            if name in retrigger:                           # (untimed)
                retrigger[name]()
            us[name].append(window(paths[name], args.steps))
    res = {"kind": args.kind, "topology": args.topology, "instances": n, "voices": P, "block": B, "steps": args.steps, "reps": args.reps, "warmup": max(args.warmup, 50),
           "kernels": {"fused": fused.kernel_name, "composed": [voice.kernel_name, "voice_mix", rack.kernel_name]},
           "device": torch.cuda.get_device_name(0), "tag": args.tag, "lib": os.path.basename(ofx.LIB_PATH)}
    for name, v in us.items():
        res[name] = {"us_per_block_median": statistics.median(v), "us_per_block_min": min(v),
                     "us_per_block_max": max(v), "us_per_block": v}
    mf, mc = res["fused"]["us_per_block_median"], res["composed"]["us_per_block_median"]
    spread = max(res[k]["us_per_block_max"] - res[k]["us_per_block_min"] for k in names)
    res["larger_spread_us"] = spread
    res["fused_over_composed_median"] = mf / mc
    res["verdict"] = "faster" if mc - mf > spread else ("slower" if mf - mc > spread else "tie")
    res["fused"]["instrument_frames_per_s"] = n * B / (mf * 1e-6)
    res["hbm_bytes_per_instrument_frame_removed"] = 8 * P + 8
    if kit:
        res["fused"]["algorithmic_bytes_per_frame"] = fused.algorithmic_bytes_per_frame
        res["fused"]["bank_read_TBs"] = 4.0 * n * P * B / (mf * 1e-6) / 1e12
    # both paths have run the same number of blocks from the same start: their last blocks must agree
    # bit for bit at the timed size too
    torch.cuda.synchronize()
    res["last_block_bit_identical"] = bool(torch.equal(out.view(torch.int32), out_c.view(torch.int32)))
    res["last_block_nonzero_finite"] = bool(torch.isfinite(out).all() and (out != 0).any())
    # (the Svf voice's drive term can run a voice of the workload's draw away to a non-finite level)
    res["last_block_nonfinite_instruments"] = int((~torch.isfinite(out)).any(dim=0).any(dim=0).sum())
    res["last_block_silent_instruments"] = int((out[0] == 0).all(dim=0).sum())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
