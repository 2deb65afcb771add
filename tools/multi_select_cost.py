#!/usr/bin/env python3
"""Cost of one selection through the gathered list against the existing one
(HIP events, fresh processes, alternating order; tools/adaptive_cost.py's (d)).

    python tools/multi_select_cost.py [--rounds 3] [--size 1920x1080] [--target 0.1]

The frame of adaptive_cost.py's (d): box, every pixel 16 samples, a random
10 % another 16.  Per dilate (1 and 8), with shard_count 1, each timed 5 times
after a warm-up call:
  old   ptg_select_active_device           select_over_kernel + list_rows_kernel + units + fill
  new   ptg_select_over_device, then       select_over_kernel
        ptg_set_active_gathered_device     list_rows_gathered_kernel + units + fill
        (timed together, and each alone)
Every round is a fresh child process; odd rounds time new before old.  Both
lists must hold the same pixels and units.  Prints one JSON line per round and
a summary line (the minimum over the rounds of each round's minimum).
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "cpu-path-tracing_amd")]
DILATES = (1, 8)


def child(args):
    import numpy as np
    import torch

    import ptgpu

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def best(fn):
        fn()  # warm-up
        t = [timed(fn) for _ in range(5)]
        return {"min": round(min(t), 4), "max": round(max(t), 4)}

    W, H = (int(v) for v in args.size.split("x"))
    scn = ptgpu.make_scene("box", W, H)
    cam = ptgpu.camera.with_config(scn.camera_parameters)
    p = ptgpu.make_params(W, H, 256, 2, ptgpu.DEFAULT_SEED)
    rand10 = (np.random.default_rng(1).random(H * W) < 0.10).astype(np.uint8)
    out = {"round": args.round, "size": args.size, "target": args.target}
    with ptgpu.Context(scn, cam, device=0) as ctx:
        ctx.reset_accumulation(p)
        ctx.set_active_mask(p)
        ctx.accumulate_active(p, 16)
        ctx.set_active_mask(p, torch.from_numpy(rand10).cuda())
        ctx.accumulate_active(p, 16)
        over = torch.zeros(H * W, dtype=torch.uint8, device="cuda:0")
        so, sn = (torch.zeros(6, dtype=torch.int64, device="cuda:0") for _ in range(2))

        def old(d):
            return lambda: ctx.select_active(p, args.target, 0.01, d, stats=so)

        def new(d):
            def both():
                ctx.select_over(p, args.target, 0.01, over, stats=sn)
                ctx.set_active_gathered(p, over, d, stats=sn)
            return both
        for d in DILATES:
            order = [("old", old(d)), ("new", new(d))]
            for name, fn in (order if args.round % 2 == 0 else order[::-1]):
                out[f"{name}_dilate{d}_ms"] = best(fn)
            out[f"new_list_dilate{d}_ms"] = best(lambda: ctx.set_active_gathered(p, over, d, stats=sn))
            so.zero_()
            sn.zero_()
            old(d)()
            new(d)()
            torch.cuda.synchronize()
            a, b = so.cpu().tolist(), sn.cpu().tolist()
            if a != b:
                sys.exit(f"dilate {d}: the two selections differ: {a} vs {b}")
            out[f"dilate{d}_over_active_units"] = [a[0], a[4], a[5]]
        out["select_over_ms"] = best(lambda: ctx.select_over(p, args.target, 0.01, over, stats=sn))
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--target", type=float, default=0.1)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--round", type=int, default=0)
    args = ap.parse_args()
    if args.child:
        return child(args)
    recs = []
    for r in range(args.rounds):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--round", str(r), "--size", args.size,
               "--target", str(args.target)]
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        if res.returncode != 0:  # nothing more is started after a failure
            sys.exit(f"round {r} failed ({res.returncode}):\n{res.stderr[-3000:]}")
        recs.append(json.loads(res.stdout.strip().splitlines()[-1]))
        print(json.dumps(recs[-1]), flush=True)
    keys = [k for k in recs[0] if k.endswith("_ms")]
    print(json.dumps({"rounds": args.rounds, "summary_min_ms": {k: min(r[k]["min"] for r in recs) for k in keys}}))


if __name__ == "__main__":
    main()
