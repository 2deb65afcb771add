#!/usr/bin/env python3
"""Cost of PTG_FLAG_MOMENTS and of one ptg_noise_device check, same box.

    python tools/moments_overhead.py [--rounds 3] [--size 1920x1080] [--spp 1024]
    PTGPU_LIB=cpu-path-tracing_amd/build/libptgpu_prev.so python tools/moments_overhead.py --plain-only

Per workload (the bench frame: box; C5: synthetic:10000) the whole frame as
ONE progressive pass (ptg_accumulate_device over [0, samples)), timed with HIP
events after one warm-up pass: without the flag, with it, in alternating
order over the rounds.  Then ptg_noise_device (stats only, and with both
slabs) on the accumulated frame.  --plain-only times the unflagged pass alone:
with PTGPU_LIB naming a build of the parent commit (tools/build_prev.sh) it
shows that the unflagged pass did not move.  Prints one JSON line per
measurement and a summary.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "cpu-path-tracing_amd")]

import torch  # noqa: E402

import ptgpu  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--spp", type=int, default=1024)
    ap.add_argument("--scenes", default="box,synthetic:10000")
    ap.add_argument("--plain-only", action="store_true")
    args = ap.parse_args()
    W, H = (int(v) for v in args.size.split("x"))
    samples = args.spp // 4
    flag = getattr(ptgpu, "FLAG_MOMENTS", 0)
    variants = [("plain", 0)] if args.plain_only or not flag else [("plain", 0), ("moments", flag)]
    summary = {}
    for name in args.scenes.split(","):
        scn = ptgpu.make_scene(name, W, H)
        cam = ptgpu.camera.with_config(scn.camera_parameters)
        ms = {v: [] for v, _ in variants}
        with ptgpu.Context(scn, cam, device=0) as ctx:
            params = {v: ptgpu.make_params(W, H, samples, 2, ptgpu.DEFAULT_SEED, flags=f) for v, f in variants}

            def one_pass(v):
                ctx.reset_accumulation(params[v])
                return timed(lambda: ctx.accumulate(params[v], 0, samples))

            for v, _ in variants:
                one_pass(v)  # warm-up (and the accumulators' allocation)
            for r in range(args.rounds):
                for v, _ in (variants if r % 2 == 0 else variants[::-1]):
                    ms[v].append(one_pass(v))
                    print(json.dumps({"scene": name, "round": r + 1, "variant": v, "pass_ms": round(ms[v][-1], 3)}))
            rec = {v: {"min": round(min(t), 3), "max": round(max(t), 3), "mean": round(sum(t) / len(t), 3)}
                   for v, t in ms.items()}
            if "moments" in ms:
                rec["moments_over_plain_pct"] = round(100.0 * (rec["moments"]["mean"] / rec["plain"]["mean"] - 1.0), 2)
                # the frame's last pass was flagged or not, by the round order: make it a flagged one
                one_pass("moments")
                p = params["moments"]
                stats = torch.zeros(4, dtype=torch.int64, device="cuda:0")
                var = torch.zeros(H * W * 3, dtype=torch.float32, device="cuda:0")
                rho = torch.zeros(H * W, dtype=torch.float32, device="cuda:0")
                ctx.noise(p, samples, 0.05, 0.01, stats=stats)  # warm-up
                chk = [timed(lambda: ctx.noise(p, samples, 0.05, 0.01, stats=stats)) for _ in range(5)]
                full = [timed(lambda: ctx.noise(p, samples, 0.05, 0.01, var, rho, stats)) for _ in range(5)]
                rec["noise_check_ms"] = {"stats_only_min": round(min(chk), 4), "stats_only_max": round(max(chk), 4),
                                         "with_slabs_min": round(min(full), 4), "with_slabs_max": round(max(full), 4)}
        summary[f"{name} {W}x{H} {args.spp}spp"] = rec
    print(json.dumps({"lib": os.path.relpath(ptgpu.LIB_PATH, ROOT), "rounds": args.rounds, "summary": summary}))


if __name__ == "__main__":
    main()
