#!/usr/bin/env python3
"""Cost of adaptive sampling on one box (HIP events, alternating order).

    tools/build_prev.sh <parent commit>        # build/libptgpu_prev.so: the baseline library
    python tools/adaptive_cost.py [--rounds 3] [--size 1920x1080] [--spp 1024] [--target 0.1]

Per workload (the bench frame: box; C5: synthetic:10000), every round runs two
fresh child processes in alternating order:
  base  PTGPU_LIB = the parent commit's library: the whole frame as ONE
        ptg_accumulate_device pass with PTG_FLAG_MOMENTS -- what (a) compares with;
  new   this tree's library:
        (a) one accumulate_active pass of the same samples with every pixel active;
        (b) the same pass with every 16th pixel active and with a random 10 % of
            the pixels active: time per sample relative to (a) shows whether
            sparse units fill the wave;
        (c) ptg_render_to_noise against ptg_render_adaptive at the CLI's defaults
            (min 16 samples per sub-pixel, at most 1 % of the pixels over, floor
            0.01, dilate 1) and --target: wall time (context creation and copies
            included), mean samples per sub-pixel, the fraction over at the end;
        (d) one select_active with dilate 0 and with dilate 1 (5 timings each).
Every timed pass follows one warm-up pass.  Prints one JSON line per
measurement and a summary line.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "cpu-path-tracing_amd")]
PREV = os.path.join(ROOT, "cpu-path-tracing_amd", "build", "libptgpu_prev.so")


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

    W, H = (int(v) for v in args.size.split("x"))
    samples = args.spp // 4
    scn = ptgpu.make_scene(args.scene, W, H)
    cam = ptgpu.camera.with_config(scn.camera_parameters)
    out = {"scene": args.scene, "variant": args.child, "lib": os.path.relpath(ptgpu.LIB_PATH, ROOT)}
    with ptgpu.Context(scn, cam, device=0) as ctx:
        if args.child == "base":
            p = ptgpu.make_params(W, H, samples, 2, ptgpu.DEFAULT_SEED, flags=ptgpu.FLAG_MOMENTS)
            for k in range(2):  # warm-up, then the timed pass
                ctx.reset_accumulation(p)
                out["moments_pass_ms"] = round(timed(lambda: ctx.accumulate(p, 0, samples)), 3)
        else:
            p = ptgpu.make_params(W, H, samples, 2, ptgpu.DEFAULT_SEED)
            every16 = np.zeros(H * W, dtype=np.uint8)
            every16[::16] = 1
            rand10 = (np.random.default_rng(1).random(H * W) < 0.10).astype(np.uint8)
            info = torch.zeros(2, dtype=torch.int64, device="cuda:0")
            for key, mask in (("all", None), ("every16", every16), ("random10", rand10)):
                m = torch.from_numpy(mask).cuda() if mask is not None else None
                for k in range(2):
                    ctx.reset_accumulation(p)
                    ctx.set_active_mask(p, m, info)
                    pixels, units = (int(v) for v in info.cpu().tolist())
                    ms = timed(lambda: ctx.accumulate_active(p, samples, units))
                out[key] = {"pass_ms": round(ms, 3), "pixels": pixels, "units": units,
                            "ns_per_sample": round(ms * 1e6 / (pixels * 4.0 * samples), 4)}
            # (d) on a frame with unequal counts: every pixel 16 samples, the random 10 % another 16
            ctx.reset_accumulation(p)
            ctx.set_active_mask(p)
            ctx.accumulate_active(p, 16)
            ctx.set_active_mask(p, torch.from_numpy(rand10).cuda())
            ctx.accumulate_active(p, 16)
            stats = torch.zeros(6, dtype=torch.int64, device="cuda:0")
            for d in (0, 1):
                ctx.select_active(p, args.target, 0.01, d, stats=stats)
                t = [timed(lambda: ctx.select_active(p, args.target, 0.01, d, stats=stats)) for _ in range(5)]
                out[f"select_dilate{d}_ms"] = {"min": round(min(t), 4), "max": round(max(t), 4)}
    if args.child == "new":  # (c), in the order the round asks for
        def to_noise():
            img = np.zeros((H * W, 3))
            t0 = time.perf_counter()
            r = ptgpu.render_to_noise(scn, cam, img, W, H, samples, args.target, 0.01, 0.01, 16)
            return {"wall_ms": round((time.perf_counter() - t0) * 1e3, 2), "mean_samples": r["samples_done"],
                    "passes": r["passes"], "over_fraction": round(r["pixels_over"] / r["pixels"], 5),
                    "converged": r["converged"]}

        def adaptive():
            img = np.zeros((H * W, 3))
            t0 = time.perf_counter()
            r = ptgpu.render_adaptive(scn, cam, img, W, H, samples, args.target, 0.01, 0.01, 16, 1)
            return {"wall_ms": round((time.perf_counter() - t0) * 1e3, 2), "mean_samples": round(r["mean_samples"], 3),
                    "passes": r["passes"], "over_fraction": round(r["pixels_over"] / r["pixels"], 5),
                    "converged": r["converged"], "pass_active": r["pass_active"]}

        to_noise()  # warm-up (code objects, allocator)
        order = [("to_noise", to_noise), ("adaptive", adaptive)]
        for name, fn in (order if args.round % 2 == 0 else order[::-1]):
            out[name] = fn()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--spp", type=int, default=1024)
    ap.add_argument("--target", type=float, default=0.1)
    ap.add_argument("--scenes", default="box,synthetic:10000")
    ap.add_argument("--child", choices=["base", "new"])
    ap.add_argument("--scene")
    ap.add_argument("--round", type=int, default=0)
    args = ap.parse_args()
    if args.child:
        return child(args)
    if not os.path.exists(PREV):
        sys.exit(f"{PREV} missing: run tools/build_prev.sh <parent commit> first")
    recs = []
    for name in args.scenes.split(","):
        for r in range(args.rounds):
            for v in (("base", "new") if r % 2 == 0 else ("new", "base")):
                env = dict(os.environ)
                if v == "base":
                    env["PTGPU_LIB"] = PREV
                else:
                    env.pop("PTGPU_LIB", None)
                cmd = [sys.executable, os.path.abspath(__file__), "--child", v, "--scene", name, "--round", str(r),
                       "--size", args.size, "--spp", str(args.spp), "--target", str(args.target)]
                res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
                if res.returncode != 0:  # nothing more is started after a failure
                    sys.exit(f"{v} child of {name} failed ({res.returncode}):\n{res.stderr[-3000:]}")
                rec = json.loads(res.stdout.strip().splitlines()[-1])
                rec["round"] = r + 1
                recs.append(rec)
                print(json.dumps(rec), flush=True)
    summary = {}
    for name in args.scenes.split(","):
        base = [r["moments_pass_ms"] for r in recs if r["scene"] == name and r["variant"] == "base"]
        new = [r for r in recs if r["scene"] == name and r["variant"] == "new"]
        mean = lambda t: sum(t) / len(t)  # noqa: E731
        s = {"base_moments_pass_ms": {"min": min(base), "max": max(base), "mean": round(mean(base), 3)}}
        for key in ("all", "every16", "random10"):
            t = [r[key]["pass_ms"] for r in new]
            s[key] = {"min": min(t), "max": max(t), "mean": round(mean(t), 3), "pixels": new[0][key]["pixels"],
                      "units": new[0][key]["units"],
                      "ns_per_sample_mean": round(mean([r[key]["ns_per_sample"] for r in new]), 4)}
        s["all_active_over_base_pct"] = round(100.0 * (s["all"]["mean"] / s["base_moments_pass_ms"]["mean"] - 1.0), 2)
        for key in ("every16", "random10"):
            s[key]["time_per_sample_vs_all"] = round(s[key]["ns_per_sample_mean"] / s["all"]["ns_per_sample_mean"], 3)
        for d in (0, 1):
            s[f"select_dilate{d}_ms_min"] = min(r[f"select_dilate{d}_ms"]["min"] for r in new)
        for key in ("to_noise", "adaptive"):
            s[key] = dict(new[-1][key], wall_ms=[r[key]["wall_ms"] for r in new])
        summary[f"{name} {args.size} {args.spp}spp target {args.target}"] = s
    print(json.dumps({"rounds": args.rounds, "summary": summary}))


if __name__ == "__main__":
    main()
