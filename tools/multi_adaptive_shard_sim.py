#!/usr/bin/env python3
"""Single-GPU estimate of the balance of an adaptive frame over N GPUs
(tools/shard_sim.py's method for ptg_multi_render_adaptive).

    python tools/multi_adaptive_shard_sim.py [--counts 2 4 8] [--target 0.05] [--spp 256]

One context per shard on ONE device runs ptg_multi_render_adaptive's schedule
through the per-context entry points (select_over, the concatenation an
all-gather would produce, set_active_gathered): the decisions are the N-GPU
frame's.  Each shard's pass (accumulate_active) and selection (select_over +
set_active_gathered) is timed alone with HIP events, one shard after another.
On N GPUs a pass takes as long as its slowest shard, so the efficiency of a
pass is sum_k T_k / (N max_k T_k), and the frame's sum over the passes of
sum_k T_k / (N sum over the passes of max_k T_k).  The all-gather and the
host synchronisation per pass are not included: SIMULATED on one device.
Prints one JSON line per (N, pass) and one per N.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cpu-path-tracing_amd"))

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
    ap.add_argument("--counts", type=int, nargs="+", default=[2, 4, 8])
    ap.add_argument("--scene", default="box")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--min-spp", type=int, default=64)
    ap.add_argument("--target", type=float, default=0.05)
    ap.add_argument("--floor", type=float, default=0.01)
    ap.add_argument("--fraction", type=float, default=0.01)
    ap.add_argument("--dilate", type=int, default=1)
    ap.add_argument("--band-rows", type=int, default=ptgpu.DEFAULT_BAND_ROWS)
    args = ap.parse_args()
    W, H = args.width, args.height
    ends = ptgpu.noise_schedule(args.min_spp // 4, args.spp // 4)
    scn = ptgpu.make_scene(args.scene, W, H)
    cam = ptgpu.camera.with_config(scn.camera_parameters)
    with ptgpu.Context(scn, cam, device=0) as c:  # warm-up: code objects, allocator
        p = ptgpu.make_params(W, H, 4, 2, ptgpu.DEFAULT_SEED)
        o = torch.zeros(H * W, dtype=torch.uint8, device="cuda:0")
        c.reset_accumulation(p)
        c.set_active_mask(p)
        c.accumulate_active(p, 4)
        c.select_over(p, args.target, args.floor, o)
        c.set_active_gathered(p, o, args.dilate)
        torch.cuda.synchronize()
    frame = f"{args.scene} {W}x{H} at most {args.spp}spp, target {args.target}, dilate {args.dilate}"
    for n in args.counts:
        ps = [ptgpu.make_params(W, H, ends[-1], 2, ptgpu.DEFAULT_SEED, args.band_rows, k, n) for k in range(n)]
        rows = ptgpu.shard_rows(H, args.band_rows, n)
        ctxs = [ptgpu.Context(scn, cam, device=0) for _ in range(n)]
        try:
            over = torch.zeros((n, rows * W), dtype=torch.uint8, device="cuda:0")
            stats = torch.zeros((n, 6), dtype=torch.int64, device="cuda:0")
            for c, p in zip(ctxs, ps):
                c.reset_accumulation(p)
                c.set_active_mask(p)
            units = [0] * n
            active = [int((ptgpu.slab_to_image_rows(H, args.band_rows, k, n) >= 0).sum()) * W for k in range(n)]
            done, sum_all, sum_max = 0, 0.0, 0.0
            for k, e in enumerate(ends):
                stats.zero_()
                t_pass = [timed(lambda: c.accumulate_active(p, e - done, u)) for c, p, u in zip(ctxs, ps, units)]
                done = e
                t_over = [timed(lambda: c.select_over(p, args.target, args.floor, over[i], stats=stats[i]))
                          for i, (c, p) in enumerate(zip(ctxs, ps))]
                gathered = over.reshape(-1)
                t_list = [timed(lambda: c.set_active_gathered(p, gathered, args.dilate, stats[i]))
                          for i, (c, p) in enumerate(zip(ctxs, ps))]
                st = stats.cpu().numpy()
                t = [a + b + c for a, b, c in zip(t_pass, t_over, t_list)]
                sum_all += sum(t)
                sum_max += max(t)
                n_over = int(st[:, 0].sum())
                print(json.dumps({"frame": frame, "simulated_on_one_device": True, "gpus": n, "pass": k + 1,
                                  "added": e if k == 0 else e - ends[k - 1], "sampled_pixels_per_shard": active,
                                  "pass_ms": [round(v, 3) for v in t_pass],
                                  "select_ms": [round(a + b, 3) for a, b in zip(t_over, t_list)],
                                  "efficiency": round(sum(t) / (n * max(t)), 4), "pixels_over": n_over,
                                  "active_after": int(st[:, 4].sum())}), flush=True)
                if n_over <= args.fraction * W * H:
                    break
                active = [int(v) for v in st[:, 4]]
                units = [max(int(v), 1) for v in st[:, 5]]
            print(json.dumps({"frame": frame, "simulated_on_one_device": True, "gpus": n, "passes": k + 1,
                              "sum_shard_ms": round(sum_all, 2), "sum_slowest_ms": round(sum_max, 2),
                              "frame_efficiency": round(sum_all / (n * sum_max), 4)}), flush=True)
        finally:
            for c in ctxs:
                c.close()


if __name__ == "__main__":
    main()
