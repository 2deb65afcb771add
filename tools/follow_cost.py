#!/usr/bin/env python3
"""Cost of the followed features against the first-hit features, same box.

    python tools/follow_cost.py [--tag r18] [--size 1920x1080] [--rounds 7]

ptg_features_follow_device at B = 0, 1 and 8 against ptg_features_device on
box, box_mirror and synthetic:10000 (nsub 2: four rays per pixel), timed with
HIP events, each call after one warm-up call, the four variants in alternating
order over the rounds; the minimum and the maximum per variant.  The followed
pass is set against a 5-iteration filter and a bench frame (--filter-ms,
--frame-ms: the figures of profiles/r14_denoise_cost.txt and the bench line
by default).  Writes profiles/<tag>_follow_cost.txt and prints it.
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
    ap.add_argument("--tag", default="r18")
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--scenes", default="box,box_mirror,synthetic:10000")
    ap.add_argument("--filter-ms", type=float, default=0.84, help="a 5-iteration filter at this size")
    ap.add_argument("--frame-ms", type=float, default=136.0, help="the bench frame (box 1920x1080, 1024 spp)")
    args = ap.parse_args()
    W, H = (int(v) for v in args.size.split("x"))
    variants = (("first-hit", None), ("B=0", 0), ("B=1", 1), ("B=8", 8))
    lines = [f"followed-feature cost, {W}x{H}, nsub 2, {args.rounds} rounds, lib {os.path.relpath(ptgpu.LIB_PATH, ROOT)}",
             f"shares: of a 5-iteration filter ({args.filter_ms} ms) and of the bench frame ({args.frame_ms} ms)",
             "scene              variant     min ms    max ms   / first-hit   of filter   of frame   mean bounces"]
    rec = {}
    for name in args.scenes.split(","):
        scn = ptgpu.make_scene(name, W, H)
        cam = ptgpu.camera.with_config(scn.camera_parameters)
        p = ptgpu.make_params(W, H, 4, 2)
        ms = {v: [] for v, _ in variants}
        mean_b = {}
        with ptgpu.Context(scn, cam, device=0) as ctx:
            feat = ctx.features(p)
            for r in range(args.rounds):
                for v, B in (variants if r % 2 == 0 else variants[::-1]):
                    ctx.features(p, feat, follow_bounces=B)  # warm-up
                    ms[v].append(timed(lambda: ctx.features(p, feat, follow_bounces=B)))
                    if r == 0:
                        torch.cuda.synchronize()
                        hit = feat[..., 7] > 0
                        mean_b[v] = float(feat[..., 11][hit].mean()) if bool(hit.any()) else 0.0
        base = min(ms["first-hit"])
        rec[name] = {v: {"min_ms": min(t), "max_ms": max(t), "mean_bounces": mean_b[v]} for v, t in ms.items()}
        for v, _ in variants:
            lo, hi = min(ms[v]), max(ms[v])
            lines.append(f"{name:18s} {v:10s} {lo:8.4f}  {hi:8.4f}   {lo / base:9.2f}   {100 * lo / args.filter_ms:7.1f} %  "
                         f"{100 * lo / args.frame_ms:7.3f} %   {mean_b[v]:8.3f}")
    lines.append(json.dumps(rec))
    text = "\n".join(lines) + "\n"
    with open(os.path.join(ROOT, "profiles", f"{args.tag}_follow_cost.txt"), "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
