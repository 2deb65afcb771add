#!/usr/bin/env python3
"""Frame time with and without PTG_FLAG_STRATIFIED, with and without light sampling.

    python tools/stratified_rate.py [--rounds 3] [--size 1920x1080] [--spp 1024]
        [--scenes box,simple,synthetic:10000] [--exact-math] [--out profiles/NAME.json]

Per scene the one-shot frame (ptg_render_device), timed with HIP events after
one warm-up frame of each variant: plain, stratified, light sampling, light
sampling + stratified, interleaved -- every round runs all four, odd rounds in
reverse order.  Prints one JSON line per measurement and a summary; --out
also writes the summary to a file.  PTGPU_LIB names another build of the
library (the parent commit's, for the "flag off costs nothing" A/B: its
`plain` and `light_sampling` rows against this tree's).

What a frame costs is half of the answer; the other half is the variance it
buys (tests/test_gpu_stratified.py prints the median variance ratio plain /
stratified at equal sample counts).  time to equal variance = (flagged ms /
plain ms) / that ratio: below 1, the flag wins.
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
    ap.add_argument("--scenes", default="box,simple,synthetic:10000")
    ap.add_argument("--exact-math", action="store_true")
    ap.add_argument("--no-flag", action="store_true", help="the unflagged variants only (a build without the flag)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    W, H = (int(v) for v in args.size.split("x"))
    samples = args.spp // 4
    mode = ptgpu.FLAG_EXACT_MATH if args.exact_math else 0
    LS, ST = ptgpu.FLAG_LIGHT_SAMPLING, 64  # (64: PTG_FLAG_STRATIFIED, also where the package predates it)
    variants = [("plain", mode), ("stratified", mode | ST), ("light_sampling", mode | LS),
                ("light_sampling_stratified", mode | LS | ST)]
    if args.no_flag:
        variants = [v for v in variants if not v[1] & ST]
    summary = {}
    for name in args.scenes.split(","):
        scn = ptgpu.make_scene(name, W, H)
        cam = ptgpu.camera.with_config(scn.camera_parameters)
        ms = {v: [] for v, _ in variants}
        out = torch.empty(H * W * 3, dtype=torch.float32, device="cuda:0")
        with ptgpu.Context(scn, cam, device=0) as ctx:
            params = {v: ptgpu.make_params(W, H, samples, 2, ptgpu.DEFAULT_SEED, flags=f) for v, f in variants}
            for v, _ in variants:
                timed(lambda: ctx.render_device(out, params[v]))  # warm-up
            for r in range(args.rounds):
                for v, _ in (variants if r % 2 == 0 else variants[::-1]):
                    ms[v].append(timed(lambda: ctx.render_device(out, params[v])))
                    print(json.dumps({"scene": name, "round": r + 1, "variant": v, "frame_ms": round(ms[v][-1], 3)}),
                          flush=True)
        rec = {"lights": ptgpu.light_list(scn, cam)}
        for v, _ in variants:
            t = ms[v]
            rec[v] = {"frame_ms_min": round(min(t), 3), "frame_ms_max": round(max(t), 3),
                      "frame_ms_mean": round(sum(t) / len(t), 3)}
        if not args.no_flag:
            rec["time_ratio"] = round(rec["stratified"]["frame_ms_mean"] / rec["plain"]["frame_ms_mean"], 4)
            rec["time_ratio_light_sampling"] = round(rec["light_sampling_stratified"]["frame_ms_mean"] /
                                                     rec["light_sampling"]["frame_ms_mean"], 4)
        summary[f"{name} {W}x{H} {args.spp}spp"] = rec
    doc = {"tool": "tools/stratified_rate.py", "library": os.path.basename(os.environ.get("PTGPU_LIB", "")) or "this tree's",
           "kernel_source_hash": ptgpu.kernel_source_hash(), "mode": "exact" if args.exact_math else "fast",
           "rounds": args.rounds, "summary": summary}
    print(json.dumps(doc))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
