#!/usr/bin/env python3
"""Frame time and scans per path with and without PTG_FLAG_LIGHT_SAMPLING.

    python tools/light_sampling_rate.py [--rounds 3] [--size 1920x1080] [--spp 1024]
        [--scenes box,simple,synthetic:10000] [--exact-math] [--out profiles/NAME.json]

Per scene the one-shot frame (ptg_render_device), timed with HIP events after
one warm-up frame of each variant: without the flag, with it, in alternating
order over the rounds.  Then one untimed frame of each through the counting
kernel (PTG_FLAG_COUNT_TESTS): scene scans per path -- shadow segments are
scans like any other.  Prints one JSON line per measurement and a summary;
--out also writes the summary to a file.

What a frame costs is half of the answer; the other half is the variance it
buys (tests/test_gpu_light_sampling.py prints the median variance ratio
plain / light sampling at equal sample counts).  time to equal variance =
(flagged ms / plain ms) / that ratio: below 1, light sampling wins.
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
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    W, H = (int(v) for v in args.size.split("x"))
    samples = args.spp // 4
    mode = ptgpu.FLAG_EXACT_MATH if args.exact_math else 0
    variants = [("plain", mode), ("light_sampling", mode | ptgpu.FLAG_LIGHT_SAMPLING)]
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
            for v, f in variants:
                seg = torch.zeros(3, dtype=torch.int64, device="cuda:0")
                ctx.render_device(out, ptgpu.make_params(W, H, samples, 2, ptgpu.DEFAULT_SEED,
                                                         flags=f | ptgpu.FLAG_COUNT_TESTS), seg)
                torch.cuda.synchronize()
                scans, spheres, boxes = seg.cpu().tolist()
                paths = W * H * 4 * samples
                t = ms[v]
                rec[v] = {"frame_ms_min": round(min(t), 3), "frame_ms_max": round(max(t), 3),
                          "frame_ms_mean": round(sum(t) / len(t), 3), "scans_per_path": round(scans / paths, 4),
                          "sphere_tests_per_scan": round(spheres / scans, 3),
                          "box_or_wall_tests_per_scan": round(boxes / scans, 3)}
            rec["time_ratio"] = round(rec["light_sampling"]["frame_ms_mean"] / rec["plain"]["frame_ms_mean"], 4)
            rec["scan_ratio"] = round(rec["light_sampling"]["scans_per_path"] / rec["plain"]["scans_per_path"], 4)
        summary[f"{name} {W}x{H} {args.spp}spp"] = rec
    doc = {"tool": "tools/light_sampling_rate.py", "kernel_source_hash": ptgpu.kernel_source_hash(),
           "mode": "exact" if args.exact_math else "fast", "rounds": args.rounds, "summary": summary}
    print(json.dumps(doc))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
