#!/usr/bin/env python3
"""Cost of the denoiser at a frame size, same box: the feature pass and the
a-trous filter per step, the tiled LDS kernel against the plain one.

    python tools/denoise_cost.py [--tag r14] [--size 1920x1080] [--rounds 5] [--scene box]

One noisy frame (16 spp) gives colour, variance and features.  The filter is
timed with HIP events at iterations = 1 .. 8, each after one warm-up call, the
two kernels in alternating order over the rounds; the time of step 2^(n-1) is
t(n) - t(n-1) of the per-count minima (each iteration is one Vbar kernel and
one filter kernel).  Each step is set against the bytes it must move at least
once -- colour, variance and the features in (72 B per pixel), colour and
variance out (24 B) -- at the 8 TB/s the HBM is specified for.  Steps above 16
run the plain kernel in either setting.  Writes
profiles/<tag>_denoise_cost.txt and prints it.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "cpu-path-tracing_amd")]

import torch  # noqa: E402

import ptgpu  # noqa: E402

HBM_BYTES_PER_S = 8.0e12
MIN_BYTES_PER_PIXEL = 72 + 24


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="r14")
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--scene", default="box")
    args = ap.parse_args()
    W, H = (int(v) for v in args.size.split("x"))
    scn = ptgpu.make_scene(args.scene, W, H)
    cam = ptgpu.camera.with_config(scn.camera_parameters)
    samples = 4
    p = ptgpu.make_params(W, H, samples, 2, flags=ptgpu.FLAG_MOMENTS)
    lines = [f"denoiser cost, {args.scene} {W}x{H}, {args.rounds} rounds, lib "
             f"{os.path.relpath(ptgpu.LIB_PATH, ROOT)}"]
    with ptgpu.Context(scn, cam, device=0) as ctx:
        color = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda:0")
        var = torch.zeros_like(color)
        ctx.reset_accumulation(p)
        ctx.accumulate(p, 0, samples)
        ctx.resolve(color, p, samples)
        ctx.noise(p, samples, 0.0, 1.0, var=var)
        feat = ctx.features(p)  # warm-up
        ft = [timed(lambda: ctx.features(p, feat)) for _ in range(args.rounds)]
        lines.append(f"features pass: min {min(ft):.4f} ms, max {max(ft):.4f} ms (nsub 2: 4 first-hit scans per pixel)")
    k = ptgpu.denoise_defaults()
    k.pixel_spread = ptgpu.pixel_spread(cam, W, H)
    scratch = torch.empty(ptgpu.denoise_scratch_bytes(W, H) // 4, dtype=torch.float32, device="cuda:0")
    kernels = (("tiled", 0), ("plain", 1))
    ms = {name: {n: [] for n in range(1, 9)} for name, _ in kernels}
    outs = {}
    for r in range(args.rounds):
        for name, choice in (kernels if r % 2 == 0 else kernels[::-1]):
            for n in range(1, 9):
                k.iterations = n
                ptgpu.denoise(color, var, feat, k, scratch=scratch, kernel_=choice)  # warm-up
                ms[name][n].append(timed(lambda: ptgpu.denoise(color, var, feat, k, scratch=scratch, kernel_=choice)))
            k.iterations = 5
            outs[name] = ptgpu.denoise(color, var, feat, k, scratch=scratch, kernel_=choice).cpu()
    lines.append("the two kernels' 5-iteration images are " +
                 ("bit-identical" if torch.equal(outs["tiled"], outs["plain"]) else "DIFFERENT"))
    floor_ms = W * H * MIN_BYTES_PER_PIXEL / HBM_BYTES_PER_S * 1e3
    lines.append(f"least traffic per iteration: {W * H * MIN_BYTES_PER_PIXEL / 1e6:.1f} MB = {floor_ms:.4f} ms at 8 TB/s")
    lines.append("step   tiled ms  (of floor)   plain ms  (of floor)   plain / tiled")
    rec = {}
    for n in range(1, 9):
        t = {name: min(ms[name][n]) - (min(ms[name][n - 1]) if n > 1 else 0.0) for name, _ in kernels}
        rec[1 << (n - 1)] = t
        lines.append(f"{1 << (n - 1):4d}  {t['tiled']:9.4f}  ({100 * floor_ms / t['tiled']:5.1f} %)  "
                     f"{t['plain']:9.4f}  ({100 * floor_ms / t['plain']:5.1f} %)  {t['plain'] / t['tiled']:6.2f}")
    five = {name: min(ms[name][5]) for name, _ in kernels}
    spread = {name: (min(ms[name][5]), max(ms[name][5])) for name, _ in kernels}
    lines.append(f"5 iterations (steps 1..16): tiled {five['tiled']:.4f} ms (max {spread['tiled'][1]:.4f}), plain "
                 f"{five['plain']:.4f} ms (max {spread['plain'][1]:.4f}): plain / tiled {five['plain'] / five['tiled']:.2f}")
    lines.append(json.dumps({"per_step_ms": rec, "five_iterations_ms": five, "features_ms_min": min(ft)}))
    text = "\n".join(lines) + "\n"
    out_dir = os.path.join(ROOT, "profiles")
    with open(os.path.join(out_dir, f"{args.tag}_denoise_cost.txt"), "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
