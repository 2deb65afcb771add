#!/usr/bin/env python3
"""Cost of what filtered adaptive and multi-GPU frames add, same box, same run.

    python tools/filtered_frame_cost.py [--tag r16] [--size 1920x1080] [--rounds 7] [--scene box] [--out-dir DIR]

1. ptg_noise_active_device against ptg_noise_device on the same frame: two
   contexts hold the same 4 samples per sub-pixel, one from a uniform
   PTG_FLAG_MOMENTS pass, one from an adaptive pass over every pixel (so the
   sums are identical and the new kernel reads 4 bytes of count per pixel
   more).  HIP events, one warm-up, the two in alternating order over the
   rounds; the variance slab alone, and with rho.
2. The tail of a denoised frame after its last pass -- resolve, variance,
   gathers, un-shards, features, filter, the copy to the host -- through
   MultiContext.resolve_denoised as n local shards on ONE GPU (the gathers are
   device copies), against the one-device tail by the pieces
   ptg_render_denoised runs, and against the unfiltered MultiContext.resolve.
   Wall clock around the synchronous calls (they end with the image on the
   host), alternating order.  Link time between GPUs is NOT measured here.
Writes profiles/<tag>_filtered_frame_cost.txt and prints it.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "cpu-path-tracing_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ptgpu  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="r16")
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--scene", default="box")
    ap.add_argument("--out-dir", default="")
    args = ap.parse_args()
    W, H = (int(v) for v in args.size.split("x"))
    scn = ptgpu.make_scene(args.scene, W, H)
    cam = ptgpu.camera.with_config(scn.camera_parameters)
    samples, nsub = 4, 2
    pm = ptgpu.make_params(W, H, samples, nsub, flags=ptgpu.FLAG_MOMENTS)
    pa = ptgpu.make_params(W, H, samples, nsub)
    lines = [f"filtered-frame cost, {args.scene} {W}x{H} nsub {nsub}, {samples} samples per sub-pixel, "
             f"{args.rounds} rounds, lib {os.path.relpath(ptgpu.LIB_PATH, ROOT)}"]
    rec = {}
    dev = "cuda:0"
    var_u = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
    var_a, rho_u = torch.zeros_like(var_u), torch.zeros((H, W), dtype=torch.float32, device=dev)
    rho_a = torch.zeros_like(rho_u)
    with ptgpu.Context(scn, cam, device=0) as cu, ptgpu.Context(scn, cam, device=0) as ca:
        cu.reset_accumulation(pm)
        cu.accumulate(pm, 0, samples)
        ca.reset_accumulation(pa)
        ca.set_active_mask(pa)
        ca.accumulate_active(pa, samples)
        runs = {
            "noise var": lambda: cu.noise(pm, samples, 0.0, 1.0, var=var_u),
            "noise_active var": lambda: ca.noise_active(pa, 1.0, var=var_a),
            "noise var+rho": lambda: cu.noise(pm, samples, 0.0, 1.0, var=var_u, rho=rho_u),
            "noise_active var+rho": lambda: ca.noise_active(pa, 1.0, var=var_a, rho=rho_a),
        }
        ms = {k: [] for k in runs}
        for r in range(args.rounds):
            for k in (list(runs) if r % 2 == 0 else list(runs)[::-1]):
                runs[k]()  # warm-up
                ms[k].append(timed(runs[k]))
        torch.cuda.synchronize()
        same = torch.equal(var_u, var_a) and torch.equal(rho_u, rho_a)
        lines.append("1. variance slab, HIP events (min / max ms over the rounds); the two slabs are " +
                     ("bit-identical" if same else "DIFFERENT"))
        for k, v in ms.items():
            lines.append(f"   {k:22s} {min(v):.4f} / {max(v):.4f}")
        for kind in ("var", "var+rho"):
            ratio = min(ms[f"noise_active {kind}"]) / min(ms[f"noise {kind}"])
            lines.append(f"   noise_active / noise ({kind}): {ratio:.3f}")
            rec[f"noise_active_over_noise_{kind}"] = ratio
        rec["noise_ms"] = {k: min(v) for k, v in ms.items()}
        # 2. the one-device tail by its pieces
        k5 = ptgpu.denoise_defaults()
        k5.pixel_spread = ptgpu.pixel_spread(cam, W, H)
        color = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
        feat = cu.features(pm)
        scratch = torch.empty(ptgpu.denoise_scratch_bytes(W, H) // 4, dtype=torch.float32, device=dev)
        host = np.zeros((H, W, 3), dtype=np.float32)

        def one_device_device_part():
            cu.resolve(color, pm, samples)
            cu.noise(pm, samples, 0.0, 1.0, var=var_u)
            cu.features(pm, feat)
            return ptgpu.denoise(color, var_u, feat, k5, scratch=scratch)

        def one_device_tail():
            host[...] = one_device_device_part().cpu().numpy()

        one_device_tail()
        ev = [timed(one_device_device_part) for _ in range(args.rounds)]
        want = host.copy()
    tails = {"one device (pieces)": one_device_tail}
    ctxs = []
    img = {}
    for n in (1, 2, 4, 8):
        m = ptgpu.MultiContext(scn, cam, [0], local_shards=n)
        m.reset_accumulation(pm)
        m.accumulate(pm, 0, samples)
        ctxs.append(m)
        img[n] = np.zeros((H, W, 3), dtype=np.float32)
        tails[f"{n} local shards, filtered"] = (lambda m=m, n=n: m.resolve_denoised(img[n], pm, samples))
        tails[f"{n} local shards, unfiltered"] = (lambda m=m, n=n: m.resolve(img[n], pm, samples))
    # (the one-device context is closed: its tail is timed on a fresh one)
    with ptgpu.Context(scn, cam, device=0) as cu:
        cu.reset_accumulation(pm)
        cu.accumulate(pm, 0, samples)
        ms = {k: [] for k in tails}
        for r in range(args.rounds):
            for k in (list(tails) if r % 2 == 0 else list(tails)[::-1]):
                tails[k]()  # warm-up
                ms[k].append(wall(tails[k]))
    equal = True
    for n in img:
        ctxs[[1, 2, 4, 8].index(n)].resolve_denoised(img[n], pm, samples)
        equal = equal and np.array_equal(img[n], want)
    for m in ctxs:
        m.close()
    lines.append("2. tail of a denoised frame, wall clock incl. the copy to the host (min / max ms); the filtered "
                 "images are " + ("bit-identical to the one-device one" if equal else "DIFFERENT"))
    lines.append(f"   one device, device part only (HIP events): {min(ev):.4f} / {max(ev):.4f}")
    for k, v in ms.items():
        lines.append(f"   {k:30s} {min(v):.4f} / {max(v):.4f}")
    lines.append("   gathers here are device copies on one GPU: link time on a multi-GPU node is not measured")
    rec["tail_ms"] = {k: min(v) for k, v in ms.items()}
    rec["one_device_device_part_ms"] = min(ev)
    lines.append(json.dumps(rec))
    text = "\n".join(lines) + "\n"
    out_dir = args.out_dir or os.path.join(ROOT, "profiles")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, f"{args.tag}_filtered_frame_cost.txt"), "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
