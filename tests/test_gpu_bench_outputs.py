"""bench.py's plain and --full runs on one GPU: a plain run reports the timed
steps only and, with --dump-outputs, writes the last timed frame -- the image
a caller of Context.render_device holds for the same scene, size and seed --
as float32; --full adds the roofline and the CPU baseline with its quality
rows to the same line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, SPP = 256, 128, 16
FRAME = ["--width", str(W), "--height", str(H), "--spp", str(SPP)]
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "segments_per_s", "cpu_baseline", "speedup_vs_cpu_baseline")


def _bench(*args):
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a visible MI355X")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *args, *FRAME],
                         capture_output=True, text=True, timeout=180, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


def test_plain_run_is_lean_and_dumps_the_last_frame(tmp_path):
    import ptgpu

    d = tmp_path / "dump"
    line = _bench("--steps", "3", "--warmup", "2", "--dump-outputs", str(d))
    assert all(k in line for k in HEADLINE) and not any(k in line for k in FULL_ONLY)
    assert line["full"] is False and line["steps"] == 3 and line["warmup"] == 2
    assert line["unit"] == "Mray-samples/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["config"]["workload"] == f"box {W}x{H} {SPP}spp"
    # value and ms_per_step are one measurement: samples of the frame / the time of one step
    assert line["ms_per_step"] > 0
    assert abs(line["value"] - W * H * SPP / (line["ms_per_step"] * 1e-3) / 1e6) <= 0.01 * line["value"] + 0.01
    assert sorted(os.listdir(d)) == ["image.npy"]
    img = np.load(d / "image.npy")
    assert img.dtype == np.float32 and img.shape == (H, W, 3)
    assert line["outputs"]["image"]["shape"] == [H, W, 3]
    # the same inputs through the API the benchmark times
    scn = ptgpu.box_scene(W, H)
    cam = ptgpu.camera.with_config(scn.camera_parameters)
    rows = ptgpu.shard_rows(H, ptgpu.DEFAULT_BAND_ROWS, 1)
    with ptgpu.Context(scn, cam, device=0) as ctx:
        slab = torch.zeros(rows * W * 3, dtype=torch.float32, device="cuda:0")
        ctx.render_device(slab, ptgpu.make_params(W, H, SPP // 4, 2, ptgpu.DEFAULT_SEED))
        torch.cuda.synchronize()
        want = ptgpu.unshard_host(slab.cpu().numpy(), W, H, ptgpu.DEFAULT_BAND_ROWS, 1)
    assert np.isfinite(img).all() and img.mean() > 0
    assert np.array_equal(img, want)


def test_full_run_adds_roofline_and_cpu_baseline():
    line = _bench("--full", "--steps", "2", "--warmup", "1")
    assert all(k in line for k in HEADLINE) and line["full"] is True and line["steps"] == 2
    assert line["roofline"]["kernel_ms"] > 0 and line["roofline"]["segments_per_sample"] > 1
    assert line["segments_per_s"] > 0
    cpu = line["cpu_baseline"]
    assert cpu["value"] > 0 and cpu["kind"] in ("reference", "port")
    q = cpu["quality"]
    assert len(q["rows"]) == 4 and q["image_mean"] > 0
    assert all(np.isfinite(q[k]) for k in ("rmse_vs_cpu_fp32", "max_abs_vs_cpu_fp32", "rmse_vs_cpu_fp64_same_rng"))
    assert line["speedup_vs_cpu_baseline"] > 0
