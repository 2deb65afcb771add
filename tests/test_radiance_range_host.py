"""The premises of tests/test_gpu_radiance_range.py, on the oracle alone (no
GPU): the scenes of tests/range_scenes.py really produce the out-of-range
classes they are named for, the numpy restatement of the clip
(tests/test_gpu_noise.py: _cl, _quant, _sums) agrees with the oracle's own
accumulation (po_render_xs_f32_ex) on such paths, and no u64 sum of any frame
the GPU tests compare can wrap: at most 3 samples of a (pixel, sub-pixel,
channel) are clipped to 2^30 (include/ptgpu.h "Sample accumulation": 4 x 2^62
is 2^64).
"""
import json
import os

import numpy as np
import pytest

import pyoracle as po
import range_scenes as rs
import shape_scenes as ss
from conftest import GOLDEN
from test_gpu_adaptive import _resolve_at
from test_gpu_noise import SEED, _paths_and_segments, _quant, _sums

NT = max(1, min(16, int(os.environ.get("OMP_NUM_THREADS", "8"))))

# every whole frame the GPU module compares with the oracle: scene, W, H, samples, nsub
FRAMES = [(name,) + rs.base_shape(name) for name in rs.CASES] + [
    ("over", 14, 6, 3, 3),  # 7 pixels x 9 sub-pixels: 63 slots
    ("nanwalls", 40, 4, 3, 1),  # 64 pixels per wave, a partial group
]
IDS = [f"{f[0]}-{f[1]}x{f[2]}x{f[3]}-nsub{f[4]}" for f in FRAMES]
COOP = ("neg", 256, 160, 8, 8)  # tests/test_gpu_frame_shapes.py's lin_nsub8_coop; four of its rows meet the oracle


def coop_rows():
    """Image rows of the cooperative frame that the GPU test compares: the first, the two either side
    of the level boundary of its recorded plan, the last (slab row j is image row j)."""
    _, W, H, n, nsub = COOP
    with open(os.path.join(GOLDEN, "launch_plans.json")) as f:
        plan = {p["name"]: p for p in json.load(f)["plans"]}[f"n9 {W}x{H}x{n} nsub{nsub}"]
    b = plan["lvl_group"][1] // plan["waves_per_row"]
    assert 0 < b - 1 and b < H - 1
    return plan, (0, b - 1, b, H - 1)


def count_high(E):
    """Per (pixel, sub-pixel, channel) the samples clipped to 2^30, as Python integers."""
    with np.errstate(invalid="ignore"):
        return [int(v) for v in (E > np.float32(rs.TOP)).sum(axis=3).reshape(-1)]


@pytest.mark.parametrize("frame", FRAMES, ids=IDS)
def test_classes_restatement_and_no_wrap(frame):
    name, W, H, n, nsub = frame
    E, segs = _paths_and_segments(name, W, H, n, nsub)
    masks = rs.classes(E)
    counts = {k: int(v.sum()) for k, v in masks.items()}
    bad = int(rs.clipped(E).sum())
    print(f"{name} {W}x{H}x{n} nsub {nsub}: {E[..., 0].size} paths, {int(segs.sum())} segments, classes {counts}, "
          f"+inf {int(np.isposinf(E).any(axis=-1).sum())}, clipped paths {bad}")
    # 1. the classes the scene is there for
    want = rs.CLASSES[name]
    if (W, H, n, nsub) == rs.base_shape(name):
        for k, figure in want.items():
            floor = figure if name == "bvh_mix" else (figure + 1) // 2
            assert counts[k] >= floor, (k, counts[k], floor)
    else:
        for k in want:
            assert counts[k] > 0, k
    for k in rs.CLIPPED + ("edge",):  # a class the scene is not named for is absent
        if k not in want:
            assert counts[k] == 0, k
    if name == "edge":  # a path at exactly 2^30 is counted only through its other components
        assert bad == counts["high"] and counts["edge"] > 0
    if name == "edge_in":  # ... and here it has none: exactly 2^30 is in range
        assert bad == 0 and counts["edge"] > 0
    if name == "cap":
        assert bad == 0 and int(segs.sum()) == 100 * segs.size and (segs == 100).all()
    if name == "nanwalls":
        assert (segs == 100).all() and int(np.isposinf(E).any(axis=-1).sum()) > 0
    if name == "tiny":  # sums of a few units of 2^-32
        tiny, _ = _sums(E, 0, n)
        assert bad == 0 and 0 < int(tiny.max()) <= 3 * n and (tiny > 0).mean() > 0.01
    if name == "s2sat":
        assert bad == 0 and counts["sq"] > 0
    # 2. no sum wraps: at most 3 samples per sum are clipped to 2^30 (each adds 2^62)
    high = count_high(E)
    assert max(high) <= 3, max(high)
    q = _quant(E).reshape(-1, n, 3)
    exact = [sum(int(v) for v in q[i, :, c]) for i in range(q.shape[0]) for c in range(3)]
    assert max(exact) < 2 ** 64
    S1, _ = _sums(E, 0, n)
    assert exact == [int(v) for v in S1.reshape(-1)]  # so numpy's modular u64 sum is the integer sum
    # 3. the restatement against the oracle's own accumulation
    sp, ca = ss.oracle_arrays(*rs.make(name, W, H))
    img, rsegs, rbad = po.render_xs_f32_count(sp, ca, W, H, n, nsub, SEED, nthreads=NT)
    assert rsegs == int(segs.sum())
    assert rbad == bad
    pix = _resolve_at(S1, np.full((H, W), n), nsub)
    assert np.isfinite(img).all() and img.min() >= 0.0 and img.max() <= 1.0
    assert img.tobytes() == pix.tobytes()
    if name == "neg":
        print(f"neg: image mean {float(img.mean()):.3f}")
        assert img.mean() > 0.035  # the frame is lit (0.070 measured)


def test_cooperative_frame_has_no_high_clip():
    """The 256x160 frame holds 8 samples per sum, so it must have no sample clipped to 2^30.
    Scene neg cannot have one at any shape: only the lamp's colour (1.8) exceeds 1, the
    throughput grows on the first 5 segments only (from the 6th on Russian roulette scales the
    colour by 1 / its largest component), and |emission| <= 9, so every component stays below
    100 x 9 x 1.8^5 < 2^15.  Checked here on the four rows the GPU test compares (every 16th
    pixel, path by path), which also hold the class the scene is there for."""
    name, W, H, n, nsub = COOP
    _, rows = coop_rows()
    sp, ca = ss.oracle_arrays(*rs.make(name, W, H))
    xs = range(0, W, 16)
    E = np.zeros((len(rows), len(xs), nsub * nsub, n, 3), dtype=np.float32)
    for r, j in enumerate(rows):  # image row j is y = H - 1 - j from the bottom
        for i, x in enumerate(xs):
            for k in range(nsub * nsub):
                for s in range(n):
                    E[r, i, k, s], _ = po.sample_f32(sp, ca, W, H, nsub, SEED, x, H - 1 - j, k % nsub, k // nsub, s)
    c = {k: int(v.sum()) for k, v in rs.classes(E).items()}
    print(f"neg {W}x{H}x{n} nsub {nsub}, rows {rows}, every 16th pixel: {E[..., 0].size} paths, classes {c}, "
          f"max |c| {float(np.abs(E).max()):.4g}")
    assert c["high"] == 0 and c["nan"] == 0 and c["neg"] > 0
    assert float(np.abs(E).max()) < 100 * 9 * 1.8 ** 5 < 2.0 ** 15


@pytest.mark.parametrize("name", ["over", "neg", "nanwalls"])
def test_mode_a_xs_on_out_of_range_scenes(name):
    """What PTG_FLAG_REFERENCE_F64 is compared with: the double path does not clip; printed: whether
    its image has non-finite pixels."""
    W, H, n, nsub = rs.BASE
    sp, ca = ss.oracle_arrays(*rs.make(name, W, H))
    img, segs = po.render_xs_f64(sp, ca, W, H, n, nsub, SEED, nthreads=NT)
    fin = np.isfinite(img)
    print(f"{name}: Mode A/xs has {int((~fin).any(axis=2).sum())} non-finite pixels of {W * H}, "
          f"min {float(img[fin].min()):.4g}, max {float(img[fin].max()):.4g}, segments {segs}")
    assert segs >= W * H * nsub * nsub * n
