"""The default (fast) arithmetic mode, path by path.

(a) The fast render kernel against the fast trace kernel, bit for bit.  Both
run the same segment<kBvh, false> device code; the build has -ffp-contract=off
and the GPU's approximate instructions are deterministic, so the raw sums of a
whole small frame (PTG_FLAG_MOMENTS passes: refill, prefetch, LDS-staged
records, partial groups) must equal the quantised sums of the one-path-per-
thread trace kernel's radiances:
    S1 == sum quant(c),  S2 == sum quant(cl(c) cl(c))    (tests/test_gpu_noise.py)
and the one-shot fast frame (in-wave / cooperative resolve) must equal the
resolve of S1.  (The frames hold up to 12,288 paths.)

(b) Fast against exact on 4,096 seeded paths of a 160x120 frame, both from the
trace kernel of one context.  A path mismatches when its segment counts differ
or a channel differs by more than 1e-3 max(1, max |exact|).  The yardstick is
the oracle's own sensitivity to the same change: y = the mismatches between
po.sample_f32 in Mode B and under BV_IEEE_SQRT | BV_IEEE_DIV | BV_LIBM_TRIG,
the variant that swaps the primitives the fast mode swaps (sqrt and rsq, the
division, the trig).  Asserted: mismatches <= 3 y + S -- 3 because both counts
are small Poisson-like numbers of the same origin; S covers the scenes with
y = 0: the smallest integer that puts every bound at twice the count measured
on an MI355X or more (at most 20 = 0.5 % of the paths).  The sliver case
(tests/shape_scenes.py) is there for kAxAnyOut's `win & neg`: a build without
it moves 19 of its paths, and none of any other scene's.

Measured on an MI355X (S = 2: open_014's one path against y = 0):

    scene            y   measured   bound (3 y + 2)
    box              3       3         11
    box_mirror       8      10         26
    simple           0       0          2
    room4            0       0          2
    room16           9       8         29
    room59          45      45        137
    sunk_scene      12      11         38
    open_014         0       1          2
    sliver           0       0          2
    synthetic:300    0       0          2
    cluster64        0       0          2
    cluster65        0       0          2
    twins_lin_low    0       0          2
    twins_room_low  17      14         53
    twins_bvh_low    0       0          2
    stack9_a         0       0          2

(The last four hold exact ties, tests/tie_scenes.py: the fast mode gives a tie
to the same sphere as the exact mode.  S stays 2: every bound is at least
twice its measured count.)
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import ptgpu  # noqa: E402
import pyoracle as po  # noqa: E402
import range_scenes  # noqa: E402
import shape_scenes as ss  # noqa: E402
import tie_scenes  # noqa: E402
from test_gpu_noise import _accumulate, _quant, _read, _sums  # noqa: E402
from test_wall_rules import sunk_scene  # noqa: E402

SEED = 0x5EED0001
EXACT = ptgpu.FLAG_EXACT_MATH
MOM = ptgpu.FLAG_MOMENTS


def _require_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a visible MI355X")


def _scene(name, W, H):
    if name in ss.CASES:
        return ss.make(name, W, H)
    if name in range_scenes.CASES:  # (tests/test_gpu_radiance_range.py)
        return range_scenes.make(name, W, H)
    if name in tie_scenes.CASES:  # (tests/test_gpu_ties.py)
        return tie_scenes.make(name, W, H)
    scn = sunk_scene(W, H) if name == "sunk_scene" else ptgpu.make_scene(name, W, H)
    return scn, ptgpu.camera.with_config(scn.camera_parameters)


# ---- (a) render kernel == trace kernel ---------------------------------------
# W, H, samples, nsub, passes
FRAMES = {
    "room4": (40, 12, 4, 2, [(0, 4)]),  # 2.5 pixel groups of 16: the nv < 64 path
    "room59": (32, 8, 4, 2, [(0, 1), (1, 4)]),
    "box_mirror": (32, 12, 8, 2, [(0, 3), (3, 8)]),
    "box": (14, 6, 4, 3, [(0, 4)]),  # 7 pixels x 9 sub-pixels: 63 slots
    "cluster64_lens": (32, 8, 4, 2, [(0, 4)]),
    "cluster65_lens": (32, 8, 4, 2, [(0, 4)]),
    "synthetic:300": (32, 18, 4, 2, [(0, 4)]),
}


def _frame_coords(W, H, n, nsub):
    """Every path of the frame, [H (y from the bottom), W, nsub^2 (sy, sx), n] x (x, y, sx, sy, s)."""
    y, x, sy, sx, s = np.meshgrid(np.arange(H), np.arange(W), np.arange(nsub), np.arange(nsub), np.arange(n),
                                  indexing="ij")
    return np.stack([x, y, sx, sy, s], axis=-1).reshape(-1, 5).astype(np.int32)


@pytest.mark.parametrize("name", list(FRAMES))
def test_fast_render_kernel_equals_fast_trace_kernel(name):
    _require_gpu()
    check_render_equals_trace(name, *FRAMES[name])


def check_render_equals_trace(name, W, H, n, nsub, passes, flags=0, count=False):
    """The identity of (a) on one frame in the mode `flags` (also used by
    tests/test_gpu_frame_shapes.py and tests/test_gpu_radiance_range.py).  Returns the trace
    kernel's radiances [H (image row), W, nsub^2, n, 3] and, with `count`, the four counters of
    the one-shot frame rendered once more with PTG_FLAG_COUNT_NONFINITE (the same image)."""
    p = ptgpu.make_params(W, H, n, nsub, SEED, flags=flags | MOM)
    plain = ptgpu.make_params(W, H, n, nsub, SEED, flags=flags)
    counting = ptgpu.make_params(W, H, n, nsub, SEED, flags=flags | ptgpu.FLAG_COUNT_TESTS | ptgpu.FLAG_COUNT_NONFINITE)
    coords = _frame_coords(W, H, n, nsub)
    with ptgpu.Context(*_scene(name, W, H)) as ctx:
        _accumulate(ctx, p, passes)
        g1, g2 = _read(ctx, p)
        c, _ = ctx.trace_samples(torch.from_numpy(coords).cuda(), plain)
        shot = torch.full((H * W * 3,), -7.0, dtype=torch.float32, device="cuda")
        ctx.render_device(shot, plain)
        if count:
            counted = torch.full((H * W * 3,), -7.0, dtype=torch.float32, device="cuda")
            counters = torch.zeros(4, dtype=torch.int64, device="cuda")
            ctx.render_device(counted, counting, counters)
        torch.cuda.synchronize()
    # trace rows count y from the bottom: image row H - 1 - y
    E = c.cpu().numpy().reshape(H, W, nsub * nsub, n, 3)[::-1]
    S1, S2 = _sums(E, 0, n)
    bad1, bad2 = int((g1 != S1).sum()), int((g2 != S2).sum())
    print(f"{name}: {coords.shape[0]} paths, S1 differs at {bad1}, S2 at {bad2} of {S1.size} sums; "
          f"lit sums {float((S1 > 0).mean()):.3f}")
    assert (S1 > 0).mean() > 0.01  # the frame is lit (room4's four samples find its lamps on 4 % of the sums)
    assert np.array_equal(S1, _quant(E).sum(axis=3, dtype=np.uint64))  # (the helper sums what it says)
    assert bad1 == 0 and bad2 == 0
    # resolve of S1: _noise_ref's pix, the clamped sub-pixel means added in (sy, sx) order
    m1 = S1.astype(np.float64) * 2.0 ** -32 / n
    inv32 = np.float32(1.0) / np.float32(nsub * nsub)
    pix = np.zeros((H, W, 3), dtype=np.float32)
    for j in range(nsub * nsub):
        mean = np.clip(m1[:, :, j].astype(np.float32), np.float32(0), np.float32(1))
        pix = (mean.astype(np.float64) * float(inv32) + pix.astype(np.float64)).astype(np.float32)
    assert np.array_equal(shot.cpu().numpy().reshape(H, W, 3), pix)
    if not count:
        return E, None
    assert torch.equal(shot, counted)  # the counting kernel's image is the plain one's
    return E, counters.cpu().tolist()


# ---- (b) fast against exact, path by path -------------------------------------
N_PATHS = 4096
TW, TH = 160, 120
S_SLACK = 2  # the table above; it may not exceed 20 (0.5 % of the paths)
SCENES_B = ["box", "box_mirror", "simple", "room4", "room16", "room59", "sunk_scene", "open_014", "sliver",
            "synthetic:300", "cluster64", "cluster65", "twins_lin_low", "twins_room_low", "twins_bvh_low", "stack9_a"]


def _coords():
    rng = np.random.default_rng(7)
    n = N_PATHS
    return np.stack([rng.integers(0, TW, n), rng.integers(0, TH, n), rng.integers(0, 2, n),
                     rng.integers(0, 2, n), rng.integers(0, 1 << 20, n)], axis=1).astype(np.int32)


def _mismatches(exact, esegs, other, osegs):
    tol = 1e-3 * np.maximum(1.0, np.abs(exact).max(axis=1))
    with np.errstate(invalid="ignore"):
        far = ~(np.abs(other.astype(np.float64) - exact.astype(np.float64)).max(axis=1) <= tol)
    return (esegs != osegs) | far


@functools.lru_cache(maxsize=None)
def _oracle_yardstick(name):
    """y: paths the oracle itself moves when sqrt/rsq, the division and the trig are swapped."""
    sp, ca = ss.oracle_arrays(*_scene(name, TW, TH))
    coords = _coords()

    def run():
        out = np.zeros((N_PATHS, 3), dtype=np.float32)
        segs = np.zeros(N_PATHS, dtype=np.int64)
        for i, (x, y, sx, sy, s) in enumerate(coords.tolist()):
            out[i], segs[i] = po.sample_f32(sp, ca, TW, TH, 2, SEED, x, y, sx, sy, s)
        return out, segs

    b, bs = run()
    with po.mode_b_variant(po.BV_IEEE_SQRT | po.BV_IEEE_DIV | po.BV_LIBM_TRIG):
        v, vs = run()
    return int(_mismatches(b, bs, v, vs).sum()), b, bs


@pytest.mark.parametrize("name", SCENES_B)
def test_fast_paths_stay_with_the_exact_paths(name):
    _require_gpu()
    y, ref, rsegs = _oracle_yardstick(name)
    coords = torch.from_numpy(_coords()).cuda()
    with ptgpu.Context(*_scene(name, TW, TH)) as ctx:
        e, es = ctx.trace_samples(coords, ptgpu.make_params(TW, TH, 1, 2, SEED, flags=EXACT))
        f, fs = ctx.trace_samples(coords, ptgpu.make_params(TW, TH, 1, 2, SEED))
        torch.cuda.synchronize()
    e, es, f, fs = e.cpu().numpy(), es.cpu().numpy(), f.cpu().numpy(), fs.cpu().numpy()
    assert e.tobytes() == ref.tobytes() and np.array_equal(es, rsegs)  # the exact side is the oracle's Mode B
    bad = _mismatches(e, es, f, fs)
    measured, bound = int(bad.sum()), 3 * y + S_SLACK
    print(f"{name}: y {y}, measured {measured}, bound {bound}; first {_coords()[bad][:4].tolist()}")
    assert np.isfinite(f).all() and (f >= 0.0).all()
    assert measured <= bound
