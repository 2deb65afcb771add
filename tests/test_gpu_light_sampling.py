"""PTG_FLAG_LIGHT_SAMPLING (next-event estimation for the small emissive
spheres, include/ptgpu.h) on the GPU.

1. Unbiased against the plain estimator, which is the reference of the test:
   raw per-pixel-channel means (from the exact sums S1, never the clamped
   image: DESIGN.md "Light sampling", the clamp trap) of 16 seeds per side
   through test_gpu_statistical.two_sample_check, unchanged.
2. The variance ratio plain / light sampling of the same renders: its median
   over pixel-channels is >= 2.2 on box and simple (half of the double
   prototype's 4.6 and 4.4; the factor 2 covers fp32 and the spread of the
   median of 9,216 sixteen-run variance ratios).  box_mirror: printed only --
   its walls are mirrors, no diffuse hit ever runs the step.
3. fp32, each mode, against PTG_FLAG_REFERENCE_F64 | PTG_FLAG_LIGHT_SAMPLING
   (csrc/ref64.hpp: the same step in double with the same draws): per-pixel
   RMSE < 1e-3, the north star's bar.
4. The frame does not depend on chunking, sharding, progressive passes or
   PTG_FLAG_MOMENTS, bit for bit, at the smallest shapes that reach each path.
5. The pool kernels against the one-thread trace kernel: sum over samples of
   quant(E) equals S1 bit for bit.
6. The adaptive guarantee: a pixel holding n_p samples equals the one-shot
   frame of n_p samples.
7. No lights, no change.   8. No path's radiance is NaN, negative or > 2^30.
9. Exact mode, per path, against the oracle's per-path double (Mode A/xs with
   the light list), within 4 times what a float32 run of the definition's
   numpy restatement (tests/light_ref.py) differs from it by.

Tests 1, 3, 4 and 5 also run on the scenes of tests/light_zoo.py ("zoo:NAME":
L up to 16, emitters of every material, overlapping lights, a light cut by a
wall, permuted scan positions, BVH scenes with several lights, hit points
inside a light), 32x24; test 1 there with the oracle's seeds and the sample
counts tests/test_oracle_light_sampling.py fixed on the CPU.

Measured on an MI355X (medians of test 2; RMSE of test 3): DESIGN.md "Light
sampling" records them.
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import light_ref  # noqa: E402
import light_zoo as zoo  # noqa: E402
import ptgpu  # noqa: E402
import test_oracle_light_sampling as oracle_ls  # noqa: E402
import tie_scenes  # noqa: E402
from test_gpu_statistical import two_sample_check  # noqa: E402

SEED = 0x5EED0001
EXACT = ptgpu.FLAG_EXACT_MATH
MOM = ptgpu.FLAG_MOMENTS
LS = ptgpu.FLAG_LIGHT_SAMPLING
MODES = pytest.mark.parametrize("mode", [0, EXACT], ids=["fast", "exact"])


def _require_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a visible MI355X")


@functools.lru_cache(maxsize=None)
def _scene(name, W, H):
    if name.startswith("zoo:"):  # (built for 32x24; other sizes keep that aspect ratio)
        assert W * zoo.H == H * zoo.W
        scn = zoo.CASES[name[4:]]()
    elif name in tie_scenes.LAMPS:  # (tests/test_gpu_ties.py: `three` with a dark twin of each light)
        scn = tie_scenes.make(name, W, H)[0]
    else:
        scn = ptgpu.make_scene(name, W, H)
    return scn, ptgpu.camera.with_config(scn.camera_parameters)


def _rows(p):
    return ptgpu.shard_rows(p.height, p.band_rows, p.shard_count)


def _frame(ctx, p, segments=None):
    out = torch.full((_rows(p) * p.width * 3,), -7.0, dtype=torch.float32, device="cuda")
    ctx.render_device(out, p, segments)
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(_rows(p), p.width, 3)


def _resolved(ctx, p, n):
    out = torch.full((_rows(p) * p.width * 3,), -7.0, dtype=torch.float32, device="cuda")
    ctx.resolve(out, p, n)
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(_rows(p), p.width, 3)


def _s1(ctx, p):
    """The exact sums S1: uint64 [rows, W, nsub^2, 3]."""
    shape = (_rows(p), p.width, p.num_subpixels ** 2, 3)
    s1 = torch.full((int(np.prod(shape)),), -1, dtype=torch.int64, device="cuda")
    ctx.read_moments(p, s1, None)
    torch.cuda.synchronize()
    return s1.cpu().numpy().view(np.uint64).reshape(shape)


# ---- 1, 2: the estimator against the plain one ------------------------------------
W1, H1, N1, RUNS = 64, 48, 1024, 16


@functools.lru_cache(maxsize=None)
def _seed_stats(name, mode):
    """Per side (plain, light sampling): mean and variance over RUNS seeds of the raw per-pixel-channel mean
    sum_sub S1 2^-32 / (n nsub^2), float64 [H, W, 3] each.  Read-only, shared by tests 1 and 2."""
    out = []
    with ptgpu.Context(*_scene(name, W1, H1)) as ctx:
        for side in (0, LS):
            means = []
            for r in range(RUNS):
                p = ptgpu.make_params(W1, H1, N1, 2, SEED + 0x9E3779B97F4A7C15 * (r + 1), flags=mode | MOM | side)
                ctx.reset_accumulation(p)
                ctx.accumulate(p, 0, N1)
                s1 = _s1(ctx, p)
                means.append(s1.astype(np.float64).sum(axis=2) * 2.0 ** -32 / (N1 * 4))
            g = np.stack(means)
            out.append((g.mean(0), g.var(0, ddof=1)))
    for m, v in out:
        m.setflags(write=False)
        v.setflags(write=False)
    return tuple(out)


@MODES
@pytest.mark.parametrize("name", ["box", "simple", "box_mirror"])
def test_unbiased_against_the_plain_estimator(name, mode):
    _require_gpu()
    (mp, vp), (ml, vl) = _seed_stats(name, mode)
    res = two_sample_check(ml, vl, mp, vp, RUNS)
    print(name, "exact" if mode else "fast", res)


@functools.lru_cache(maxsize=None)
def _zoo_seed_stats(name, mode):
    """_seed_stats for a zoo scene as tests/test_oracle_light_sampling.py takes them on the CPU: 32x24 at
    zoo.SAMPLES[name], the plain side from seeds 0..15, the flagged side from the disjoint seeds 32..47."""
    W, H, n = zoo.W, zoo.H, zoo.SAMPLES[name]
    out = []
    with ptgpu.Context(*_scene("zoo:" + name, W, H)) as ctx:
        for side, first in ((0, 0), (LS, 2 * RUNS)):
            means = []
            for r in range(first, first + RUNS):
                p = ptgpu.make_params(W, H, n, zoo.NSUB, SEED + 0x9E3779B97F4A7C15 * (r + 1), flags=mode | MOM | side)
                ctx.reset_accumulation(p)
                ctx.accumulate(p, 0, n)
                means.append(_s1(ctx, p).astype(np.float64).sum(axis=2) * 2.0 ** -32 / (n * zoo.NSUB ** 2))
            ctx.reset_accumulation(p)
            g = np.stack(means)
            out.append((g.mean(0), g.var(0, ddof=1)))
    return tuple(out)


@MODES
@pytest.mark.parametrize("name", list(zoo.CASES))
def test_unbiased_against_the_plain_estimator_on_the_zoo(name, mode):
    _require_gpu()
    (mp, vp), (ml, vl) = _zoo_seed_stats(name, mode)
    assert not np.array_equal(ml, mp)
    res = two_sample_check(ml, vl, mp, vp, RUNS)
    print("zoo:" + name, "exact" if mode else "fast", res)


def _variance_ratio(name, mode):
    (_, vp), (_, vl) = _seed_stats(name, mode)
    keep = vl > 0
    return float(np.median(vp[keep] / vl[keep])), float(vp.sum() / vl.sum())


@MODES
@pytest.mark.parametrize("name", ["box", "simple"])
def test_variance_drops_where_lights_are_sampled(name, mode):
    _require_gpu()
    med, tot = _variance_ratio(name, mode)
    print(f"{name} {'exact' if mode else 'fast'}: variance plain / light sampling, median {med:.3f}, sum {tot:.3f}")
    assert med >= 2.2, (med, tot)


@MODES
def test_variance_of_box_mirror_is_reported(mode):
    _require_gpu()
    med, tot = _variance_ratio("box_mirror", mode)
    print(f"box_mirror {'exact' if mode else 'fast'}: variance plain / light sampling, median {med:.3f}, sum {tot:.3f} "
          "(mirror walls: the step never runs)")


# ---- 3: the double definition ------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _f64_frame(name, W, H, n):
    with ptgpu.Context(*_scene(name, W, H)) as ctx:
        img = _frame(ctx, ptgpu.make_params(W, H, n, 2, SEED, flags=ptgpu.FLAG_REFERENCE_F64 | LS))
    img.setflags(write=False)
    return img


@MODES
@pytest.mark.parametrize("name,W,H,n", [("box", 64, 48, 64), ("simple", 64, 48, 64), ("synthetic:300", 32, 18, 128)]
                         + [(f"zoo:{k}", zoo.W, zoo.H, 64) for k in zoo.CASES]
                         + [(k, zoo.W, zoo.H, 64) for k in tie_scenes.LAMPS])
def test_fp32_against_the_double_definition(name, W, H, n, mode):
    _require_gpu()
    ref = _f64_frame(name, W, H, n).astype(np.float64)
    with ptgpu.Context(*_scene(name, W, H)) as ctx:
        if name == "zoo:through_ceiling":  # (the lamp through the ceiling leaves box mode and the wall pairs on)
            info = ctx.launch_info(ptgpu.make_params(W, H, n, 2, SEED, flags=EXACT | LS))
            assert info["box_mode"] == 1 and info["wall_pairs"] == 3, info
        img = _frame(ctx, ptgpu.make_params(W, H, n, 2, SEED, flags=mode | LS)).astype(np.float64)
        plain = _frame(ctx, ptgpu.make_params(W, H, n, 2, SEED, flags=mode)).astype(np.float64)
    rmse = float(np.sqrt(((img - ref) ** 2).mean()))
    print(f"{name} {'exact' if mode else 'fast'}: per-pixel RMSE vs REFERENCE_F64 | LIGHT_SAMPLING {rmse:.3e} "
          f"(the plain frame differs by {float(np.sqrt(((plain - ref) ** 2).mean())):.3e})")
    assert rmse < 1e-3
    assert not np.array_equal(img, plain)  # (the flag did something)


# ---- 4, 8: invariances ---------------------------------------------------------------
# name, W, H, n, nsub
SHAPES = {
    "box": ("box", 32, 24, 16, 2),
    "box_partial_group": ("box", 40, 12, 4, 2),  # 2.5 pixel groups of 16
    "box_nsub3": ("box", 14, 6, 4, 3),           # 7 pixels x 9 sub-pixels: 63 slots
    "bvh": ("synthetic:300", 32, 18, 4, 2),      # the BVH kernel
    "sixteen": ("zoo:sixteen", 32, 24, 4, 2),       # L = 16, every material
    "glass_lamp": ("zoo:glass_lamp", 32, 24, 4, 2),  # hit points inside a light
    "bvh_lights": ("zoo:bvh_lights", 32, 24, 4, 2),  # L = 5 on the BVH kernel
}


def _params(shape, flags, **kw):
    name, W, H, n, nsub = SHAPES[shape]
    return ptgpu.make_params(W, H, n, nsub, SEED, kw.pop("band_rows", 1), flags=flags, **kw)


@MODES
@pytest.mark.parametrize("shape", list(SHAPES))
def test_frame_does_not_depend_on_how_it_is_cut(shape, mode):
    _require_gpu()
    name, W, H, n, nsub = SHAPES[shape]
    k = min(5, n - 1)  # the progressive split [0, 5) + [5, n); n = 4: [0, 3) + [3, 4)
    with ptgpu.Context(*_scene(name, W, H)) as ctx:
        seg = torch.zeros(4, dtype=torch.int64, device="cuda")
        one = _frame(ctx, _params(shape, mode | LS | ptgpu.FLAG_COUNT_NONFINITE), seg)
        counters = seg.cpu().tolist()
        assert counters[0] > W * H * nsub * nsub * n and counters[3] == 0, counters  # test 8
        assert np.array_equal(one, _frame(ctx, _params(shape, mode | LS)))  # (the counting kernel)
        assert not np.array_equal(one, _frame(ctx, _params(shape, mode)))   # (the flag did something)
        for chunk in (1, 3):
            assert np.array_equal(one, _frame(ctx, _params(shape, mode | LS, chunk_samples=chunk))), chunk
        whole = np.full((H, W, 3), -7.0, dtype=np.float32)
        for rank in range(3):
            p = _params(shape, mode | LS, band_rows=2, shard_rank=rank, shard_count=3)
            rows = ptgpu.slab_to_image_rows(H, 2, rank, 3)
            whole[rows[rows >= 0]] = _frame(ctx, p)[rows >= 0]
        assert np.array_equal(one, whole)
        for flags in (mode | LS, mode | LS | MOM):
            p = _params(shape, flags)
            ctx.reset_accumulation(p)
            ctx.accumulate(p, 0, k)
            ctx.accumulate(p, k, n)
            assert np.array_equal(one, _resolved(ctx, p, n)), flags
        ctx.reset_accumulation(_params(shape, mode | LS))


# ---- 5: the pool against the one-thread trace -------------------------------------------
def _quant(c):
    """tests/test_gpu_noise.py's restatement of quant(): NaN and negative -> 0, above 2^30 -> 2^30, trunc(c 2^32)."""
    c = np.where(c >= 0, c, np.float32(0))
    c = np.minimum(c, np.float32(2.0 ** 30)).astype(np.float32)
    return (c.astype(np.float64) * 2.0 ** 32).astype(np.uint64)  # exact in double, then truncated


@MODES
@pytest.mark.parametrize("name,W,H,n", [("box", 16, 12, 4), ("synthetic:300", 16, 9, 2)]
                         + [(f"zoo:{k}", 16, 12, 2) for k in ("three", "sixteen", "glass_lamp", "permuted",
                                                              "bvh_lights")]
                         + [(k, 16, 12, 2) for k in tie_scenes.LAMPS])
def test_pool_kernel_equals_the_trace_kernel(name, W, H, n, mode):
    _require_gpu()
    nsub = 2
    p = ptgpu.make_params(W, H, n, nsub, SEED, 1, flags=mode | LS | MOM)
    # coords x, y (from the bottom), sx, sy, sample in the order of S1's [row, x, sub, (sample)]
    row, x, sy, sx, s = np.meshgrid(np.arange(H), np.arange(W), np.arange(nsub), np.arange(nsub), np.arange(n),
                                    indexing="ij")
    coords = np.stack([x, H - 1 - row, sx, sy, s], axis=-1).reshape(-1, 5).astype(np.int32)
    with ptgpu.Context(*_scene(name, W, H)) as ctx:
        ctx.reset_accumulation(p)
        ctx.accumulate(p, 0, n)
        s1 = _s1(ctx, p)
        E, segs = ctx.trace_samples(torch.from_numpy(coords).cuda(), p)
        torch.cuda.synchronize()
        E0, segs0 = ctx.trace_samples(torch.from_numpy(coords).cuda(), ptgpu.make_params(W, H, n, nsub, SEED, 1,
                                                                                         flags=mode))
        torch.cuda.synchronize()
        ctx.reset_accumulation(p)
    E = E.cpu().numpy().reshape(H, W, nsub * nsub, n, 3)
    assert np.array_equal(_quant(E).sum(axis=3, dtype=np.uint64), s1)
    assert int(segs.sum()) > int(segs0.sum())  # shadow segments are scans
    assert not np.array_equal(E.reshape(-1, 3), E0.cpu().numpy())


# ---- 9: per path against the oracle ---------------------------------------------------------
@pytest.mark.parametrize("name", oracle_ls.PATH_SCENES)
def test_exact_mode_paths_against_the_oracle(name):
    """trace_samples in exact mode against the oracle's per-path double, 12,288
    paths (32x24, 4 sub-pixels, 4 samples).  The tolerance comes from the
    reference: the definition's numpy restatement run in float32
    (tests/light_ref.py) differs from the oracle by at most `err` over the
    paths whose segment counts agree; the kernel may differ by 4 times that
    (the margin of test_features_against_numpy_first_hit: another fp32
    formulation of the same definition, not the same rounding), and at most
    0.5 % of its paths may end with another segment count.  Float32
    restatement, measured on the CPU: sixteen err 7.96e-2, 0.065 % of the
    paths differ; dome 5.72e-3, 0.057 %.  The kernel's figures are printed."""
    _require_gpu()
    coords, E, segs, _, _ = oracle_ls.per_path_reference(name)
    err, share = oracle_ls.float32_yardstick(name)
    assert share <= 0.005  # the reference alone (also tests/test_oracle_light_sampling.py, on the CPU)
    p = ptgpu.make_params(zoo.W, zoo.H, oracle_ls.PATH_SAMPLES, zoo.NSUB, SEED, 1, flags=EXACT | LS)
    with ptgpu.Context(*_scene("zoo:" + name, zoo.W, zoo.H)) as ctx:
        got, gsegs = ctx.trace_samples(torch.from_numpy(coords.copy()).cuda(), p)
        torch.cuda.synchronize()
    got, gsegs = got.cpu().numpy().astype(np.float64), gsegs.cpu().numpy()
    agree = gsegs == segs
    d = float(np.abs(got - E)[agree].max())
    print(f"zoo:{name}: kernel against the oracle per path: max |diff| {d:.3e} where the segment counts agree "
          f"(float32 restatement {err:.3e}, bound 4x), {100 * (1 - agree.mean()):.3f} % of {len(segs)} paths differ "
          f"in the count (restatement {100 * share:.3f} %)")
    assert 1.0 - agree.mean() <= 0.005
    assert d <= 4.0 * err, (d, err)


# ---- 6: adaptive ------------------------------------------------------------------------
@MODES
def test_adaptive_pixels_equal_the_one_shot_frame_at_their_count(mode):
    _require_gpu()
    name, W, H, nsub = "box", 32, 24, 2
    p = ptgpu.make_params(W, H, 16, nsub, SEED, 1, flags=mode | LS)
    checker = ((np.arange(W)[None, :] + np.arange(H)[:, None]) % 2).astype(np.uint8)
    with ptgpu.Context(*_scene(name, W, H)) as ctx:
        ctx.reset_accumulation(p)
        ctx.set_active_mask(p)
        ctx.accumulate_active(p, 2)
        ctx.set_active_mask(p, torch.from_numpy(checker.reshape(-1).copy()).cuda())
        ctx.accumulate_active(p, 3)
        counts = torch.full((H * W,), -1, dtype=torch.int32, device="cuda")
        ctx.read_sample_counts(p, counts)
        img = torch.full((H * W * 3,), -7.0, dtype=torch.float32, device="cuda")
        ctx.resolve_active(img, p)
        torch.cuda.synchronize()
        counts = counts.cpu().numpy().reshape(H, W)
        img = img.cpu().numpy().reshape(H, W, 3)
        assert np.array_equal(counts, 2 + 3 * checker.astype(np.int32))
        ctx.reset_accumulation(p)
        for n in (2, 5):
            one = _frame(ctx, ptgpu.make_params(W, H, n, nsub, SEED, 1, flags=mode | LS))
            assert np.array_equal(img[counts == n], one[counts == n]), n
            plain = _frame(ctx, ptgpu.make_params(W, H, n, nsub, SEED, 1, flags=mode))
            assert not np.array_equal(img[counts == n], plain[counts == n]), n


# ---- too many lights: refused where the flag is given, by every kind of entry point ---------------
def test_seventeen_lights_are_refused_with_the_flag_only():
    _require_gpu()
    W, H = 16, 12
    scn = ptgpu.make_scene("box", W, H)
    scn.spheres = scn.spheres[:5] + [
        ptgpu.sphere(0.02, (-0.35 + 0.04 * i, 0.0, -0.5), (2.0, 2.0, 2.0), (0.5, 0.5, 0.5),
                     ptgpu.reflection_type.diffuse) for i in range(17)]
    cam = ptgpu.camera.with_config(scn.camera_parameters)
    plain, flagged = (ptgpu.make_params(W, H, 2, 2, SEED, flags=f) for f in (0, LS))
    unsupported = r"\(-4\).*17 small emitters"
    with ptgpu.Context(scn, cam) as ctx:
        assert _frame(ctx, plain).max() > 0
        with pytest.raises(ptgpu.PtgError, match=unsupported):
            _frame(ctx, flagged)
        with pytest.raises(ptgpu.PtgError, match=unsupported):
            ctx.accumulate(flagged, 0, 2)
        with pytest.raises(ptgpu.PtgError, match=unsupported):
            ctx.set_active_mask(flagged)
        with pytest.raises(ptgpu.PtgError, match=unsupported):
            ctx.trace_samples(torch.zeros((1, 5), dtype=torch.int32, device="cuda"), flagged)
    with pytest.raises(ptgpu.PtgError, match=unsupported):
        ptgpu.render(scn, cam, np.zeros((H * W, 3)), W, H, 2, flags=LS)


# ---- 7: no lights ---------------------------------------------------------------------------
@MODES
def test_no_lights_no_change(mode):
    _require_gpu()
    W, H = 32, 24
    scn = ptgpu.make_scene("box", W, H)
    d = ptgpu.reflection_type.diffuse
    scn.spheres = [ptgpu.sphere(0.2, (-0.15, 0.0, -0.5), (0.0, 0.0, 0.0), (0.7, 0.4, 0.3), d),
                   ptgpu.sphere(0.15, (0.2, -0.05, -0.4), (0.0, 0.0, 0.0), (0.3, 0.6, 0.8), d)]
    cam = ptgpu.camera.with_config(scn.camera_parameters)
    assert ptgpu.light_list(scn, cam) == []
    with ptgpu.Context(scn, cam) as ctx:
        plain = _frame(ctx, ptgpu.make_params(W, H, 8, 2, SEED, flags=mode))
        flagged = _frame(ctx, ptgpu.make_params(W, H, 8, 2, SEED, flags=mode | LS))
    assert plain.std() > 0.01  # (the spheres are in view, lit by the sky)
    assert np.array_equal(plain, flagged)
