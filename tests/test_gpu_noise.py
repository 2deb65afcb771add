"""Per-pixel noise estimates (PTG_FLAG_MOMENTS, ptg_noise_device,
ptg_render_to_noise) against their definition, restated here in numpy.

Per path and channel, c the fp32 radiance component:
    cl(c)  NaN or negative -> 0, above 2^30 -> 2^30        (quant()'s clip)
    q1 = quant(c) = trunc(cl(c) * 2^32),  q2 = quant(cl(c) * cl(c))   (one fp32 multiply)
summed exactly in u64 per (pixel, sub-pixel, channel): S1, S2.  After n >= 2
samples, in double and in (sy, sx) order:
    m1 = S1 2^-32 / n, m2 = S2 2^-32 / n, v = max(0, m2 - m1 m1) / (n - 1)
    V_c = inv_sub2^2 sum_sub min(v, 1/4)         inv_sub2 = (float)1 / nsub^2
    p_c = the pixel value of ptg_resolve_device
    rho = (float)(sqrt((V_r + V_g + V_b) / 3) / max((p_r + p_g + p_b) / 3, floor))

The per-path values come from the oracle (pyoracle.sample_f32, Mode B: the
exact mode's arithmetic), so the raw sums are compared bit for bit.
Tolerances of the slabs (the sums being equal, both sides evaluate the same
double expressions):
    var  2^-22 ref + 2^-40 inv_sub2^2 sum_sub (m2 + m1^2) / (n - 1)
         (float rounding of a double result; rounding of the cancelling difference)
    rho  2^-20 ref + 2^-19                       (the square root of the above)
The stats are integers and are compared exactly with the four values
recomputed from the GPU's own rho slab.
"""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import ptgpu  # noqa: E402
import pyoracle as po  # noqa: E402
import range_scenes  # noqa: E402

SEED = 0x5EED0001
EXACT = ptgpu.FLAG_EXACT_MATH
MOM = ptgpu.FLAG_MOMENTS
FLOOR = 0.01

# name, W, H, n, nsub, passes
CASES = {
    "box": ("box", 32, 24, 16, 2, [(0, 5), (5, 16)]),
    "simple": ("simple", 32, 24, 8, 2, [(0, 8)]),
    "box_partial_group": ("box", 40, 12, 4, 2, [(0, 4)]),  # 40 = 2.5 pixel groups of 16: the nv < 64 path
    "box_nsub3": ("box", 14, 6, 4, 3, [(0, 4)]),  # 7 pixels x 9 sub-pixels: 63 slots
    "bvh": ("synthetic:300", 32, 18, 4, 2, [(0, 4)]),  # > 64 spheres: the BVH kernel
}


def _require_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a visible MI355X")


@functools.lru_cache(maxsize=None)
def _scene(name, W, H):
    if name in range_scenes.CASES:  # (tests/test_gpu_radiance_range.py)
        return range_scenes.make(name, W, H)
    scn = ptgpu.make_scene(name, W, H)
    cam = ptgpu.camera.with_config(scn.camera_parameters)
    return scn, cam


@functools.lru_cache(maxsize=None)
def _paths_and_segments(name, W, H, n, nsub, seed=SEED):
    """Every path from the oracle: its radiance, float32 [H (image row), W, nsub^2, n, 3], and its
    segment count, int64 [H, W, nsub^2, n]; both read-only."""
    scn, cam = _scene(name, W, H)
    sp = np.ascontiguousarray(scn.to_array().view(po.SPHERE_DT))
    ca = np.ascontiguousarray(cam.to_array().view(po.CAMERA_DT))
    E = np.zeros((H, W, nsub * nsub, n, 3), dtype=np.float32)
    segs = np.zeros((H, W, nsub * nsub, n), dtype=np.int64)
    for y in range(H):  # sample_f32's y counts from the bottom: image row H-1-y
        for x in range(W):
            for sy in range(nsub):
                for sx in range(nsub):
                    for s in range(n):
                        j = (H - 1 - y, x, sy * nsub + sx, s)
                        E[j], segs[j] = po.sample_f32(sp, ca, W, H, nsub, seed, x, y, sx, sy, s)
    E.setflags(write=False)
    segs.setflags(write=False)
    return E, segs


def _paths(name, W, H, n, nsub, seed=SEED):
    """Radiance of every path from the oracle: float32 [H (image row), W, nsub^2, n, 3], read-only."""
    return _paths_and_segments(name, W, H, n, nsub, seed)[0]


def _cl(c):
    c = np.where(c >= 0, c, np.float32(0))  # NaN and negative -> 0
    return np.minimum(c, np.float32(2.0 ** 30)).astype(np.float32)


def _quant(c):
    return (_cl(c).astype(np.float64) * 2.0 ** 32).astype(np.uint64)  # exact in double, then truncated


def _sums(E, s0, s1):
    """S1, S2 of samples [s0, s1): uint64 [H, W, nsub^2, 3]."""
    c = _cl(E[:, :, :, s0:s1])
    return _quant(c).sum(axis=3, dtype=np.uint64), _quant(c * c).sum(axis=3, dtype=np.uint64)


def _noise_ref(S1, S2, n, nsub, floor=FLOOR):
    """V [H, W, 3] (double), its tolerance, rho [H, W] (float32) from the definition."""
    m1 = S1.astype(np.float64) * 2.0 ** -32 / n
    m2 = S2.astype(np.float64) * 2.0 ** -32 / n
    v = np.maximum(0.0, m2 - m1 * m1) / (n - 1)
    inv32 = np.float32(1.0) / np.float32(nsub * nsub)
    w = float(inv32) ** 2
    V = np.zeros(S1.shape[:2] + (3,))
    pix = np.zeros(S1.shape[:2] + (3,), dtype=np.float32)
    for j in range(nsub * nsub):  # (sy, sx) order
        V = V + np.minimum(v[:, :, j], 0.25)
        mean = np.clip(m1[:, :, j].astype(np.float32), np.float32(0), np.float32(1))
        # fmaf(mean, inv_sub2, pix): the product of two floats is exact in double
        pix = (mean.astype(np.float64) * float(inv32) + pix.astype(np.float64)).astype(np.float32)
    V = w * V
    tol = 2.0 ** -22 * V + 2.0 ** -40 * w * ((m2 + m1 * m1) / (n - 1)).sum(axis=2)
    sigma = np.sqrt(V.sum(axis=2) / 3.0)
    mu = pix.astype(np.float64).sum(axis=2) / 3.0
    return V, tol, (sigma / np.maximum(mu, floor)).astype(np.float32)


def _params(case, flags=EXACT | MOM, **kw):
    name, W, H, n, nsub, _ = CASES[case]
    return ptgpu.make_params(W, H, n, nsub, kw.pop("seed", SEED), kw.pop("band_rows", 1), flags=flags, **kw)


def _accumulate(ctx, p, passes):
    ctx.reset_accumulation(p)
    for a, b in passes:
        ctx.accumulate(p, a, b)


def _read(ctx, p):
    rows = ptgpu.shard_rows(p.height, p.band_rows, p.shard_count)
    shape = (rows, p.width, p.num_subpixels ** 2, 3)
    s1 = torch.full((int(np.prod(shape)),), -1, dtype=torch.int64, device="cuda")
    s2 = torch.full_like(s1, -1)
    ctx.read_moments(p, s1, s2)
    torch.cuda.synchronize()
    return s1.cpu().numpy().view(np.uint64).reshape(shape), s2.cpu().numpy().view(np.uint64).reshape(shape)


def _noise(ctx, p, n, rel_error, floor=FLOOR):
    """var [rows, W, 3], rho [rows, W], stats [4] of the context's sums after n samples."""
    rows = ptgpu.shard_rows(p.height, p.band_rows, p.shard_count)
    var = torch.full((rows * p.width * 3,), -7.0, dtype=torch.float32, device="cuda")
    rho = torch.full((rows * p.width,), -7.0, dtype=torch.float32, device="cuda")
    stats = torch.zeros(4, dtype=torch.int64, device="cuda")
    ctx.noise(p, n, rel_error, floor, var, rho, stats)
    torch.cuda.synchronize()
    return (var.cpu().numpy().reshape(rows, p.width, 3), rho.cpu().numpy().reshape(rows, p.width),
            stats.cpu().numpy().view(np.uint64))


def _stats_of(rho, rel_error):
    """The four statistics of a rho slab (valid pixels only), as ptg_noise_device defines them."""
    r = rho.reshape(-1)
    fixed = (np.minimum(r, np.float32(4096)) * np.float32(2.0 ** 20)).astype(np.uint64).sum(dtype=np.uint64)
    return np.array([(r.astype(np.float64) > rel_error).sum(), fixed, r.view(np.uint32).max(), r.size],
                    dtype=np.uint64)


# ---- 1. raw moments, bit for bit -------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_raw_moments_bitexact_vs_oracle_paths(case):
    _require_gpu()
    name, W, H, n, nsub, passes = CASES[case]
    S1, S2 = _sums(_paths(name, W, H, n, nsub), 0, n)
    assert (S1 > 0).mean() > 0.05 and (S2 > 0).mean() > 0.05  # the scene is lit (4 samples of box find the lamp rarely)
    p = _params(case)
    with ptgpu.Context(*_scene(name, W, H)) as ctx:
        _accumulate(ctx, p, passes)
        g1, g2 = _read(ctx, p)
    assert np.array_equal(g1, S1)
    assert np.array_equal(g2, S2)


@pytest.mark.parametrize("chunk", [0, 1, 3])
def test_raw_moments_do_not_depend_on_chunking(chunk):
    _require_gpu()
    name, W, H, n, nsub, passes = CASES["box"]
    S1, S2 = _sums(_paths(name, W, H, n, nsub), 0, n)
    p = _params("box", chunk_samples=chunk)
    with ptgpu.Context(*_scene(name, W, H)) as ctx:
        _accumulate(ctx, p, passes)
        g1, g2 = _read(ctx, p)
    assert np.array_equal(g1, S1) and np.array_equal(g2, S2)


def _shard_rows_of(p):
    m = ptgpu.slab_to_image_rows(p.height, p.band_rows, p.shard_rank, p.shard_count)
    return m >= 0, m[m >= 0]


def test_raw_moments_and_stats_of_three_shards():
    """3 shards of 2-row bands: every shard's sums are the frame's rows, and
    the shards' stats add up (max for [2]) to the whole frame's exactly."""
    _require_gpu()
    name, W, H, n, nsub, passes = CASES["box"]
    S1, S2 = _sums(_paths(name, W, H, n, nsub), 0, n)
    rel = 0.2
    with ptgpu.Context(*_scene(name, W, H)) as ctx:
        p = _params("box")
        _accumulate(ctx, p, passes)
        _, rho_whole, whole = _noise(ctx, p, n, rel)
        total = np.zeros(4, dtype=np.uint64)
        for rank in range(3):
            ps = _params("box", band_rows=2, shard_rank=rank, shard_count=3)
            _accumulate(ctx, ps, passes)
            g1, g2 = _read(ctx, ps)
            ok, rows = _shard_rows_of(ps)
            assert np.array_equal(g1[ok], S1[rows]) and np.array_equal(g2[ok], S2[rows])
            assert not g1[~ok].any() and not g2[~ok].any()  # padding rows receive nothing
            _, rho, st = _noise(ctx, ps, n, rel)
            assert np.array_equal(rho[ok], rho_whole[rows])
            assert (rho[~ok] == -7.0).all()  # rows past the image are left untouched
            assert np.array_equal(st, _stats_of(rho[ok], rel))
            total[[0, 1, 3]] += st[[0, 1, 3]]
            total[2] = max(total[2], st[2])
    assert 0 < whole[0] < whole[3] == W * H
    assert np.array_equal(total, whole)


# ---- 2. the slabs against the definition -----------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_slabs_match_the_definition(case):
    _require_gpu()
    name, W, H, n, nsub, passes = CASES[case]
    check_slabs(case, name, W, H, n, nsub, _params(case))


def check_slabs(case, name, W, H, n, nsub, p):
    """The module's criterion on one frame (also used by tests/test_gpu_frame_shapes.py)."""
    E = _paths(name, W, H, n, nsub)
    with ptgpu.Context(*_scene(name, W, H)) as ctx:
        for done in sorted({n, max(2, n // 2 + 1)}):  # the full count and a partial one
            _accumulate(ctx, p, [(0, done)])
            V, tol, rho_ref = _noise_ref(*_sums(E, 0, done), done, nsub)
            rel = float(np.median(rho_ref))
            var, rho, stats = _noise(ctx, p, done, rel)
            err_v = np.abs(var.astype(np.float64) - V)
            print(f"{case} n={done}: var max err/tol {float((err_v / np.maximum(tol, 1e-300)).max()):.3g}, "
                  f"rho max err {float(np.abs(rho.astype(np.float64) - rho_ref).max()):.3g}, "
                  f"median rho {rel:.4g}, stats {stats.tolist()}")
            assert V.max() > 0
            assert (err_v <= tol).all()
            r64 = rho_ref.astype(np.float64)
            assert (np.abs(rho.astype(np.float64) - r64) <= 2.0 ** -20 * r64 + 2.0 ** -19).all()
            assert np.array_equal(stats, _stats_of(rho, rel))
            assert 0 < stats[0] < stats[3] == W * H


def test_noise_outputs_are_optional():
    _require_gpu()
    name, W, H, n, nsub, passes = CASES["box_partial_group"]
    p = _params("box_partial_group")
    with ptgpu.Context(*_scene(name, W, H)) as ctx:
        _accumulate(ctx, p, passes)
        var, rho, stats = _noise(ctx, p, n, 0.1)
        rho_only = torch.zeros(H * W, dtype=torch.float32, device="cuda")
        ctx.noise(p, n, 0.1, FLOOR, rho=rho_only)
        stats_only = torch.zeros(4, dtype=torch.int64, device="cuda")
        ctx.noise(p, n, 0.1, FLOOR, stats=stats_only)
        ctx.noise(p, n, 0.1, FLOOR)  # nothing asked for
        torch.cuda.synchronize()
    assert np.array_equal(rho_only.cpu().numpy().reshape(H, W), rho)
    assert np.array_equal(stats_only.cpu().numpy().view(np.uint64), stats)


# ---- 3. the image is untouched ---------------------------------------------
@pytest.mark.parametrize("mode", [EXACT, 0], ids=["exact", "fast"])
@pytest.mark.parametrize("chunk", [0, 3])
def test_image_untouched_by_the_flag(mode, chunk):
    _require_gpu()
    name, W, H, n, nsub, passes = CASES["box"]
    scn, cam = _scene(name, W, H)
    plain = _params("box", flags=mode, chunk_samples=chunk)
    flagged = _params("box", flags=mode | MOM, chunk_samples=chunk)

    def slab():
        return torch.full((H * W * 3,), -7.0, dtype=torch.float32, device="cuda")

    with ptgpu.Context(scn, cam) as ctx, ptgpu.Context(scn, cam) as fresh:
        a, b, c, d, e = slab(), slab(), slab(), slab(), slab()
        _accumulate(ctx, plain, passes)
        ctx.resolve(a, plain, n)
        _accumulate(ctx, flagged, passes)
        ctx.resolve(b, flagged, n)
        ctx.render_device(c, plain)  # one shot, straight after flagged passes (no reset)
        ctx.render_device(d, flagged)  # the flag has no effect outside accumulate
        fresh.render_device(e, plain)
        torch.cuda.synchronize()
    a, b, c, d, e = (t.cpu().numpy() for t in (a, b, c, d, e))
    assert a.min() >= 0.0 and a.mean() > 0.05
    assert np.array_equal(a, b) and np.array_equal(a, c) and np.array_equal(a, d) and np.array_equal(a, e)


# ---- 4. the estimate means what it says ------------------------------------
def test_predicted_variance_matches_variance_across_seeds():
    """box 32x24x16, seeds 1000..1023, exact mode: the variance of the images
    across the seeds against the mean of the variance slabs.  The oracle gives
    a median ratio of 0.95 here (0.60 on simple, 0.93 on box_mirror); the band
    [0.4, 2.5] is there to catch a wrong factor (n, n - 1, nsub^4), not
    sampling noise."""
    _require_gpu()
    name, W, H, n, nsub, _ = CASES["box"]
    imgs, preds = [], []
    with ptgpu.Context(*_scene(name, W, H)) as ctx:
        for seed in range(1000, 1024):
            p = _params("box", seed=seed)
            _accumulate(ctx, p, [(0, n)])
            out = torch.zeros(H * W * 3, dtype=torch.float32, device="cuda")
            ctx.resolve(out, p, n)
            var, _, _ = _noise(ctx, p, n, 0.0)
            imgs.append(out.cpu().numpy().astype(np.float64))
            preds.append(var.reshape(-1).astype(np.float64))
    emp = np.var(np.stack(imgs), axis=0, ddof=1)
    pred = np.mean(np.stack(preds), axis=0)
    ok = pred > 0
    ratio = float(np.median(emp[ok] / pred[ok]))
    print(f"empirical / predicted variance: median {ratio:.3f} over {int(ok.sum())} pixel-channels")
    assert ok.mean() > 0.9
    assert 0.4 <= ratio <= 2.5


# ---- 5. render until converged ----------------------------------------------
def _plain_render(name, W, H, samples, flags):
    img = np.zeros((H * W, 3))
    ptgpu.render(*_scene(name, W, H), img, W, H, samples, 2, SEED, flags=flags)
    return img


@pytest.mark.parametrize("mode", [EXACT, 0], ids=["exact", "fast"])
def test_render_to_noise_stops_at_the_first_pass_or_never(mode):
    _require_gpu()
    name, W, H, n, nsub, _ = CASES["box"]
    img = np.zeros((H * W, 3))
    rep = ptgpu.render_to_noise(*_scene(name, W, H), img, W, H, n, rel_error=1e9, floor=FLOOR, max_fraction=0.0,
                                min_samples=4, flags=mode)
    assert (rep["samples_done"], rep["passes"], rep["converged"]) == (4, 1, 1)
    assert rep["pass_samples"] == [4] and rep["pass_over"] == [0] and rep["pixels"] == W * H
    assert 0 < rep["mean_rho"] <= rep["max_rho"] < 1e9
    assert np.array_equal(img, _plain_render(name, W, H, 4, mode))

    img = np.zeros((H * W, 3))
    rep = ptgpu.render_to_noise(*_scene(name, W, H), img, W, H, n, rel_error=0.0, floor=FLOOR, max_fraction=0.0,
                                min_samples=4, flags=mode)
    assert (rep["samples_done"], rep["passes"], rep["converged"]) == (n, 3, 0)
    assert rep["pass_samples"] == [4, 8, 16] == ptgpu.noise_schedule(4, n)
    assert all(o > 0 for o in rep["pass_over"]) and rep["pixels_over"] == rep["pass_over"][-1]
    assert np.array_equal(img, _plain_render(name, W, H, n, mode))


MID = ("box", 16, 12, 64, 2)  # passes of 16, 32, 64 samples: below 16 the 1/4 cap decides rho, which then does not fall with n


def _first_pass_within(over, limit):
    return next((k for k, o in enumerate(over) if o <= limit), len(over) - 1)


def test_render_to_noise_stops_at_a_mid_target():
    """A target half way between the 75th percentiles of the numpy rho values
    after 16 and after 32 samples, with max_fraction 1/4: the first pass is
    over the limit, the second within it."""
    _require_gpu()
    name, W, H, n, nsub = MID
    E = _paths(name, W, H, n, nsub)
    ends = ptgpu.noise_schedule(16, n)
    assert ends == [16, 32, 64]
    rhos = [_noise_ref(*_sums(E, 0, e), e, nsub)[2].astype(np.float64) for e in ends]
    target = 0.5 * float(np.quantile(rhos[0], 0.75) + np.quantile(rhos[1], 0.75))
    limit = 0.25 * W * H
    # rho is within 2^-20 rho + 2^-19 of numpy's: a count may differ by the pixels that close to the target
    near = [int((np.abs(r - target) <= 2.0 ** -20 * r + 2.0 ** -19).sum()) for r in rhos]
    over = [int((r > target).sum()) for r in rhos]
    assert over[0] - near[0] > limit >= over[1] + near[1], (over, near, limit)  # the target separates the passes
    img = np.zeros((H * W, 3))
    rep = ptgpu.render_to_noise(*_scene(name, W, H), img, W, H, n, rel_error=target, floor=FLOOR, max_fraction=0.25,
                                min_samples=16, flags=EXACT)
    print(f"target {target:.4f}, numpy counts {over} (near {near}), limit {limit}: {rep}")
    assert (rep["samples_done"], rep["passes"], rep["converged"]) == (32, 2, 1)
    assert rep["pass_samples"] == ends[:2]
    assert rep["pass_over"][0] > limit >= rep["pass_over"][1] == rep["pixels_over"]
    for k in range(2):
        assert abs(rep["pass_over"][k] - over[k]) <= near[k]
    assert rep["max_rho"] <= float(rhos[1].max()) * (1 + 2.0 ** -19) + 2.0 ** -19
    assert np.array_equal(img, _plain_render(name, W, H, 32, EXACT))


# ---- 6. errors ---------------------------------------------------------------
def test_noise_errors():
    _require_gpu()
    name, W, H, n, nsub, passes = CASES["box_partial_group"]
    plain, flagged = _params("box_partial_group", flags=EXACT), _params("box_partial_group")
    with ptgpu.Context(*_scene(name, W, H)) as ctx:
        ctx.reset_accumulation(flagged)
        with pytest.raises(ptgpu.PtgError, match=r"\(-1\).*no PTG_FLAG_MOMENTS pass"):
            ctx.noise(flagged, n, 0.1, FLOOR)
        ctx.accumulate(plain, 0, 2)
        with pytest.raises(ptgpu.PtgError, match=r"\(-1\).*no PTG_FLAG_MOMENTS pass"):
            ctx.noise(flagged, 2, 0.1, FLOOR)
        ctx.accumulate(flagged, 2, 4)  # a mix of unflagged and flagged passes
        with pytest.raises(ptgpu.PtgError, match=r"\(-1\).*without PTG_FLAG_MOMENTS"):
            ctx.noise(flagged, n, 0.1, FLOOR)
        s2 = torch.zeros(H * W * 4 * 3, dtype=torch.int64, device="cuda")
        with pytest.raises(ptgpu.PtgError, match=r"\(-1\).*without PTG_FLAG_MOMENTS"):
            ctx.read_moments(flagged, sumsq=s2)
        _accumulate(ctx, flagged, passes)  # the reset clears the record
        ctx.noise(flagged, n, 0.1, FLOOR)
        with pytest.raises(ptgpu.PtgError, match=r"\(-1\).*samples_done"):
            ctx.noise(flagged, 1, 0.1, FLOOR)
        with pytest.raises(ptgpu.PtgError, match=r"\(-1\).*samples_done"):
            ctx.noise(flagged, n + 1, 0.1, FLOOR)
        with pytest.raises(ptgpu.PtgError, match=r"\(-1\).*floor"):
            ctx.noise(flagged, n, 0.1, 0.0)
        with pytest.raises(ptgpu.PtgError, match=r"\(-4\)"):  # PTG_ERR_UNSUPPORTED, as without the flag
            ctx.accumulate(_params("box_partial_group", flags=MOM | ptgpu.FLAG_REFERENCE_F64), 0, 2)
        ctx.render_device(torch.zeros(H * W * 3, dtype=torch.float32, device="cuda"),
                          _params("box_partial_group", flags=EXACT, chunk_samples=1))  # a one-shot frame through the accumulator
        with pytest.raises(ptgpu.PtgError, match=r"\(-1\).*no PTG_FLAG_MOMENTS pass"):
            ctx.noise(flagged, n, 0.1, FLOOR)
        torch.cuda.synchronize()


# ---- 7. the CLI ----------------------------------------------------------------
def test_cli_noise_target_writes_the_plain_image_of_its_spp(tmp_path):
    _require_gpu()
    cli = os.path.join(os.path.dirname(ptgpu.LIB_PATH), "pt_render_gpu")
    W, H, spp = 64, 48, 256
    # the CLI's defaults: fast mode, floor 0.01, at most 1 % of the pixels over, passes of 64, 128,
    # 256 spp (16, 32, 64 per sub-pixel).  The target: half way between the 99th percentiles of
    # rho after the first two passes; the GPU's own rho slabs say where the run must stop.
    ends, limit, rho = [16, 32, 64], 0.01 * W * H, {}
    p = ptgpu.make_params(W, H, spp // 4, 2, SEED, flags=MOM)
    with ptgpu.Context(*_scene("box", W, H)) as ctx:
        for done in ends:
            _accumulate(ctx, p, [(0, done)])
            rho[done] = _noise(ctx, p, done, 0.0)[1].astype(np.float64)
    target = float(np.float32(0.5 * (np.quantile(rho[16], 0.99) + np.quantile(rho[32], 0.99))))
    over = [int((rho[e] > target).sum()) for e in ends]
    stop = _first_pass_within(over, limit)
    print(f"target {target}, pixels over {over}, limit {limit}: stop at pass {stop + 1}")
    assert stop in (1, 2) and over[stop] <= limit  # not at the first pass, and converged

    def run(*extra):
        out = tmp_path / f"o{len(extra)}.ppm"
        r = subprocess.run([cli, "--scene", "box", "--width", str(W), "--height", str(H), "--format", "p6",
                            "--out", str(out), *extra], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        return out.read_bytes(), r.stderr

    got, err = run("--spp", str(spp), "--noise-target", f"{target:.9g}")
    m = re.search(r"^noise: stopped at (\d+) spp after (\d+) passes, (\d+)/(\d+) pixels above (\S+), max (\S+), "
                  r"mean (\S+), converged ([01])$", err, re.M)
    assert m, err
    assert (int(m.group(1)), int(m.group(2)), int(m.group(3)), int(m.group(4)), int(m.group(8))) == \
        (4 * ends[stop], stop + 1, over[stop], W * H, 1)
    assert float(m.group(5)) == pytest.approx(target, rel=1e-5)  # (printed with 6 digits)
    plain, _ = run("--spp", m.group(1))
    assert got == plain and len(got) == len(f"P6\n{W} {H}\n255\n") + W * H * 3
    r = subprocess.run([cli, "--noise-target", "0.1", "--devices", "0,1", "--width", "8", "--height", "8"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "one device" in r.stderr
