"""Radiance outside [0, 2^30] on every kernel that accumulates it.

include/ptgpu.h ("Sample accumulation", PTG_FLAG_COUNT_NONFINITE,
PTG_FLAG_MOMENTS): per path and channel q(c) = trunc(cl(c) 2^32), cl sending
NaN and negative values to 0 and values above 2^30 to 2^30 (exactly 2^30 is in
range); S2 += q(cl(c) cl(c)); the fourth counter counts the paths with a
clipped component; the sub-pixel mean is clamped to [0, 1].  The other GPU
modules run this code with in-range radiance only.  Here the scenes of
tests/range_scenes.py feed it NaN, +inf, negative values, values above, at and
just below 2^30, squares above 2^30 and sums of a few units of 2^-32;
tests/test_radiance_range_host.py checks on the oracle alone that they do, that
the numpy restatement used here (tests/test_gpu_noise.py: _cl, _quant, _sums,
_noise_ref; tests/test_gpu_adaptive.py: _resolve_at) equals the oracle's own
accumulation on them, and that no u64 sum of these frames wraps.

A  raw sums, one-shot image, segments and counter of every scene (exact mode)
B  every epilogue: in-wave, HBM accumulation + resolve_kernel, cooperative,
   shards, the BVH kernel
C  the fast and the light-sampling kernels: render kernel == trace kernel, the
   trace kernel's floats (NaN and inf included) quantised in numpy
D  noise_kernel on clipped sums
E  gather_kernel (adaptive passes)
F  PTG_FLAG_REFERENCE_F64, which does not clip, against the oracle's Mode A/xs

Every comparison is exact, but for D's var and rho, which use
tests/test_gpu_noise.py's tolerance formulas unchanged.  Where a sum holds a
sample clipped to 2^30 that var formula is wide (its second term follows
m1^2 ~ 2^60, the size of the cancelling difference); rho and the integer
statistics are what bind there.
"""
import functools
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import ptgpu  # noqa: E402
import pyoracle as po  # noqa: E402
import range_scenes as rs  # noqa: E402
import shape_scenes as ss  # noqa: E402
from test_gpu_adaptive import _counts, _image, _moments, _resolve_at, _select  # noqa: E402
from test_gpu_fast_paths import check_render_equals_trace  # noqa: E402
from test_gpu_frame_shapes import _progressive, _slab  # noqa: E402
from test_gpu_noise import (EXACT, FLOOR, MOM, SEED, _accumulate, _cl, _noise, _noise_ref,  # noqa: E402
                            _paths_and_segments, _quant, _read, _require_gpu, _scene, _stats_of, _sums)
from test_gpu_ref64 import check_matches_mode_a_xs  # noqa: E402
from test_radiance_range_host import COOP, FRAMES, IDS, coop_rows  # noqa: E402

NT = max(1, min(16, int(os.environ.get("OMP_NUM_THREADS", "8"))))
COUNT = ptgpu.FLAG_COUNT_TESTS | ptgpu.FLAG_COUNT_NONFINITE
LS = ptgpu.FLAG_LIGHT_SAMPLING


@functools.lru_cache(maxsize=None)
def _ref(name, W, H, n, nsub):
    """The oracle's frame restated in numpy: paths E, S1, S2, image, segments, clipped paths (read-only)."""
    E, segs = _paths_and_segments(name, W, H, n, nsub)
    S1, S2 = _sums(E, 0, n)
    pix = _resolve_at(S1, np.full((H, W), n), nsub)
    for a in (S1, S2, pix):
        a.setflags(write=False)
    return E, S1, S2, pix, int(segs.sum()), int(rs.clipped(E).sum())


def _passes(n):
    return [(0, 1), (1, n)]


def _same(a, b):
    return a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- A. raw sums and counter, exact mode, every scene -------------------------------
@pytest.mark.parametrize("frame", [f for f in FRAMES if f[0] != "over_ls"], ids=[i for i in IDS if "over_ls" not in i])
def test_sums_image_segments_and_counter(frame):
    _require_gpu()
    name, W, H, n, nsub = frame
    E, S1, S2, pix, rsegs, rbad = _ref(*frame)
    p = ptgpu.make_params(W, H, n, nsub, SEED, flags=EXACT | MOM)
    shot = ptgpu.make_params(W, H, n, nsub, SEED, flags=EXACT | COUNT)
    cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
    with ptgpu.Context(*_scene(name, W, H)) as ctx:
        assert ctx.launch_info(shot)["bvh"] == int(name == "bvh_mix")
        _accumulate(ctx, p, _passes(n))
        g1, g2 = _read(ctx, p)
        out = torch.full((H * W * 3,), -7.0, dtype=torch.float32, device="cuda")
        ctx.render_device(out, shot, cnt)
        torch.cuda.synchronize()
    img = out.cpu().numpy().reshape(H, W, 3)
    segs, _, _, bad = cnt.cpu().tolist()
    print(f"{name} {W}x{H}x{n} nsub {nsub}: S1 differs at {int((g1 != S1).sum())}, S2 at {int((g2 != S2).sum())} of "
          f"{S1.size} sums, image at {int((img != pix).sum())} values; segments {segs} / {rsegs}, counter {bad} / {rbad}")
    assert np.array_equal(g1, S1)
    assert np.array_equal(g2, S2)
    assert _same(img, pix)
    assert segs == rsegs
    assert bad == rbad
    if any(k in rs.CLIPPED for k in rs.CLASSES[name]):
        assert bad > 0
    masks = rs.classes(E)
    if name == "edge":  # the paths above 2^30 ...
        assert bad == int(masks["high"].sum()) > 0
    if name == "edge_in":  # ... not those at it
        assert bad == 0 and int(masks["edge"].sum()) > 0
        assert int((S1 >= 1 << 62).sum()) > 0  # sums hold the unclipped 2^30
    if name == "cap":
        assert segs == 100 * W * H * nsub * nsub * n and bad == 0
    if name == "s2sat":  # S2's own clip: a square above 2^30 adds exactly 2^62
        assert bad == 0 and int((S2 >= 1 << 62).sum()) > 0 and int(S1.max()) < 1 << 62
    if name == "tiny":
        assert 0 < int(S1.max()) <= 3 * n and not S2.any()


# ---- B. every epilogue and kernel template ----------------------------------------------
@pytest.mark.parametrize("name", ["over", "neg", "nanwalls"])
def test_every_epilogue_of_the_linear_kernel(name):
    """The kernel without counters: auto chunk (HBM accumulation + resolve_kernel), one unit per
    pixel group (in-wave resolve), one sample per unit, progressive passes, two shards of 3-row bands."""
    _require_gpu()
    W, H, n, nsub = rs.BASE
    _, _, _, pix, _, _ = _ref(name, W, H, n, nsub)

    def params(chunk=0, rank=0, count=1, band=1):
        return ptgpu.make_params(W, H, n, nsub, SEED, band, rank, count, chunk, flags=EXACT)

    with ptgpu.Context(*_scene(name, W, H)) as ctx:
        auto, whole = ctx.launch_info(params()), ctx.launch_info(params(chunk=n))
        assert (auto["resolve_pass"], whole["resolve_pass"]) == (1, 0)  # both routes are taken
        frames = {"auto": _slab(ctx, params())[0], "in-wave": _slab(ctx, params(chunk=n))[0],
                  "chunk 1": _slab(ctx, params(chunk=1))[0], "progressive": _progressive(ctx, params(), _passes(n))}
        shards = []
        for rank in range(2):
            for chunk in (0, n):
                shards.append((rank, chunk, _slab(ctx, params(chunk, rank, 2, 3))[0]))
            shards.append((rank, "progressive", _progressive(ctx, params(0, rank, 2, 3), _passes(n))))
    for key, img in frames.items():
        assert _same(img, pix), key
    for rank, key, slab in shards:
        m = ptgpu.slab_to_image_rows(H, 3, rank, 2)
        assert _same(slab[m >= 0], pix[m[m >= 0]]), (rank, key)
        assert (slab[m < 0] == -7.0).all(), (rank, key)


def test_cooperative_epilogue_on_negative_radiance():
    """tests/test_gpu_frame_shapes.py's lin_nsub8_coop frame (256x160, nsub 8, 8 samples: one
    pixel per wave, LDS-reduced tail) on scene neg, which has no sample clipped to 2^30, so 8
    samples cannot wrap a sum (tests/test_radiance_range_host.py)."""
    _require_gpu()
    name, W, H, n, nsub = COOP
    plan, rows = coop_rows()
    assert (plan["n_levels"], plan["needs_resolve"]) == (2, 0)
    scn, cam = _scene(name, W, H)
    sp, ca = ss.oracle_arrays(scn, cam)
    p = ptgpu.make_params(W, H, n, nsub, SEED, flags=EXACT)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    with ptgpu.Context(scn, cam) as ctx:
        info = ctx.launch_info(p)
        assert (info["bvh"], info["levels"], info["resolve_pass"]) == (0, 2, 0), \
            f"the plan on a device of {cus} CUs is not of the kind under test: {info}"
        auto, _ = _slab(ctx, p)
        prog = _progressive(ctx, p, [(0, 3), (3, n)])
    assert _same(auto, prog)
    for j in rows:
        y = H - 1 - j
        ref, _ = po.render_xs_rect(sp, ca, W, H, n, nsub, SEED, rows=(y, y + 1, 1), nthreads=NT)
        print(f"neg coop: row {j}: oracle mean {ref[j].mean():.5f}, differs at {int((auto[j] != ref[j]).sum())} values")
        assert ref[j].mean() > 0, j
        assert _same(auto[j], ref[j]), j


def test_bvh_kernel_in_wave_resolve():
    """bvh_mix through resolve_kernel is item A's frame; here one unit holds every sample."""
    _require_gpu()
    frame = ("bvh_mix",) + rs.BVH_BASE
    name, W, H, n, nsub = frame
    _, _, _, pix, rsegs, rbad = _ref(*frame)
    with ptgpu.Context(*_scene(name, W, H)) as ctx:
        whole = ptgpu.make_params(W, H, n, nsub, SEED, chunk_samples=n, flags=EXACT)
        info = ctx.launch_info(whole)
        assert (info["bvh"], info["resolve_pass"]) == (1, 0)
        img, _ = _slab(ctx, whole)
        counting = ptgpu.make_params(W, H, n, nsub, SEED, chunk_samples=n, flags=EXACT | COUNT)
        cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
        out = torch.full((H * W * 3,), -7.0, dtype=torch.float32, device="cuda")
        ctx.render_device(out, counting, cnt)
        torch.cuda.synchronize()
    assert _same(img, pix)
    assert _same(out.cpu().numpy().reshape(H, W, 3), pix)
    assert (cnt[0].item(), cnt[3].item()) == (rsegs, rbad) and rbad > 0


# ---- C. fast mode and light sampling: render kernel == trace kernel ------------------------
C_CASES = [(name, 0) for name in ("over", "edge", "neg", "nanwalls", "bvh_mix")] + \
          [(name, flags) for name in ("over_ls", "bvh_mix") for flags in (LS, LS | EXACT)]


@pytest.mark.parametrize("name,flags", C_CASES, ids=[f"{n}-flags{f}" for n, f in C_CASES])
def test_fast_and_light_sampling_kernels_clip_like_numpy(name, flags):
    """There is no fp32 oracle for these kernels; their trace kernel returns the unquantised
    floats, and the sums, the one-shot image and the counter must be numpy's from those."""
    _require_gpu()
    W, H, n, nsub = rs.base_shape(name)
    if flags & LS:
        assert len(ptgpu.light_list(*_scene(name, W, H))) == 1
    E, counters = check_render_equals_trace(name, W, H, n, nsub, _passes(n), flags=flags, count=True)
    counts = {k: int(v.sum()) for k, v in rs.classes(E).items()}
    bad = int(rs.clipped(E).sum())
    print(f"{name} flags {flags}: classes {counts}, clipped paths {bad}, counter {counters[3]}")
    for k, figure in rs.CLASSES[name].items():  # the oracle test's thresholds halved again
        floor = figure // 2 if name == "bvh_mix" else (figure + 3) // 4
        assert counts[k] >= floor, (k, counts[k], floor)
    assert counters[3] == bad > 0


# ---- D. noise on clipped sums ------------------------------------------------------------------
REL = 0.1


def _check_noise(name, S1, S2, n, nsub, var, rho, stats, floor):
    V, tol, rho_ref = _noise_ref(S1, S2, n, nsub, floor)
    err_v = np.abs(var.astype(np.float64) - V)
    r64 = rho_ref.astype(np.float64)
    err_r = np.abs(rho.astype(np.float64) - r64)
    print(f"{name} floor {floor}: var max err {float(err_v.max()):.3g} (max tol {float(tol.max()):.3g}), rho max err "
          f"{float(err_r.max()):.3g}, max rho {float(r64.max()):.4g}, pixels with rho > 0 {int((r64 > 0).sum())}, "
          f"stats {stats.tolist()}")
    assert np.isfinite(var).all() and np.isfinite(rho).all()
    assert (err_v <= tol).all()
    assert (err_r <= 2.0 ** -20 * r64 + 2.0 ** -19).all()
    assert np.array_equal(stats, _stats_of(rho, REL))
    return r64


@pytest.mark.parametrize("name", ["over", "edge", "s2sat", "nanwalls", "tiny"])
def test_noise_of_clipped_sums(name):
    _require_gpu()
    W, H, n, nsub = rs.BASE
    _, S1, S2, _, _, _ = _ref(name, W, H, n, nsub)
    p = ptgpu.make_params(W, H, n, nsub, SEED, flags=EXACT | MOM)
    with ptgpu.Context(*_scene(name, W, H)) as ctx:
        _accumulate(ctx, p, [(0, n)])
        var, rho, stats = _noise(ctx, p, n, REL)
        low = _noise(ctx, p, n, REL, floor=1e-6) if name == "s2sat" else None
    r64 = _check_noise(name, S1, S2, n, nsub, var, rho, stats, FLOOR)
    assert stats[3] == W * H
    if name == "tiny":  # squares below 2^-32: no variance at all
        assert not var.any() and not rho.any() and stats[0] == 0
    else:
        assert 0 < stats[0] == int((rho.astype(np.float64) > REL).sum()) and r64.max() > REL
    if low is not None:
        _check_noise(name, S1, S2, n, nsub, *low, 1e-6)


def test_statistic_cap_with_a_small_floor():
    """min(rho, 4096) 2^20, the capped statistic, with floor = 1e-6 on s2sat.

    No uniform frame reaches the cap: for clipped samples a_i in [0, 2^30] of one sum,
    (n - 1) v <= m2 <= n m1^2 up to the quantisation, so sqrt(v) is at most sqrt(n / (n - 1))
    times the mean while the mean is below the clamp, and at most 1/2 (the 1/4 cap) against a
    mean of 1 above it: rho stays below 2 whatever the floor (1.73 on this scene, floor 1e-6:
    test_noise_of_clipped_sums prints it).  The only rho above 4096 is the +inf of a pixel with
    fewer than two samples, so the cap is met through ptg_select_active_device: one sample
    everywhere, two more on a checkerboard."""
    _require_gpu()
    name = "s2sat"
    W, H, n, nsub = rs.BASE
    E, _, _, _, _, _ = _ref(name, W, H, n, nsub)
    mask = ((np.arange(W)[None, :] + np.arange(H)[:, None]) % 2).astype(np.uint8)
    counts = np.where(mask != 0, 3, 1)
    p = ptgpu.make_params(W, H, n, nsub, SEED, flags=EXACT)
    with ptgpu.Context(*_scene(name, W, H)) as ctx:
        ctx.reset_accumulation(p)
        ctx.set_active_mask(p)
        ctx.accumulate_active(p, 1)
        ctx.set_active_mask(p, torch.from_numpy(mask.reshape(-1).copy()).cuda())
        ctx.accumulate_active(p, 2)
        rho, st = _select(ctx, p, REL, 0, floor=1e-6)
        assert np.array_equal(_counts(ctx, p), counts)
    S1, S2 = _sums_at(E, counts)
    ref = _noise_ref(S1, S2, np.maximum(counts, 2)[:, :, None, None].astype(np.float64), nsub, 1e-6)[2]
    ref = np.where(counts >= 2, ref, np.float32(np.inf)).astype(np.float64)
    capped = int((ref > 4096).sum())
    assert capped == int((counts < 2).sum()) > 0  # the reference has pixels above the cap
    assert np.array_equal(np.isposinf(rho), counts < 2)
    fin = np.isfinite(ref)
    assert (np.abs(rho[fin].astype(np.float64) - ref[fin]) <= 2.0 ** -20 * ref[fin] + 2.0 ** -19).all()
    assert np.array_equal(st[:4], _stats_of(rho, REL))
    whole = int((np.minimum(rho[fin], np.float32(4096)) * np.float32(2.0 ** 20)).astype(np.uint64).sum())
    assert int(st[1]) == whole + capped * (4096 << 20)  # the capped integer sum


def test_noise_active_at_uniform_counts_equals_noise_device_on_nan_paths():
    _require_gpu()
    name = "nanwalls"
    W, H, n, nsub = rs.BASE
    pa = ptgpu.make_params(W, H, n, nsub, SEED, flags=EXACT)
    pm = ptgpu.make_params(W, H, n, nsub, SEED, flags=EXACT | MOM)
    with ptgpu.Context(*_scene(name, W, H)) as ctx:
        ctx.reset_accumulation(pa)
        ctx.set_active_mask(pa)
        ctx.accumulate_active(pa, n)
        var = torch.full((H * W * 3,), -7.0, dtype=torch.float32, device="cuda")
        rho = torch.full((H * W,), -7.0, dtype=torch.float32, device="cuda")
        ctx.noise_active(pa, FLOOR, var, rho)
        _accumulate(ctx, pm, [(0, n)])
        want_var, want_rho, _ = _noise(ctx, pm, n, REL)
    assert _same(var.cpu().numpy().reshape(H, W, 3), want_var) and _same(rho.cpu().numpy().reshape(H, W), want_rho)
    assert (want_rho > 0).any()


# ---- E. adaptive pass (gather_kernel) ---------------------------------------------------------------
def _sums_at(E, counts):
    """S1, S2 over samples [0, counts[y, x]) of every sub-pixel: uint64 [H, W, nsub^2, 3]."""
    c = _cl(E)
    keep = (np.arange(E.shape[3])[None, None, None, :] < np.asarray(counts)[:, :, None, None])[..., None]
    return ((_quant(c) * keep).sum(axis=3, dtype=np.uint64), (_quant(c * c) * keep).sum(axis=3, dtype=np.uint64))


@pytest.mark.parametrize("name", ["neg", "over"])
def test_adaptive_pass_on_out_of_range_radiance(name):
    """Two samples everywhere, one more on a checkerboard: a pixel with count n_p holds samples
    [0, n_p), and each pass counts the clipped paths among exactly the samples it ran."""
    _require_gpu()
    W, H, n, nsub = rs.BASE
    E, _, _, _, _, _ = _ref(name, W, H, n, nsub)
    mask = ((np.arange(W)[None, :] + np.arange(H)[:, None]) % 2).astype(np.uint8)
    counts = np.where(mask != 0, 3, 2)
    p = ptgpu.make_params(W, H, n, nsub, SEED, flags=EXACT | COUNT)
    first, second = (torch.zeros(4, dtype=torch.int64, device="cuda") for _ in range(2))
    with ptgpu.Context(*_scene(name, W, H)) as ctx:
        ctx.reset_accumulation(p)
        ctx.set_active_mask(p)
        ctx.accumulate_active(p, 2, segments=first)
        ctx.set_active_mask(p, torch.from_numpy(mask.reshape(-1).copy()).cuda())
        ctx.accumulate_active(p, 1, segments=second)
        got = _counts(ctx, p)
        g1, g2 = _moments(ctx, p)
        img = _image(ctx, p)
    assert np.array_equal(got, counts)
    S1, S2 = _sums_at(E, counts)
    assert np.array_equal(g1, S1)
    assert np.array_equal(g2, S2)
    assert _same(img, _resolve_at(S1, counts, nsub))
    bad = rs.clipped(E)  # [H, W, nsub^2, n]
    want_first, want_second = int(bad[:, :, :, :2].sum()), int(bad[mask != 0][:, :, 2].sum())
    print(f"{name}: clipped paths of the passes {first[3].item()} / {want_first}, {second[3].item()} / {want_second}")
    assert first[3].item() == want_first > 0
    assert second[3].item() == want_second > 0


# ---- F. PTG_FLAG_REFERENCE_F64 ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["over", "neg", "nanwalls"])
def test_reference_f64_agrees_with_mode_a_xs_on_what_happens_instead(name):
    """The double path does not clip; tests/test_gpu_ref64.py's criterion, unchanged, and the
    non-finite pixels (if any) at the same positions on both sides."""
    _require_gpu()
    W, H, n, nsub = rs.BASE
    img, ref = check_matches_mode_a_xs(name, W, H, n, nsub, scene=rs.make(name, W, H)[0])
    print(f"{name}: non-finite pixels: GPU {int((~np.isfinite(img)).any(axis=2).sum())}, "
          f"oracle {int((~np.isfinite(ref)).any(axis=2).sum())}")
    assert np.array_equal(np.isnan(img), np.isnan(ref)) and np.array_equal(np.isinf(img), np.isinf(ref))
