"""Followed features on the GPU (include/ptgpu.h "denoising",
ptg_features_follow_device; DESIGN.md "Denoising"):

1. max_bounces = 0 is ptg_features_device, 2. nothing to follow, 3. against
the float64 restatement tests/follow_ref.py, 4. independence of everything
random and of the accumulation state, 5. every driver with follow_bounces,
6. acceptance.  "Equal" means bit for bit.
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import follow_ref  # noqa: E402
import follow_scenes  # noqa: E402
import ptgpu  # noqa: E402
from follow_scenes import BOUNCES, GPU_CASES, MARGIN, MAX_EXCLUDED, scene_and_camera  # noqa: E402

DEV = "cuda:0"
EXACT, LS, MOM = ptgpu.FLAG_EXACT_MATH, ptgpu.FLAG_LIGHT_SAMPLING, ptgpu.FLAG_MOMENTS
SIZES = dict((n, (W, H)) for n, W, H in GPU_CASES)


def _feat(ctx, p, follow=None, fill=None):
    rows = ptgpu.shard_rows(p.height, p.band_rows, p.shard_count)
    out = None
    if fill is not None:
        out = torch.full((rows, p.width, 12), fill, dtype=torch.float32, device=DEV)
    out = ctx.features(p, out, follow_bounces=follow)
    torch.cuda.synchronize()
    return out.cpu().numpy()


# ---- 1. B = 0 is the old kernel -------------------------------------------------------------
@pytest.mark.parametrize("nsub", [1, 2])
@pytest.mark.parametrize("name", ["box", "box_mirror", "simple", "synthetic:300"])
def test_no_bounce_equals_the_first_hit_kernel(name, nsub):
    W, H = SIZES[name]
    scn, cam = scene_and_camera(name, W, H)
    with ptgpu.Context(scn, cam, device=0) as ctx:
        p = ptgpu.make_params(W, H, 4, nsub)
        want = _feat(ctx, p)
        assert np.array_equal(_feat(ctx, p, 0), want) and (want[..., 7] > 0).any()
        # 33x21 as 3 shards in bands of 2: slabs of 8 rows, 24 for 21 -- rows past the image stay untouched
        past = 0
        whole = _feat(ctx, ptgpu.make_params(33, 21, 4, nsub))
        assert np.array_equal(_feat(ctx, ptgpu.make_params(33, 21, 4, nsub), 0), whole)
        for rank in range(3):
            q = ptgpu.make_params(33, 21, 4, nsub, band_rows=2, shard_rank=rank, shard_count=3)
            old, new = _feat(ctx, q, None, -7.0), _feat(ctx, q, 0, -7.0)
            rows = ptgpu.slab_to_image_rows(21, 2, rank, 3)
            ok = rows >= 0
            assert np.array_equal(new, old) and np.array_equal(new[ok], whole[rows[ok]])
            assert (new[~ok] == -7.0).all()
            # ... and a followed slab holds the followed frame's rows
            f4 = _feat(ctx, q, 4, -7.0)
            assert np.array_equal(f4[ok], _feat(ctx, ptgpu.make_params(33, 21, 4, nsub), 4)[rows[ok]])
            assert (f4[~ok] == -7.0).all()
            past += int((~ok).sum())
        assert past == 3


# ---- 2. nothing to follow ---------------------------------------------------------------------
@pytest.mark.parametrize("nsub", [1, 2])
def test_all_diffuse_scene_has_nothing_to_follow(nsub):
    W, H = 64, 48
    scn, cam = scene_and_camera("box_all_diffuse", W, H)
    with ptgpu.Context(scn, cam, device=0) as ctx:
        p = ptgpu.make_params(W, H, 4, nsub)
        assert np.array_equal(_feat(ctx, p, 8), _feat(ctx, p, 0))
    scn, cam = scene_and_camera("box", W, H)  # (with the mirror and the glass ball it differs)
    with ptgpu.Context(scn, cam, device=0) as ctx:
        a, b = _feat(ctx, p, 8), _feat(ctx, p, 0)
        assert not np.array_equal(a, b) and a[..., 11].max() >= 1 and (b[..., 11] == 0).all()


# ---- 3. against the float64 restatement -----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reference(name, nsub, B):
    """(float64 frame, pixels kept, the float32 restatement's differences) -- read-only."""
    W, H = SIZES[name]
    scn, cam = scene_and_camera(name, W, H)
    f64, _, _, margin = follow_ref.follow(scn, cam, W, H, nsub, B, np.float64)
    f32, _, _, _ = follow_ref.follow(scn, cam, W, H, nsub, B, np.float32)
    keep = (margin >= MARGIN).all(-1)
    f64.setflags(write=False)
    keep.setflags(write=False)
    return f64, keep, follow_ref.followed_differences(f32, f64, keep)


# The float32 restatement's largest differences from float64 over the kept pixels, measured on the CPU
# (|dn|, |dz| / z, |dP| / |P|, |d albedo|); the bound on the kernel is 4 times the figure of its own case
# (scene, nsub, B), computed in the test.  At B = 1 and B = 8, nsub 1 / nsub 2 (DESIGN.md "Denoising" has
# every case, with the share of excluded pixels):
#   box            B 1: n 2.9e-4 / 6.4e-5  z 2.3e-5 / 5.3e-5  P 1.2e-4 / 9.6e-5  a 4.8e-8 / 1.4e-7
#                  B 8: n 2.9e-4 / 6.4e-5  z 1.2e-4 / 5.3e-5  P 5.1e-4 / 9.6e-5  a 4.8e-8 / 1.4e-7
#   simple         B 1: n 6.9e-5 / 9.7e-6  z 5.2e-4 / 6.0e-5  P 6.4e-4 / 1.2e-4  a 3.9e-8 / 6.2e-8
#                  B 8: n 6.9e-5 / 1.6e-5  z 5.2e-4 / 6.0e-5  P 6.4e-4 / 1.2e-4  a 1.9e-8 / 4.8e-8
#   box_mirror     B 1: n 8.6e-5 / 7.1e-5  z 1.4e-5 / 1.0e-5  P 8.5e-5 / 5.6e-5  a 8.1e-8 / 1.3e-7
#                  B 8: n 4.1e-3 / 2.4e-3  z 1.2e-3 / 2.6e-3  P 6.7e-3 / 8.8e-3  a 2.3e-7 / 2.3e-7
#   synthetic:300  B 1: n 8.2e-5 / 2.5e-5  z 7.2e-4 / 2.2e-4  P 1.1e-3 / 9.6e-5  a 4.5e-8 / 4.5e-8
#                  B 8: n 8.2e-5 / 2.5e-5  z 7.2e-4 / 2.2e-4  P 1.1e-3 / 9.6e-5  a 2.8e-8 / 4.0e-8
#   mirror_back    B 1: n 2.9e-4 / 6.4e-5  z 2.3e-5 / 5.3e-5  P 1.2e-4 / 9.6e-5  a 4.8e-8 / 1.5e-7
#                  B 8: n 2.9e-4 / 6.4e-5  z 1.4e-4 / 6.5e-5  P 8.6e-4 / 3.6e-4  a 4.8e-8 / 1.5e-7
# (a chain of eight mirror bounces in box_mirror multiplies the first hit's rounding: every curved bounce on
# the mirror ball spreads it.)  Excluded pixels: at most 1.9 % (box_mirror, nsub 2, B = 8).
@pytest.mark.parametrize("B", BOUNCES)
@pytest.mark.parametrize("nsub", [1, 2])
@pytest.mark.parametrize("name", [n for n, _, _ in GPU_CASES])
def test_followed_features_against_the_float64_restatement(name, nsub, B):
    W, H = SIZES[name]
    scn, cam = scene_and_camera(name, W, H)
    f64, keep, ref = _reference(name, nsub, B)
    with ptgpu.Context(scn, cam, device=0) as ctx:
        got = _feat(ctx, ptgpu.make_params(W, H, 4, nsub), B)
    d = follow_ref.followed_differences(got, f64, keep)
    print(f"{name} nsub {nsub} B {B}: excluded {1 - keep.mean():.4f}, followed pixels "
          f"{int((f64[..., 11] > 0).sum())}, float32 restatement {ref}, kernel {d}")
    assert 1 - keep.mean() <= MAX_EXCLUDED
    assert np.array_equal(got[..., 7][keep], f64[..., 7][keep].astype(np.float32))
    assert np.array_equal(got[..., 11][keep], f64[..., 11][keep].astype(np.float32))
    for key in "nzPa":
        assert d[key] <= 4.0 * ref[key], (key, d[key], ref[key])
    sky = keep & (f64[..., 7] == 0)
    assert (got[sky][:, :8] == 0).all() and (got[sky][:, 8:11] == 1).all()


# ---- 4. independence ---------------------------------------------------------------------------------
def test_followed_features_depend_on_nothing_random_and_leave_the_sums_alone():
    W, H, nsub, B = 32, 16, 2, 8
    scn, cam = scene_and_camera("box_mirror", W, H)
    with ptgpu.Context(scn, cam, device=0) as ctx:
        base = _feat(ctx, ptgpu.make_params(W, H, 4, nsub), B)
        for p in (ptgpu.make_params(W, H, 4, nsub, seed=7), ptgpu.make_params(W, H, 1000, nsub),
                  ptgpu.make_params(W, H, 4, nsub, flags=EXACT), ptgpu.make_params(W, H, 4, nsub, flags=0),
                  ptgpu.make_params(W, H, 4, nsub, flags=LS | MOM)):
            assert np.array_equal(_feat(ctx, p, B), base)
    assert base[..., 11].max() > 1
    # between two passes of a progressive frame (tests/test_gpu_denoise.py's scheme)
    p = ptgpu.make_params(W, H, 4, nsub, flags=MOM)
    res = []
    for with_call in (False, True):
        with ptgpu.Context(scn, cam, device=0) as ctx:
            color = torch.zeros((H, W, 3), dtype=torch.float32, device=DEV)
            var = torch.zeros_like(color)
            ctx.reset_accumulation(p)
            ctx.accumulate(p, 0, 2)
            if with_call:
                ctx.features(p, follow_bounces=B)
            ctx.accumulate(p, 2, 4)
            ctx.resolve(color, p, 4)
            ctx.noise(p, 4, 0.0, 1.0, var=var)
            res.append((color.cpu().numpy(), var.cpu().numpy()))
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])


# ---- 5. the drivers --------------------------------------------------------------------------------------
FOLLOW = 4
DRV = dict(name="mirror_back", W=48, H=32, nsub=2, samples=8)


def _k(cam, W, H, follow):
    k = ptgpu.denoise_defaults()
    k.pixel_spread = ptgpu.pixel_spread(cam, W, H)
    k.follow_bounces = follow
    return k


@pytest.mark.parametrize("flags", [0, EXACT], ids=["fast", "exact"])
def test_drivers_equal_their_pieces_and_the_host_filter(flags):
    name, W, H, nsub, samples = (DRV[k] for k in ("name", "W", "H", "nsub", "samples"))
    scn, cam = scene_and_camera(name, W, H)
    k = _k(cam, W, H, FOLLOW)
    p = ptgpu.make_params(W, H, samples, nsub, flags=flags | MOM)
    with ptgpu.Context(scn, cam, device=0) as ctx:
        color = torch.zeros((H, W, 3), dtype=torch.float32, device=DEV)
        var = torch.zeros_like(color)
        ctx.reset_accumulation(p)
        ctx.accumulate(p, 0, samples)
        ctx.resolve(color, p, samples)
        ctx.noise(p, samples, 0.0, 1.0, var=var)
        feat = ctx.features(p, follow_bounces=FOLLOW)
        first = ctx.features(p)
        want = ptgpu.denoise(color, var, feat, k).cpu().numpy()
        want0 = ptgpu.denoise(color, var, first, k).cpu().numpy()
        color, var, feat = color.cpu().numpy(), var.cpu().numpy(), feat.cpu().numpy()
    assert not np.array_equal(want, want0)  # the guide matters on this scene
    assert np.array_equal(ptgpu.denoise_host(color, var, feat, k), want)
    img = np.zeros((H, W, 3))
    ptgpu.render_denoised(scn, cam, img, W, H, samples, nsub, device=0, flags=flags, params=k)
    assert np.array_equal(img, want.astype(np.float64))
    # the noise-target driver that runs to the budget, and the adaptive one whose target is never met (every
    # pixel then holds `samples`): the same frame through the other two drivers
    img = np.zeros((H, W, 3))
    rep = ptgpu.render_to_noise_denoised(scn, cam, img, W, H, samples, 0.0, min_samples=4, num_subpixels=nsub, device=0,
                                         flags=flags, params=k)
    assert rep["samples_done"] == samples and np.array_equal(img, want.astype(np.float64))
    # with 0 the drivers are today's (params None: the same defaults)
    k0 = _k(cam, W, H, 0)
    a, b = np.zeros((H, W, 3)), np.zeros((H, W, 3))
    ptgpu.render_denoised(scn, cam, a, W, H, samples, nsub, device=0, flags=flags, params=k0)
    ptgpu.render_denoised(scn, cam, b, W, H, samples, nsub, device=0, flags=flags)
    assert np.array_equal(a, b) and np.array_equal(a, want0.astype(np.float64))


@pytest.mark.parametrize("flags", [0, EXACT], ids=["fast", "exact"])
def test_adaptive_driver_equals_its_pieces(flags):
    from test_gpu_adaptive import _rows, _run
    name, W, H, nsub = DRV["name"], DRV["W"], DRV["H"], DRV["nsub"]
    ends, target = (2, 4, 8), 0.1
    scn, cam = scene_and_camera(name, W, H)
    k = _k(cam, W, H, FOLLOW)
    p = ptgpu.make_params(W, H, ends[-1], nsub, flags=flags)
    with ptgpu.Context(scn, cam, device=0) as ctx:
        _run(ctx, p, ends, target, 1)
        color = torch.zeros((_rows(p), W, 3), dtype=torch.float32, device=DEV)
        var = torch.zeros_like(color)
        ctx.resolve_active(color, p)
        ctx.noise_active(p, 1.0, var)
        feat = ctx.features(p, follow_bounces=FOLLOW)
        want = ptgpu.denoise(color[:H], var[:H], feat[:H], k).cpu().numpy()
        color, var, feat = color[:H].cpu().numpy(), var[:H].cpu().numpy(), feat[:H].cpu().numpy()
    img = np.zeros((H, W, 3))
    rep, counts = ptgpu.render_adaptive_denoised(scn, cam, img, W, H, ends[-1], target, 0.01, 0.0, ends[0], 1, nsub,
                                                 ptgpu.DEFAULT_SEED, 0, flags, sample_counts=True, params=k)
    assert len(np.unique(counts)) >= 2
    assert np.array_equal(img, want.astype(np.float64))
    assert np.array_equal(ptgpu.denoise_host(color, var, feat, k), want)


@functools.lru_cache(maxsize=None)
def _one_device(W, H, kind):
    name, nsub, samples = DRV["name"], DRV["nsub"], DRV["samples"]
    scn, cam = scene_and_camera(name, W, H)
    k = _k(cam, W, H, FOLLOW)
    img = np.zeros((H * W, 3))
    if kind == "plain":
        ptgpu.render_denoised(scn, cam, img, W, H, samples, nsub, device=0, flags=EXACT, params=k)
        rest = ()
    elif kind == "to_noise":
        rest = (ptgpu.render_to_noise_denoised(scn, cam, img, W, H, samples, 0.1, 0.01, 0.3, 2, nsub, device=0, flags=EXACT,
                                               params=k),)
    else:
        rest = ptgpu.render_adaptive_denoised(scn, cam, img, W, H, samples, 0.1, 0.01, 0.0, 2, 1, nsub, device=0,
                                              flags=EXACT, sample_counts=True, params=k)
    img.setflags(write=False)
    return (img,) + tuple(rest)


def _multi_equals_one_device(m, cam, W, H, br):
    nsub, samples = DRV["nsub"], DRV["samples"]
    k = _k(cam, W, H, FOLLOW)
    p = ptgpu.make_params(W, H, samples, nsub, band_rows=br, flags=EXACT)
    got = np.zeros((H * W, 3))
    m.render_denoised(got, p, k)
    assert np.array_equal(got, _one_device(W, H, "plain")[0])
    got = np.zeros((H * W, 3))
    rep = m.render_to_noise_denoised(got, p, 0.1, 0.01, 0.3, 2, k)
    want = _one_device(W, H, "to_noise")
    assert rep == want[1] and np.array_equal(got, want[0])
    got = np.zeros((H * W, 3))
    rep, counts = m.render_adaptive_denoised(got, p, 0.1, 0.01, 0.0, 2, 1, sample_counts=True, denoise=k)
    want = _one_device(W, H, "adaptive")
    assert rep == want[1] and np.array_equal(counts, want[2]) and np.array_equal(got, want[0])
    # the pieces on the context's sums
    pm = ptgpu.make_params(W, H, samples, nsub, band_rows=br, flags=EXACT | MOM)
    m.reset_accumulation(pm)
    m.accumulate(pm, 0, samples)
    f32 = m.resolve_denoised(np.zeros((H, W, 3), np.float32), pm, samples, k)
    assert np.array_equal(f32.reshape(-1, 3).astype(np.float64), _one_device(W, H, "plain")[0])


@pytest.mark.parametrize("W,H,L,br", [(48, 32, L, br) for L in (1, 2, 3) for br in (1, 4)] + [(33, 21, 3, 2)])
def test_multi_drivers_equal_the_one_device_drivers(W, H, L, br):
    scn, cam = scene_and_camera(DRV["name"], W, H)
    k0 = _k(cam, W, H, 0)
    first = np.zeros((H * W, 3))
    ptgpu.render_denoised(scn, cam, first, W, H, DRV["samples"], DRV["nsub"], device=0, flags=EXACT, params=k0)
    assert not np.array_equal(first, _one_device(W, H, "plain")[0])  # the comparison proves something
    with ptgpu.MultiContext(scn, cam, [0], local_shards=L) as m:
        _multi_equals_one_device(m, cam, W, H, br)


def test_one_rank_communicator_and_the_one_shot_forms():
    W, H = DRV["W"], DRV["H"]
    scn, cam = scene_and_camera(DRV["name"], W, H)
    with ptgpu.MultiContext(scn, cam, [0]) as m:
        assert m.comm_info() == [(1, 0, 0)]  # a real communicator
        _multi_equals_one_device(m, cam, W, H, 1)
    # create + the call + destroy
    sp, ca = scn.to_array(), cam.to_array()
    k = _k(cam, W, H, FOLLOW)
    p = ptgpu.make_params(W, H, DRV["samples"], DRV["nsub"], flags=EXACT)
    L = ptgpu.lib()
    devs = (C.c_int * 1)(0)
    img = np.zeros((H * W, 3))
    ptgpu._abi.check(L.ptg_render_denoised_multi(sp.ctypes.data_as(C.c_void_p), len(sp), ca.ctypes.data_as(C.c_void_p),
                                                 C.byref(p), devs, 1, C.byref(k), img.ctypes.data_as(C.c_void_p)),
                     "ptg_render_denoised_multi")
    assert np.array_equal(img, _one_device(W, H, "plain")[0])


def test_seventeen_bounces_are_refused_by_every_driver():
    W, H = 16, 8
    scn, cam = scene_and_camera("box", W, H)
    sp, ca = scn.to_array(), cam.to_array()
    spp, cap = sp.ctypes.data_as(C.c_void_p), ca.ctypes.data_as(C.c_void_p)
    img = np.zeros((H, W, 3))
    f32 = np.zeros((H, W, 3), np.float32)
    ip = img.ctypes.data_as(C.c_void_p)
    devs = (C.c_int * 1)(0)
    nt = ptgpu.NoiseTarget(0.1, 0.01, 0.01, 2, 0)
    at = ptgpu._abi.AdaptiveTarget(0.1, 0.01, 0.01, 2, 1)
    L = ptgpu.lib()
    for bad in (17, -1):
        k = _k(cam, W, H, bad)
        p = ptgpu.make_params(W, H, 4, 2)
        pm = ptgpu.make_params(W, H, 4, 2, flags=MOM)
        with ptgpu.MultiContext(scn, cam, [0], local_shards=2) as m:
            m.reset_accumulation(pm)
            m.accumulate(pm, 0, 4)
            calls = {
                "ptg_render_denoised": lambda: L.ptg_render_denoised(spp, len(sp), cap, C.byref(p), 0, C.byref(k), ip),
                "ptg_render_to_noise_denoised": lambda: L.ptg_render_to_noise_denoised(
                    spp, len(sp), cap, C.byref(p), 0, C.byref(nt), C.byref(k), ip, None),
                "ptg_render_adaptive_denoised": lambda: L.ptg_render_adaptive_denoised(
                    spp, len(sp), cap, C.byref(p), 0, C.byref(at), C.byref(k), ip, None, None),
                "ptg_multi_resolve_denoised": lambda: L.ptg_multi_resolve_denoised(
                    m._h, C.byref(pm), 4, C.byref(k), f32.ctypes.data_as(C.c_void_p)),
                "ptg_multi_render_denoised": lambda: L.ptg_multi_render_denoised(m._h, C.byref(p), C.byref(k), ip),
                "ptg_multi_render_to_noise_denoised": lambda: L.ptg_multi_render_to_noise_denoised(
                    m._h, C.byref(p), C.byref(nt), C.byref(k), ip, None),
                "ptg_multi_render_adaptive_denoised": lambda: L.ptg_multi_render_adaptive_denoised(
                    m._h, C.byref(p), C.byref(at), C.byref(k), ip, None, None),
                "ptg_render_denoised_multi": lambda: L.ptg_render_denoised_multi(
                    spp, len(sp), cap, C.byref(p), devs, 1, C.byref(k), ip),
                "ptg_render_to_noise_denoised_multi": lambda: L.ptg_render_to_noise_denoised_multi(
                    spp, len(sp), cap, C.byref(p), devs, 1, C.byref(nt), C.byref(k), ip, None),
                "ptg_render_adaptive_denoised_multi": lambda: L.ptg_render_adaptive_denoised_multi(
                    spp, len(sp), cap, C.byref(p), devs, 1, C.byref(at), C.byref(k), ip, None, None),
            }
            for who, call in calls.items():
                assert call() == -1, (who, bad)
                assert b"follow_bounces" in L.ptg_last_error(), (who, L.ptg_last_error())
            # (the adaptive pieces: ptg_multi_resolve_active_denoised on adaptive sums)
            m.reset_accumulation(p)
            m.set_active_mask(p)
            m.accumulate_active(p, 2)
            assert L.ptg_multi_resolve_active_denoised(m._h, C.byref(p), C.byref(k),
                                                       f32.ctypes.data_as(C.c_void_p)) == -1
            assert b"follow_bounces" in L.ptg_last_error()
    assert (img == 0).all() and (f32 == 0).all()
    with ptgpu.Context(scn, cam, device=0) as ctx:
        with pytest.raises(ptgpu.PtgError, match="max_bounces"):
            ctx.features(ptgpu.make_params(W, H, 4, 2), follow_bounces=17)


def test_cli_follow(tmp_path):
    cli = os.path.join(os.path.dirname(ptgpu.LIB_PATH), "pt_render_gpu")
    W, H, spp = 64, 48, 64

    def run(tag, *extra):
        out = tmp_path / f"{tag}.ppm"
        r = subprocess.run([cli, "--scene", "box_mirror", "--width", str(W), "--height", str(H), "--format", "p6",
                            "--spp", str(spp), "--out", str(out), *extra], capture_output=True, text=True, timeout=120)
        return r, (out.read_bytes() if out.exists() else b"")

    head = len(f"P6\n{W} {H}\n255\n")
    scn = ptgpu.make_scene("box_mirror", W, H)
    cam = ptgpu.camera.with_config(scn.camera_parameters)
    k = ptgpu.denoise_defaults()
    k.pixel_spread, k.follow_bounces = 0.0, FOLLOW
    want = np.zeros((H, W, 3))
    ptgpu.render_denoised(scn, cam, want, W, H, spp // 4, 2, device=0, params=k)
    v = np.round(np.clip(want, 0, 1) ** (1 / 2.2) * 255).astype(np.int16).reshape(-1)
    for opt in ("--denoise", "--filter"):
        r, got = run(opt.strip("-"), opt, "--denoise-follow", str(FOLLOW))
        assert r.returncode == 0, r.stderr
        # (equal up to one 8-bit step where the two pow() round a tie apart, as tests/test_gpu_denoise.py compares)
        d = np.abs(np.frombuffer(got[head:], dtype=np.uint8).astype(np.int16) - v)
        assert d.max() <= 1 and (d != 0).sum() <= 2
    r, plain = run("plain", "--denoise")
    assert r.returncode == 0 and plain != got
    r, zero = run("zero", "--denoise", "--denoise-follow", "0")
    assert r.returncode == 0 and zero == plain
    # --features-follow: ptgpu.features(follow_bounces=) through the documented mapping
    r, _ = run("ff", "--features-out", str(tmp_path / "f"), "--features-follow", "8")
    assert r.returncode == 0, r.stderr
    feat = ptgpu.features(scn, cam, W, H, 2, device=0, follow_bounces=8).astype(np.float64)
    step = lambda x: np.floor(np.clip(x, 0, 1) * 255 + 0.5).astype(np.uint8).tobytes()  # noqa: E731
    assert (tmp_path / "f_albedo.ppm").read_bytes() == f"P6\n{W} {H}\n255\n".encode() + step(feat[..., 8:11])
    assert (tmp_path / "f_normal.ppm").read_bytes() == f"P6\n{W} {H}\n255\n".encode() + step((feat[..., 0:3] + 1) / 2)
    with ptgpu.Context(scn, cam, device=0) as ctx:
        assert np.array_equal(feat.astype(np.float32), _feat(ctx, ptgpu.make_params(W, H, 4, 2), 8))
    for extra, word in ((("--denoise-follow", "4"), "--denoise-follow"),
                        (("--denoise", "--denoise-follow", "17"), "0..16"),
                        (("--features-follow", "4"), "--features-out"),
                        (("--features-out", str(tmp_path / "g"), "--features-follow", "17"), "0..16")):
        r, _ = run("bad", *extra)
        assert r.returncode == 2 and word in r.stderr, (extra, r.stderr)


# ---- 6. acceptance ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _accept(name):
    """RMSE of the noisy frame, the first-hit filtered one and the followed filtered one (B = 8) against
    ptg_render_device at 4096 samples with light sampling: 64x48, nsub 2, 16 samples, filter defaults, the
    scene's own camera; all three from the same noisy frame."""
    W, H, nsub, samples = 64, 48, 2, 16
    scn = follow_scenes.mirror_back(W, H) if name == "mirror_back" else ptgpu.make_scene(name, W, H)
    cam = ptgpu.camera.with_config(scn.camera_parameters)
    k = ptgpu.denoise_defaults()
    k.pixel_spread = ptgpu.pixel_spread(cam, W, H)
    with ptgpu.Context(scn, cam, device=0) as ctx:
        ref = torch.zeros((H, W, 3), dtype=torch.float32, device=DEV)
        ctx.render_device(ref, ptgpu.make_params(W, H, 4096, nsub, flags=LS))
        p = ptgpu.make_params(W, H, samples, nsub, flags=MOM)
        color = torch.zeros((H, W, 3), dtype=torch.float32, device=DEV)
        var = torch.zeros_like(color)
        ctx.reset_accumulation(p)
        ctx.accumulate(p, 0, samples)
        ctx.resolve(color, p, samples)
        ctx.noise(p, samples, 0.0, 1.0, var=var)
        first = ptgpu.denoise(color, var, ctx.features(p), k)
        followed = ptgpu.denoise(color, var, ctx.features(p, follow_bounces=8), k)
        torch.cuda.synchronize()
        ref = ref.cpu().numpy().astype(np.float64)
        rmse = lambda a: float(np.sqrt(((a.cpu().numpy().astype(np.float64) - ref) ** 2).mean()))  # noqa: E731
        out = rmse(color), rmse(first), rmse(followed)
    print(f"{name}: RMSE noisy {out[0]:.5f} first-hit {out[1]:.5f} ({out[1] / out[0]:.3f}) followed {out[2]:.5f} "
          f"({out[2] / out[0]:.3f})")
    return out


def test_followed_guide_is_nearer_the_converged_frame_behind_a_mirror_wall():
    noisy, first, followed = _accept("mirror_back")
    assert followed < first and followed < noisy


@pytest.mark.parametrize("name", ["box", "simple"])
def test_followed_guide_keeps_the_existing_bar(name):
    noisy, first, followed = _accept(name)
    assert followed < noisy


def test_box_mirror_followed_guide_beats_the_first_hit_guide():
    """box_mirror, the scene whose first-hit filtered frame is further from the
    converged one than the noisy frame (ratio 1.265, DESIGN.md "Denoising"):
    every wall is a mirror there, so the first-hit guide sees five flat
    regions.  Measured: noisy 0.02137, first-hit 0.02703 (1.265), followed
    0.02113 (0.989) -- the followed guide removes the damage; it is asserted
    against the first-hit guide, not against the noisy frame, which it beats by
    a per cent only (most chains end in the sky, where the colour term alone
    acts)."""
    noisy, first, followed = _accept("box_mirror")
    assert followed < first
