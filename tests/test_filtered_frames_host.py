"""Host side of the filtered adaptive and multi-GPU frames (no GPU): the new
symbols, their argument checks (which run before any device call), the
command-line tool's refusals, and the numpy statement of the variance with
each pixel's own count against the uniform-count restatement."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import noise_active_ref
import ptgpu
from conftest import ROOT

INVALID, UNSUPPORTED = -1, -4
NEW = ("ptg_noise_active_device", "ptg_render_adaptive_denoised", "ptg_multi_resolve_denoised",
       "ptg_multi_resolve_active_denoised", "ptg_multi_render_denoised", "ptg_multi_render_to_noise_denoised",
       "ptg_multi_render_adaptive_denoised", "ptg_render_denoised_multi", "ptg_render_to_noise_denoised_multi",
       "ptg_render_adaptive_denoised_multi")
CLI = os.path.join(os.path.dirname(ptgpu.LIB_PATH), "pt_render_gpu")


def test_new_symbols_are_exported_declared_and_bound():
    with open(os.path.join(ROOT, "include", "ptgpu.h")) as f:
        header = f.read()
    out = subprocess.run(["nm", "-D", "--defined-only", ptgpu.LIB_PATH], capture_output=True, text=True).stdout
    L = ptgpu.lib()
    for s in NEW:
        assert re.search(rf"^int {s}\(", header, re.M), s
        assert re.search(rf"\bT {s}\b", out), s
        assert s in ptgpu.EXPORTS
        assert getattr(L, s).argtypes is not None and getattr(L, s).restype is C.c_int, s
    assert int(re.search(r"#define PTG_ABI_VERSION (\d+)", header).group(1)) == 2  # additive: the version stays
    for name in ("noise_active",):
        assert callable(getattr(ptgpu.Context, name))
    for name in ("resolve_denoised", "resolve_active_denoised", "render_denoised", "render_to_noise_denoised",
                 "render_adaptive_denoised"):
        assert callable(getattr(ptgpu.MultiContext, name))
    assert callable(ptgpu.render_adaptive_denoised)


def _scene():
    scn = ptgpu.box_scene(8, 8)
    cam = ptgpu.camera.with_config(scn.camera_parameters)
    return scn.to_array(), cam.to_array()


def _vp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _target(**kw):
    return ptgpu.AdaptiveTarget(kw.get("rel_error", 0.1), kw.get("floor", 0.01), kw.get("max_fraction", 0.0),
                                kw.get("min_samples", 4), kw.get("dilate", 1))


def _filter(**kw):
    k = ptgpu.denoise_defaults()
    for name, v in kw.items():
        setattr(k, name, v)
    return k


def test_adaptive_denoised_argument_checks():
    L = ptgpu.lib()
    sp, ca = _scene()
    img = np.zeros((64, 3))
    p = ptgpu.make_params(8, 8, 16)

    def call(sp=sp, ca=ca, p=p, target=_target(), k=None, img=img):
        return L.ptg_render_adaptive_denoised(_vp(sp), len(sp), _vp(ca), C.byref(p) if p else None, -1,
                                              C.byref(target) if target else None, C.byref(k) if k else None,
                                              _vp(img), None, None)

    cases = [
        (dict(img=None), b"NULL"), (dict(target=None), b"NULL"), (dict(p=None), b"NULL"), (dict(ca=None), b"NULL"),
        (dict(target=_target(floor=0.0)), b"floor"), (dict(target=_target(rel_error=-1.0)), b"rel_error"),
        (dict(target=_target(max_fraction=1.0)), b"max_fraction"), (dict(target=_target(dilate=9)), b"dilate"),
        (dict(target=_target(dilate=-1)), b"dilate"), (dict(target=_target(min_samples=1)), b">= 2"),
        (dict(p=ptgpu.make_params(8, 8, 1)), b">= 2"),
        (dict(p=ptgpu.make_params(8, 8, 16, shard_rank=1, shard_count=2)), b"shard_count"),
        (dict(k=_filter(iterations=9)), b"iterations"), (dict(k=_filter(eps_color=0.0)), b"eps_color"),
        (dict(k=_filter(pixel_spread=-1.0)), b"pixel_spread"), (dict(k=_filter(k_color=float("nan"))), b"k_"),
    ]
    for kw, msg in cases:
        assert call(**kw) == INVALID, kw
        assert msg in L.ptg_last_error(), (kw, L.ptg_last_error())
    assert call(p=ptgpu.make_params(8, 8, 16, flags=ptgpu.FLAG_REFERENCE_F64)) == UNSUPPORTED
    assert b"fp32 only" in L.ptg_last_error()
    assert not img.any()  # nothing was added to the image


def test_noise_active_and_multi_pieces_reject_null_arguments():
    L = ptgpu.lib()
    p = ptgpu.make_params(8, 8, 16)
    f32 = np.zeros((64, 3), dtype=np.float32)
    f64 = np.zeros((64, 3))
    assert L.ptg_noise_active_device(None, C.byref(p), 0.01, None, None, None) == INVALID
    assert b"NULL context" in L.ptg_last_error()
    assert L.ptg_multi_resolve_denoised(None, C.byref(p), 4, None, _vp(f32)) == INVALID
    assert L.ptg_multi_resolve_active_denoised(None, C.byref(p), None, _vp(f32)) == INVALID
    assert L.ptg_multi_render_denoised(None, C.byref(p), None, _vp(f64)) == INVALID
    t, a = ptgpu.NoiseTarget(0.1, 0.01, 0.0, 4, 0), _target()
    assert L.ptg_multi_render_to_noise_denoised(None, C.byref(p), C.byref(t), None, _vp(f64), None) == INVALID
    assert L.ptg_multi_render_adaptive_denoised(None, C.byref(p), C.byref(a), None, _vp(f64), None, None) == INVALID


def test_one_shot_multi_forms_check_their_arguments_before_any_device_work():
    L = ptgpu.lib()
    sp, ca = _scene()
    img = np.zeros((64, 3))
    devs = (C.c_int * 2)(0, 1)
    scene = (_vp(sp), len(sp), _vp(ca))
    p = ptgpu.make_params(8, 8, 16)
    t, a = ptgpu.NoiseTarget(0.1, 0.01, 0.0, 4, 0), _target()
    bad = _filter(iterations=9)

    def plain(p=p, k=None, img=img, n=2):
        return L.ptg_render_denoised_multi(*scene, C.byref(p), devs, n, C.byref(k) if k else None, _vp(img))

    def to_noise(p=p, t=t, k=None, img=img, n=2):
        return L.ptg_render_to_noise_denoised_multi(*scene, C.byref(p), devs, n, C.byref(t) if t else None,
                                                    C.byref(k) if k else None, _vp(img), None)

    def adaptive(p=p, a=a, k=None, img=img, n=2):
        return L.ptg_render_adaptive_denoised_multi(*scene, C.byref(p), devs, n, C.byref(a) if a else None,
                                                    C.byref(k) if k else None, _vp(img), None, None)

    for call in (plain, to_noise, adaptive):
        assert call(img=None) == INVALID and call(n=0) == INVALID
        assert call(k=bad) == INVALID and b"iterations" in L.ptg_last_error()
        assert call(p=ptgpu.make_params(8, 8, 16, shard_rank=1, shard_count=2)) == INVALID
        assert b"shard_count" in L.ptg_last_error()
        assert call(p=ptgpu.make_params(8, 8, 16, flags=ptgpu.FLAG_REFERENCE_F64)) == UNSUPPORTED
        assert call(p=ptgpu.make_params(8, 8, 1)) == INVALID and b">= 2" in L.ptg_last_error()
    assert to_noise(t=None) == INVALID and adaptive(a=None) == INVALID
    assert to_noise(t=ptgpu.NoiseTarget(0.1, 0.0, 0.0, 4, 0)) == INVALID and b"floor" in L.ptg_last_error()
    assert adaptive(a=_target(dilate=9)) == INVALID and b"dilate" in L.ptg_last_error()
    assert adaptive(a=_target(max_fraction=1.0)) == INVALID and b"max_fraction" in L.ptg_last_error()
    assert not img.any()


def _cli(*args):
    return subprocess.run([CLI, "--width", "8", "--height", "8", *args], capture_output=True, text=True, timeout=60)


def test_cli_refusals():
    """Exit status 2 before the scene is built or a device is touched."""
    for args, word in ((("--filter", "--denoise", "--spp", "64"), "--filter"),
                       (("--filter", "--spp", "4"), "--spp >= 8"),
                       (("--filter", "--denoise-iterations", "9", "--spp", "64"), "0..8"),
                       (("--filter", "--adaptive", "--spp", "64"), "--noise-target"),
                       (("--denoise-iterations", "3", "--spp", "64"), "--denoise"),
                       # the two refusals tests/test_gpu_denoise.py pins are unchanged
                       (("--denoise", "--noise-target", "0.1", "--adaptive", "--spp", "64"), "--adaptive"),
                       (("--denoise", "--devices", "0,1", "--spp", "64"), "one device")):
        r = _cli(*args)
        assert r.returncode == 2 and word in r.stderr, (args, r.returncode, r.stderr)


# ---- the variance with each pixel's own count, in numpy ---------------------------------------
def _random_sums(H, W, nsub, n, seed):
    """Sums a frame of n samples could hold: S1 of values in [0, 4), S2 >= S1^2 / n up to a heavy tail."""
    rng = np.random.default_rng(seed)
    c = rng.gamma(0.5, 0.8, size=(H, W, nsub * nsub, n, 3)).astype(np.float32)
    c[rng.random(c.shape) < 0.3] = 0.0
    q = lambda x: (x.astype(np.float64) * 2.0 ** 32).astype(np.uint64)  # noqa: E731
    return q(c).sum(axis=3, dtype=np.uint64), q(c * c).sum(axis=3, dtype=np.uint64)


@pytest.mark.parametrize("nsub,n", [(1, 2), (2, 2), (2, 16), (3, 7)])
def test_numpy_statement_equals_the_uniform_restatement(nsub, n):
    """At a uniform count n the statement with n_p = n is tests/test_gpu_noise.py's
    restatement of ptg_noise_device, to the bit: both definitions agree."""
    from test_gpu_noise import _noise_ref
    H, W, floor = 6, 9, 0.01
    S1, S2 = _random_sums(H, W, nsub, n, 100 * nsub + n)
    V, _, rho = _noise_ref(S1, S2, n, nsub, floor)
    got_v, got_rho = noise_active_ref.noise_active(S1, S2, np.full((H, W), n), nsub, floor)
    assert np.array_equal(got_v, V.astype(np.float32)) and np.array_equal(got_rho, rho)
    assert (got_v > 0).any() and np.isfinite(got_rho).all()


@pytest.mark.parametrize("nsub", [1, 2, 3, 8])
def test_numpy_statement_below_two_samples(nsub):
    """n_p < 2: rho = +inf and per channel the clamp's bound, whatever the sums hold."""
    S1, S2 = _random_sums(2, 3, nsub, 1, nsub)
    counts = np.array([[0, 1, 2], [1, 0, 5]])
    V, rho = noise_active_ref.noise_active(S1, S2, counts, nsub, 0.01)
    cap = noise_active_ref.v_cap(nsub)
    unknown = counts < 2
    assert (V[unknown] == cap).all() and np.isinf(rho[unknown]).all()
    assert np.isfinite(rho[~unknown]).all() and (V[~unknown] <= cap).all()
    # the cap is what the definition yields with every sub-pixel's variance at 1/4
    inv32 = np.float32(1.0) / np.float32(nsub * nsub)
    vs = 0.0
    for _ in range(nsub * nsub):
        vs += 0.25
    assert cap == np.float32(float(inv32) * float(inv32) * vs)
