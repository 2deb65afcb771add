"""Host side of the noise-target and adaptive frames on several GPUs (no GPU):
the new declarations of include/ptgpu.h against the ctypes bindings, the
argument checks that run before any device work, and a numpy restatement of
the two rules the gathered active list rests on -- where a pixel of the image
lives in rank-major gathered slabs, and the clipped window dilation.
tests/test_gpu_multi_adaptive.py uses the restatement as its expectation; here
it is checked against ptgpu.slab_to_image_rows / unshard_host."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ptgpu
from conftest import ROOT

INVALID, NO_DEVICE, UNSUPPORTED = -1, -3, -4
NEW = ("ptg_select_over_device", "ptg_set_active_gathered_device", "ptg_multi_noise", "ptg_multi_set_active_mask",
       "ptg_multi_select_active", "ptg_multi_accumulate_active", "ptg_multi_resolve_active",
       "ptg_multi_read_sample_counts", "ptg_multi_render_to_noise", "ptg_multi_render_adaptive",
       "ptg_render_to_noise_multi", "ptg_render_adaptive_multi")


# ---- the numpy restatement --------------------------------------------------------------
def gathered_place(r, band_rows, n):
    """(rank, slab row) of image row r in n rank-major slabs of interleaved bands."""
    band = r // band_rows
    return band % n, (band // n) * band_rows + r % band_rows


def slab_rows(H, band_rows, n):
    bands = -(-H // band_rows)
    return -(-bands // n) * band_rows


def split_rank_major(a, band_rows, n):
    """Image rows a [H, ...] -> [n, slab rows, ...], zero in the slab rows past the image."""
    a = np.asarray(a)
    out = np.zeros((n, slab_rows(a.shape[0], band_rows, n)) + a.shape[1:], dtype=a.dtype)
    for r in range(a.shape[0]):
        k, j = gathered_place(r, band_rows, n)
        out[k, j] = a[r]
    return out


def join_rank_major(g, H, band_rows, n):
    """The inverse: [n, slab rows, ...] -> [H, ...]."""
    g = np.asarray(g)
    out = np.zeros((H,) + g.shape[2:], dtype=g.dtype)
    for r in range(H):
        k, j = gathered_place(r, band_rows, n)
        out[r] = g[k, j]
    return out


def dilate_clipped(over, d):
    """active[y, x] = some over byte of rows y-d..y+d, columns x-d..x+d inside the image is set."""
    over = np.asarray(over) != 0
    H, W = over.shape
    out = np.zeros((H, W), dtype=bool)
    for y in range(H):
        rows = over[max(y - d, 0):min(y + d, H - 1) + 1].any(axis=0)  # the column OR: the kernel's first step
        for x in range(W):
            out[y, x] = rows[max(x - d, 0):min(x + d, W - 1) + 1].any()
    return out


def units_of(active, ppw):
    """A row's active pixels cut into units of ppw: the total over the rows."""
    return int(sum(-(-int(r.sum()) // ppw) for r in np.asarray(active) != 0))


@pytest.mark.parametrize("H,br,n", [(9, 2, 3), (9, 1, 2), (9, 7, 3), (5, 2, 1), (1, 1, 3), (24, 4, 3), (18, 7, 8)])
def test_rank_major_mapping_is_the_slab_layout(H, br, n):
    assert slab_rows(H, br, n) == ptgpu.shard_rows(H, br, n)
    seen = np.full(H, -1)
    for k in range(n):
        m = ptgpu.slab_to_image_rows(H, br, k, n)
        for j, r in enumerate(m):
            if r >= 0:
                assert gathered_place(int(r), br, n) == (k, j)
                seen[r] = k
    assert (seen >= 0).all()
    W = 4
    img = np.arange(H * W * 3, dtype=np.float32).reshape(H, W, 3) + 1
    g = split_rank_major(img, br, n)
    assert np.array_equal(ptgpu.unshard_host(g, W, H, br, n), img)
    assert np.array_equal(join_rank_major(g, H, br, n), img)
    pad = np.ones(g.shape[:2], dtype=bool)
    for r in range(H):
        pad[gathered_place(r, br, n)] = False
    assert not g[pad].any()  # the slab rows past the image


def test_clipped_dilation():
    rng = np.random.default_rng(5)
    for H, W in ((9, 30), (5, 7), (1, 1), (1, 12), (20, 1)):
        over = rng.random((H, W)) < 0.06
        assert np.array_equal(dilate_clipped(over, 0), over)
        for d in (1, 2, 8):
            got = dilate_clipped(over, d)
            want = np.zeros_like(over)
            ys, xs = np.nonzero(over)
            for y, x in zip(ys, xs):  # every set byte paints its own window
                want[max(y - d, 0):y + d + 1, max(x - d, 0):x + d + 1] = True
            assert np.array_equal(got, want), (H, W, d)
    one = np.zeros((9, 300), np.uint8)
    one[0, 255] = 1
    a = dilate_clipped(one, 8)
    assert a.sum() == 9 * 17 and a[8, 263] and a[0, 247] and not a[0, 264] and not a[0, 246]
    assert units_of(a, 16) == 9 * 2 and units_of(a, 64) == 9 and units_of(np.zeros((3, 3)), 16) == 0


# ---- declarations and bindings -----------------------------------------------------------
def test_header_declares_the_new_entry_points_and_the_abi_version_stays():
    with open(os.path.join(ROOT, "include", "ptgpu.h")) as f:
        text = f.read()
    for name in NEW:
        assert re.search(rf"^int {name}\(", text, re.M), name
        assert name in ptgpu.EXPORTS and hasattr(ptgpu.lib(), name), name
    assert int(re.search(r"#define PTG_ABI_VERSION (\d+)", text).group(1)) == 2 == ptgpu.ABI_VERSION  # additive
    for meth in ("noise", "set_active_mask", "select_active", "accumulate_active", "resolve_active",
                 "read_sample_counts", "render_to_noise", "render_adaptive"):
        assert callable(getattr(ptgpu.MultiContext, meth)), meth
    assert callable(ptgpu.Context.select_over) and callable(ptgpu.Context.set_active_gathered)


# ---- argument checks before any device work ----------------------------------------------
def _scene8():
    scn = ptgpu.box_scene(8, 8)
    cam = ptgpu.camera.with_config(scn.camera_parameters)
    return scn, cam, scn.to_array(), cam.to_array()


def _vp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def test_device_primitives_refuse_bad_arguments_without_gpu_work():
    L = ptgpu.lib()
    p = ptgpu.make_params(8, 8, 16)
    sh = ptgpu.make_params(8, 8, 16, band_rows=2, shard_rank=1, shard_count=3)
    P = C.byref(p)
    # non-NULL handles that the argument checks never dereference.  A real zeroed allocation, far larger
    # than a context, so that a check moved behind the first dereference fails this test (a context
    # without a scene on device 0) and does not take the process down with a wild pointer.
    zeros = C.create_string_buffer(1 << 20)
    one = C.cast(zeros, C.c_void_p)
    assert L.ptg_select_over_device(None, P, 0.1, 0.01, one, None, None, None) == INVALID and b"NULL" in L.ptg_last_error()
    assert L.ptg_select_over_device(one, P, 0.1, 0.01, None, None, None, None) == INVALID and b"NULL" in L.ptg_last_error()
    assert L.ptg_select_over_device(one, None, 0.1, 0.01, one, None, None, None) == INVALID
    assert b"params is NULL" in L.ptg_last_error()
    assert L.ptg_select_over_device(one, P, 0.1, 0.0, one, None, None, None) == INVALID and b"floor" in L.ptg_last_error()
    assert L.ptg_select_over_device(one, P, -1.0, 0.01, one, None, None, None) == INVALID
    assert L.ptg_set_active_gathered_device(None, P, one, 0, None, None) == INVALID and b"NULL" in L.ptg_last_error()
    assert L.ptg_set_active_gathered_device(one, P, None, 0, None, None) == INVALID and b"NULL" in L.ptg_last_error()
    assert L.ptg_set_active_gathered_device(one, None, one, 0, None, None) == INVALID
    for d in (-1, 9):  # a shard is accepted with any dilate in 0..8: only the range is refused
        assert L.ptg_set_active_gathered_device(one, C.byref(sh), one, d, None, None) == INVALID
        assert b"dilate" in L.ptg_last_error()
    # the existing entry point keeps refusing a dilated list on a shard
    assert L.ptg_select_active_device(one, C.byref(sh), 0.1, 0.01, 1, None, None, None) == UNSUPPORTED


def test_multi_entry_points_refuse_null_contexts():
    L = ptgpu.lib()
    p = ptgpu.make_params(8, 8, 16)
    P = C.byref(p)
    st = np.zeros(6, dtype=np.uint64)
    img = np.zeros((64, 3))
    t, a = ptgpu.NoiseTarget(0.1, 0.01, 0.0, 4, 0), ptgpu.AdaptiveTarget(0.1, 0.01, 0.0, 4, 1)
    calls = [lambda: L.ptg_multi_noise(None, P, 4, 0.1, 0.01, _vp(st)),
             lambda: L.ptg_multi_set_active_mask(None, P, None),
             lambda: L.ptg_multi_select_active(None, P, 0.1, 0.01, 1, _vp(st)),
             lambda: L.ptg_multi_accumulate_active(None, P, 1),
             lambda: L.ptg_multi_resolve_active(None, P, _vp(img)),
             lambda: L.ptg_multi_read_sample_counts(None, P, _vp(img)),
             lambda: L.ptg_multi_render_to_noise(None, P, C.byref(t), _vp(img), None),
             lambda: L.ptg_multi_render_adaptive(None, P, C.byref(a), _vp(img), None, None)]
    for call in calls:
        assert call() == INVALID and b"NULL" in L.ptg_last_error()
    assert L.ptg_multi_render_to_noise(None, P, None, _vp(img), None) == INVALID
    assert L.ptg_multi_render_adaptive(None, P, C.byref(a), None, None, None) == INVALID
    assert not img.any()


def _adaptive(sp, ca, p, target, img, devices=(0,), counts=None, rep=None):
    devs = (C.c_int * max(len(devices), 1))(*devices) if devices is not None else None
    return ptgpu.lib().ptg_render_adaptive_multi(_vp(sp), len(sp) if sp is not None else 0, _vp(ca),
                                                 C.byref(p) if p else None, devs, len(devices) if devices else 0,
                                                 C.byref(target) if target else None, _vp(img), _vp(counts),
                                                 C.byref(rep) if rep else None)


def _to_noise(sp, ca, p, target, img, devices=(0,), rep=None):
    devs = (C.c_int * max(len(devices), 1))(*devices) if devices is not None else None
    return ptgpu.lib().ptg_render_to_noise_multi(_vp(sp), len(sp) if sp is not None else 0, _vp(ca),
                                                 C.byref(p) if p else None, devs, len(devices) if devices else 0,
                                                 C.byref(target) if target else None, _vp(img),
                                                 C.byref(rep) if rep else None)


def test_one_shot_wrappers_check_their_arguments_before_any_device_work():
    L = ptgpu.lib()
    scn, cam, sp, ca = _scene8()
    img = np.zeros((64, 3))
    p = ptgpu.make_params(8, 8, 16)
    ok = lambda **kw: ptgpu.AdaptiveTarget(kw.get("rel_error", 0.1), kw.get("floor", 0.01),  # noqa: E731
                                           kw.get("max_fraction", 0.0), kw.get("min_samples", 4), kw.get("dilate", 1))
    nt = lambda **kw: ptgpu.NoiseTarget(kw.get("rel_error", 0.1), kw.get("floor", 0.01),  # noqa: E731
                                        kw.get("max_fraction", 0.0), kw.get("min_samples", 4), 0)
    sharded = ptgpu.make_params(8, 8, 16, shard_rank=1, shard_count=2)
    cases = [
        (dict(p=p, target=ok(), img=None), b"NULL"),
        (dict(p=p, target=None, img=img), b"NULL"),
        (dict(p=None, target=ok(), img=img), b"NULL"),
        (dict(p=p, target=ok(), img=img, devices=None), b"NULL"),
        (dict(p=p, target=ok(), img=img, devices=()), b"no device"),
        (dict(p=sharded, target=ok(), img=img), b"shard_count"),
        (dict(p=p, target=ok(dilate=9), img=img), b"dilate"),
        (dict(p=p, target=ok(dilate=-1), img=img), b"dilate"),
        (dict(p=p, target=ok(floor=0.0), img=img), b"floor"),
        (dict(p=p, target=ok(rel_error=-0.5), img=img), b"rel_error"),
        (dict(p=p, target=ok(max_fraction=1.0), img=img), b"max_fraction"),
        (dict(p=p, target=ok(min_samples=1), img=img), b">= 2"),
    ]
    for kw, msg in cases:
        assert _adaptive(sp, ca, **kw) == INVALID, msg
        assert msg in L.ptg_last_error(), (msg, L.ptg_last_error())
        if b"dilate" in msg:
            continue
        kw = dict(kw, target=nt(**{k: getattr(kw["target"], k) for k in ("rel_error", "floor", "max_fraction",
                                                                           "min_samples")}) if kw["target"] else None)
        assert _to_noise(sp, ca, **kw) == INVALID, msg
        assert msg in L.ptg_last_error(), (msg, L.ptg_last_error())
    p64 = ptgpu.make_params(8, 8, 16, flags=ptgpu.FLAG_REFERENCE_F64)
    assert _adaptive(sp, ca, p64, ok(), img) == UNSUPPORTED and b"fp32" in L.ptg_last_error()
    assert _to_noise(sp, ca, p64, nt(), img) == UNSUPPORTED and b"fp32" in L.ptg_last_error()
    n = C.c_int(0)
    L.ptg_device_count(C.byref(n))
    if n.value == 0:  # no GPU here: valid arguments reach the device layer and come back cleanly
        counts = np.full((8, 8), -5, dtype=np.int32)
        rep, nrep = ptgpu.AdaptiveReport(), ptgpu.NoiseReport()
        assert _adaptive(sp, ca, p, ok(), img, counts=counts, rep=rep) == NO_DEVICE
        assert _adaptive(sp, ca, p, ok(), img, devices=(0, 1), counts=counts, rep=rep) == NO_DEVICE
        assert _to_noise(sp, ca, p, nt(), img, rep=nrep) == NO_DEVICE
        assert (counts == -5).all() and rep.passes == 0 and nrep.passes == 0
        with pytest.raises(ptgpu.PtgError, match=r"\(-3\)"):
            ptgpu.MultiContext(scn, cam, [0])
    assert not img.any()  # nothing was added to the image
