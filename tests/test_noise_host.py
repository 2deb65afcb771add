"""Host side of the noise estimates (no GPU): the pass schedule and the
argument checks of ptg_render_to_noise, which run before any device call."""
import ctypes as C

import numpy as np
import pytest

import ptgpu

INVALID = -1  # PTG_ERR_INVALID_ARGUMENT


def test_schedule_doubles_and_ends_on_samples():
    assert ptgpu.noise_schedule(2, 2) == [2]
    assert ptgpu.noise_schedule(4, 100) == [4, 8, 16, 32, 64, 100]
    assert ptgpu.noise_schedule(16, 64) == [16, 32, 64]
    assert ptgpu.noise_schedule(16, 65) == [16, 32, 64, 65]


def test_schedule_min_above_samples():
    assert ptgpu.noise_schedule(8, 5) == [5]
    assert ptgpu.noise_schedule(8, 2) == [2]
    with pytest.raises(ptgpu.PtgError, match=">= 2"):
        ptgpu.noise_schedule(8, 1)
    with pytest.raises(ptgpu.PtgError, match=">= 2"):
        ptgpu.noise_schedule(1, 64)


def test_schedule_longest_fits_the_report():
    ends = ptgpu.noise_schedule(2, 2 ** 31 - 1)
    assert len(ends) == 31 <= ptgpu.NoiseReport.pass_samples.size // 4
    assert ends[-1] == 2 ** 31 - 1 and ends[-2] == 2 ** 30


def test_schedule_cap_too_small():
    L = ptgpu.lib()
    ends = (C.c_int32 * 8)(*([-7] * 8))
    n = C.c_int32(-1)
    assert L.ptg_noise_schedule(4, 100, ends, 5, C.byref(n)) == INVALID
    assert b"room for 5" in L.ptg_last_error() and n.value == 0
    assert list(ends[5:]) == [-7, -7, -7]  # nothing written past cap
    assert L.ptg_noise_schedule(4, 100, ends, 6, C.byref(n)) == 0 and n.value == 6
    assert L.ptg_noise_schedule(4, 100, None, 6, C.byref(n)) == INVALID
    assert L.ptg_noise_schedule(4, 100, ends, 6, None) == INVALID


def _call(sp, ca, p, target, img, rep=None):
    L = ptgpu.lib()
    vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
    return L.ptg_render_to_noise(vp(sp), len(sp) if sp is not None else 0, vp(ca), C.byref(p) if p else None, -1,
                                 C.byref(target) if target else None, vp(img), C.byref(rep) if rep else None)


def test_render_to_noise_argument_checks():
    L = ptgpu.lib()
    scn = ptgpu.box_scene(8, 8)
    cam = ptgpu.camera.with_config(scn.camera_parameters)
    sp, ca = scn.to_array(), cam.to_array()
    img = np.zeros((64, 3))
    p = ptgpu.make_params(8, 8, 16)
    ok = lambda **kw: ptgpu.NoiseTarget(kw.get("rel_error", 0.1), kw.get("floor", 0.01),  # noqa: E731
                                        kw.get("max_fraction", 0.0), kw.get("min_samples", 4), 0)
    cases = [
        ((sp, ca, p, ok(), None), b"NULL"),
        ((sp, ca, p, None, img), b"NULL"),
        ((sp, ca, None, ok(), img), b"params is NULL"),
        ((sp, None, p, ok(), img), b"NULL"),
        ((sp, ca, p, ok(floor=0.0), img), b"floor"),
        ((sp, ca, p, ok(floor=-1.0), img), b"floor"),
        ((sp, ca, p, ok(floor=float("nan")), img), b"floor"),
        ((sp, ca, p, ok(rel_error=-0.5), img), b"rel_error"),
        ((sp, ca, p, ok(max_fraction=1.0), img), b"max_fraction"),
        ((sp, ca, p, ok(max_fraction=-0.1), img), b"max_fraction"),
        ((sp, ca, p, ok(max_fraction=float("nan")), img), b"max_fraction"),
        ((sp, ca, ptgpu.make_params(8, 8, 16, shard_rank=1, shard_count=2), ok(), img), b"shard_count"),
        ((sp, ca, p, ok(min_samples=1), img), b">= 2"),
        ((sp, ca, ptgpu.make_params(8, 8, 1), ok(), img), b">= 2"),
    ]
    for args, msg in cases:
        assert _call(*args) == INVALID, msg
        assert msg in L.ptg_last_error(), (msg, L.ptg_last_error())
    assert not img.any()  # nothing was added to the image
    # a NULL sphere array with a non-zero count
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    t = ok()
    assert L.ptg_render_to_noise(None, 3, vp(ca), C.byref(p), -1, C.byref(t), vp(img), None) == INVALID
    # the reference-arithmetic mode has no progressive passes
    p64 = ptgpu.make_params(8, 8, 16, flags=ptgpu.FLAG_REFERENCE_F64)
    assert _call(sp, ca, p64, ok(), img) == -4 and b"fp32 only" in L.ptg_last_error()


def test_flag_and_struct_layout_match_the_header():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "ptgpu.h")) as f:
        text = f.read()
    assert int(re.search(r"#define PTG_FLAG_MOMENTS (\d+)", text).group(1)) == ptgpu.FLAG_MOMENTS == 16
    assert int(re.search(r"#define PTG_NOISE_MAX_PASSES (\d+)", text).group(1)) == len(ptgpu.NoiseReport().pass_over)
    assert int(re.search(r"#define PTG_ABI_VERSION (\d+)", text).group(1)) == 2  # additive: the version stays
    assert ptgpu.NoiseReport.pass_over.offset == 48 + 4 * 32 and ptgpu.NoiseTarget.min_samples.offset == 24
