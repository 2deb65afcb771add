"""The cases of tests/shape_scenes.py on the CPU: the library's host scene
preparation lays every one out as the oracle does, the layouts are the ones
the GPU tests count on (which walls pair, which stay single, which take the
general anchor), the oracle renders each to a finite, lit image, and -- the
guard on the cases, test_wall_rules.py's bar -- testing every sphere in index
order (BV_FULL_SCAN: no pairs, no box mode) gives the same image on at least
99.9 % of the pixels.
"""
import functools

import numpy as np
import pytest

import ptgpu
import pyoracle as po
import shape_scenes as ss

SEED = 0x5EED0001
W, H, SAMPS = 48, 32, 4


@functools.lru_cache(maxsize=None)
def _oracle(name):
    sp, ca = ss.oracle_arrays(*ss.make(name, W, H))
    img, segs = po.render_xs_f32(sp, ca, W, H, SAMPS, 2, SEED)
    img.setflags(write=False)
    return sp, ca, img, segs


@pytest.mark.parametrize("name", list(ss.CASES))
def test_layout_equals_the_oracles(name):
    scn, cam = ss.make(name, W, H)
    sp, ca = ss.oracle_arrays(scn, cam)
    assert ptgpu.scene_layout(scn, cam) == po.scan_layout(sp, ca)
    counts = {"empty": 0, "single": 1, "room59": 64, "inside0": 5, "outside0": 5}
    if name in counts:
        assert len(scn.spheres) == counts[name]
    if name.startswith("cluster"):
        assert len(scn.spheres) == int(name[7:9])
        assert cam.lens_radius == (0.15 if name.endswith("_lens") else 0.0)


@pytest.mark.parametrize("name", list(ss.LAYOUTS))
def test_layout_is_the_expected_one(name):
    scn, cam = ss.make(name, W, H)
    want = ss.LAYOUTS[name]
    axis, order = po.scan_layout(*ss.oracle_arrays(scn, cam))
    assert axis[:len(want)] == want
    assert axis[len(want):] == [-1] * (len(scn.spheres) - len(want))  # the rest are small spheres
    if name in ss.BOX_MODE:
        assert len(scn.spheres) - len(want) == ss.BOX_MODE[name]


@pytest.mark.parametrize("name", list(ss.CASES))
def test_oracle_image_is_finite_and_lit(name):
    sp, ca, img, segs = _oracle(name)
    assert np.isfinite(img).all() and img.min() >= 0.0 and img.max() <= 1.0
    assert float(img.mean()) > 0.0
    if name in ss.ROOMS or name in ss.OPEN or name in ("inside0", "outside0", "sliver"):
        assert float(img.mean()) > 0.01
    if name == "empty":
        # every path is one segment into the sky, (1 - t) (1, 1, 1) + t (0.5, 0.7, 1): whatever t
        # each path has, the mean keeps g = 0.4 + 0.6 r and b = 1
        assert segs == W * H * 4 * SAMPS
        r, g, b = (img[..., c].astype(np.float64) for c in range(3))
        assert r.min() >= 0.5 and np.abs(g - (0.4 + 0.6 * r)).max() < 1e-5 and np.abs(b - 1.0).max() < 1e-5
        # and t = (u_y + 1) / 2 of the unit direction u: the sky through each pixel's centre from
        # the camera position.  A path aims within 0.75 pixel of the centre (the tent filter:
        # u_y moves by < 0.75 * 2 tan(0.25) / 32 = 0.012) from a lens point within 0.2 of the
        # position, 2.6 from the focus plane (< 0.077): r = 1 - t / 2 within 0.25 * 0.089 = 0.022
        c = ca[0]
        v = (H - 1 - np.arange(H) + 0.5)[:, None, None] / H  # image row 0 is the top
        u = ((np.arange(W) + 0.5) / W)[None, :, None]
        d = c["lower_left_corner"] + u * c["cam_x_axis"] + v * c["cam_y_axis"] - c["position"]
        uy = d[..., 1] / np.sqrt((d * d).sum(axis=2))
        dev = float(np.abs(r - (1.0 - 0.25 * (uy + 1.0))).max())
        print(f"empty: max |r - sky(pixel centre)| {dev:.4f}; r spans {r.min():.3f} .. {r.max():.3f}")
        assert dev < 0.022


@pytest.mark.parametrize("name", list(ss.CASES))
def test_full_scan_gives_the_same_image(name):
    sp, ca, img, _ = _oracle(name)
    with po.mode_b_variant(po.BV_FULL_SCAN):
        full, _ = po.render_xs_f32(sp, ca, W, H, SAMPS, 2, SEED)
    same = float((np.abs(img.astype(np.float64) - full).max(axis=2) == 0).mean())
    assert same >= 0.999, same
