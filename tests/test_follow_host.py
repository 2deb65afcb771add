"""Followed features on the CPU (include/ptgpu.h "denoising",
ptg_features_follow_device): the numpy restatement tests/follow_ref.py against
tests/denoise_ref.first_hit, against a mirror image, against Snell's law
written independently, at the bounce cap; the exclusion rule of the GPU test
proved between float32 and float64; and the ABI."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import denoise_ref
import follow_ref
import follow_scenes
import ptgpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- B = 0 ---------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name,W,H,nsub", [("box_mirror", 32, 24, 2), ("simple", 32, 24, 1), ("synthetic:300", 16, 9, 2)])  # noqa: E501
def test_no_bounce_is_the_first_hit(name, W, H, nsub, dtype):
    scn, cam = follow_scenes.scene_and_camera(name, W, H)
    want, ids = denoise_ref.first_hit(scn, cam, W, H, nsub, dtype)
    got, chains, bounces, _ = follow_ref.follow(scn, cam, W, H, nsub, 0, dtype)
    assert np.array_equal(got, want)
    assert np.array_equal(chains[..., 0], ids)
    assert np.array_equal(bounces, np.where(ids >= 0, 0, -1))


# ---- a mirror shows the mirror image ---------------------------------------------
def test_plane_like_mirror_shows_the_mirror_image():
    """One bounce on a specular sphere of R = 1e5 touching the plane z = 0
    against the direct view from the camera reflected in that plane (whose x
    axis is the mirror image too: column x there is column W - 1 - x here).
    The sphere leaves the plane by the sagitta s = r^2 / 2R at distance r from
    the touching point and its normal tilts by r / R, which turns the
    reflected ray by 2 r / R: over a path of length L behind the mirror the
    ray moves sideways by at most 2 s + 2 (r / R) L where it ends, so the point
    on a surface met at cosine c by (2 s + 2 (r / R) L) / c, the distance by at
    most twice that, the normal of a sphere of radius rb by that over rb."""
    W, H = 48, 36
    scn, cam = follow_scenes.mirror_plane(W, H)
    got, chains, bounces, _ = follow_ref.follow(scn, cam, W, H, 1, 1)
    mscn, mcam = follow_scenes.mirror_plane(W, H, mirrored_camera=True)
    want, ids = denoise_ref.first_hit(mscn, mcam, W, H, 1)
    want, ids = want[:, ::-1], ids[:, ::-1]
    first = chains[..., 0, 0] == 2  # the rays that meet the mirror first (the others see the ball directly)
    same = chains[..., 0, 1] == ids[..., 0]
    assert first.mean() > 0.8 and same[first].mean() >= 0.99
    m = first & same & (ids[..., 0] >= 0)
    assert m.mean() > 0.25 and set(ids[..., 0][m]) == {0, 1}  # the ball's image and the floor's
    # per pixel, from the direct view: where the ray crosses z = 0 (r from the touching point), the path L
    # behind the mirror, and the cosine at which it meets the surface it ends on
    d = want[..., 4:7] - np.array(mcam.position)
    cross = np.array(mcam.position) + d * (3.0 / d[..., 2:3])
    r = np.linalg.norm(cross[..., :2], axis=-1)
    L = np.linalg.norm(want[..., 4:7] - cross, axis=-1)
    cosi = np.abs((want[..., 0:3] * d).sum(-1)) / np.linalg.norm(d, axis=-1)
    sag, tilt = r * r / (2 * follow_scenes.MIRROR_R), r / follow_scenes.MIRROR_R
    with np.errstate(invalid="ignore", divide="ignore"):  # (sky pixels: not compared)
        tol_P = (2 * sag + 2 * tilt * L) / cosi
    radius = np.where(ids[..., 0] == 0, follow_scenes.BALL_R, 1000.0)
    dP = np.linalg.norm(got[..., 4:7] - want[..., 4:7], axis=-1)
    dz = np.abs(got[..., 3] - want[..., 3])
    dn = np.abs(got[..., 0:3] - want[..., 0:3]).max(-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratios = ((dP / tol_P)[m].max(), (dz / (2 * tol_P))[m].max(), (dn * radius / tol_P)[m].max())
    print(f"r <= {r[m].max():.3f}, L <= {L[m].max():.3f}, sagitta <= {sag[m].max():.2e}: largest dP / tol "
          f"{ratios[0]:.3f}, dz / 2 tol {ratios[1]:.3f}, "
          f"dn / (tol / R) {ratios[2]:.3f}; dP <= {dP[m].max():.2e}")
    assert dP[m].max() > 0  # (the sphere is not the plane: the comparison is not of a thing with itself)
    assert (dP <= tol_P)[m].all() and (dz <= 2 * tol_P)[m].all() and (dn <= tol_P / radius + 1e-12)[m].all()
    assert (got[..., 7][m] == 1).all() and (got[..., 11][m] == 1).all()
    assert np.allclose(got[..., 8:11][m], want[..., 8:11][m], rtol=0, atol=1e-15)  # T = the mirror's (1, 1, 1)


# ---- glass against Snell's law -----------------------------------------------------
def test_glass_ball_against_snells_law():
    """A glass ball (the renderer's ratio 0.5 entering: index 2) in front of a
    wall, B = 2.  Written with unit directions, angles and asin: the ray
    enters at angle ti to the normal, runs a chord at tt = asin(sin ti / 2),
    meets the far side at the same angle tt and leaves at ti."""
    W, H = 40, 30
    scn, cam = follow_scenes.glass_ball(W, H)
    got, chains, bounces, _ = follow_ref.follow(scn, cam, W, H, 1, 2)
    ca = cam.to_array()[0]
    o = ca["position"]
    base = ca["lower_left_corner"] - o
    rows, xs = np.mgrid[0:H, 0:W]
    fs, ft = (xs + 0.5) / W, (H - 1 - rows + 0.5) / H
    d = base + fs[..., None] * ca["cam_x_axis"] + ft[..., None] * ca["cam_y_axis"]
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    R, Cw, Rw = 0.5, np.array([0.0, 0.0, -1002.0]), 1000.0
    # the ball from outside: foot of the perpendicular from its centre (the origin)
    tca = -(o * d).sum(-1)
    h2 = (o * o).sum() - tca * tca
    through = chains[..., 0, 0] == 0
    assert np.array_equal(through, h2 < R * R) and through.sum() > 50
    t1 = tca - np.sqrt(np.where(through, R * R - h2, 0))
    p1 = o + t1[..., None] * d
    n1 = p1 / R
    ti = np.arccos(np.clip(-(d * n1).sum(-1), -1, 1))
    tt = np.arcsin(np.sin(ti) / 2.0)
    tang = d + np.cos(ti)[..., None] * n1
    tl = np.linalg.norm(tang, axis=-1, keepdims=True)
    tang = np.where(tl > 1e-12, tang / np.maximum(tl, 1e-300), 0)
    din = -np.cos(tt)[..., None] * n1 + np.sin(tt)[..., None] * tang
    chord = 2 * R * np.cos(tt)
    p2 = p1 + chord[..., None] * din
    n2 = p2 / R
    tang2 = din - (din * n2).sum(-1, keepdims=True) * n2
    tl = np.linalg.norm(tang2, axis=-1, keepdims=True)
    tang2 = np.where(tl > 1e-12, tang2 / np.maximum(tl, 1e-300), 0)
    dout = np.cos(ti)[..., None] * n2 + np.sin(ti)[..., None] * tang2
    # the wall: the near root of |p2 + t dout - Cw| = Rw for a unit dout
    oc = p2 - Cw
    hb = (oc * dout).sum(-1)
    disc = hb * hb - ((oc * oc).sum(-1) - Rw * Rw)
    t3 = -hb - np.sqrt(np.maximum(disc, 0))
    p3 = p2 + t3[..., None] * dout
    n3 = (p3 - Cw) / Rw
    # (index 2 turns a ray that enters near the rim by up to 120 degrees: those leave into the sky)
    m = through & (disc > 0) & (t3 > 0)
    lost = through & ~m
    assert m.sum() > 50 and lost.sum() > 0
    assert (chains[m][:, 0] == [0, 0, 1]).all() and (bounces[m] == 2).all()
    assert (chains[lost][:, 0] == [0, 0, follow_ref.SKY]).all() and (bounces[lost] == -1).all()
    assert (got[lost][:, :8] == 0).all() and (got[lost][:, 8:11] == 1).all() and (got[lost][:, 11] == 0).all()
    assert (got[..., 11][m] == 2).all() and (got[..., 7][m] == 1).all()
    assert np.abs(got[..., 4:7] - p3)[m].max() <= 1e-9
    assert np.abs(got[..., 0:3] - n3)[m].max() <= 1e-9
    assert np.abs(got[..., 3] - (t1 + chord + t3))[m].max() <= 1e-9
    glass, wall = np.array(scn.spheres[0].color), np.array(scn.spheres[1].color)
    assert np.abs(got[..., 8:11][m] - glass * glass * wall).max() <= 1e-15
    # beside the ball: the wall directly, no bounce
    assert (got[..., 11][~through] == 0).all() and (chains[~through][:, 0, 0] == 1).all()


# ---- the cap ------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_facing_mirrors_stop_at_the_cap(dtype):
    W, H, B = 24, 18, 3
    scn, cam = follow_scenes.facing_mirrors(W, H)
    got, chains, bounces, _ = follow_ref.follow(scn, cam, W, H, 2, B, dtype)
    assert (bounces == B).all() and (chains == [1, 0, 1, 0]).all()
    assert (got[..., 11] == B).all() and (got[..., 7] == 1).all()
    assert np.allclose(got[..., 8:11], 0.9 ** 4)  # T of three bounces times the last mirror's colour
    assert (np.abs(got[..., 0]) > 0.99).all()  # a mirror's normal


# ---- float32 against float64: the exclusion rule ---------------------------------------
@pytest.mark.parametrize("nsub", [1, 2])
@pytest.mark.parametrize("name,W,H", follow_scenes.GPU_CASES)
def test_float32_takes_the_float64_chain_outside_the_margin(name, W, H, nsub):
    """On every GPU case, at the largest B (its chains contain those of the
    smaller ones): every ray whose float64 margin is at least 1e-4 takes the
    same chain in float32, and the rays below exclude at most 2 % of the
    pixels."""
    B = max(follow_scenes.BOUNCES)
    scn, cam = follow_scenes.scene_and_camera(name, W, H)
    f64, c64, b64, margin = follow_ref.follow(scn, cam, W, H, nsub, B, np.float64)
    f32, c32, b32, _ = follow_ref.follow(scn, cam, W, H, nsub, B, np.float32)
    keep_ray = margin >= follow_scenes.MARGIN
    same = (c64 == c32).all(-1) & (b64 == b32)
    excluded = 1.0 - keep_ray.all(-1).mean()
    print(f"{name} nsub {nsub}: excluded pixels {excluded:.4f}, rays off the float64 chain "
          f"{(~same).sum()} (kept: {(~same & keep_ray).sum()}), max bounces taken {b64.max()}")
    assert same[keep_ray].all()
    assert excluded <= follow_scenes.MAX_EXCLUDED
    keep = keep_ray.all(-1)
    assert np.array_equal(f32[..., 7][keep], f64[..., 7][keep].astype(np.float32))
    assert np.array_equal(f32[..., 11][keep], f64[..., 11][keep].astype(np.float32))


# ---- the ABI ---------------------------------------------------------------------------
def _header():
    with open(os.path.join(ROOT, "include", "ptgpu.h")) as f:
        return f.read()


def test_denoise_params_keep_their_layout():
    text = _header()
    body = re.search(r"typedef struct ptg_denoise_params \{(.*?)\} ptg_denoise_params;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(int32_t|float)\s+(\w+)(?:\[(\d+)\])?;", body)
    ctype = {"int32_t": C.c_int32, "float": C.c_float}
    want = [(n, ctype[t] * int(k) if k else ctype[t]) for t, n, k in fields]
    assert [n for n, _ in want] == ["iterations", "follow_bounces", "k_color", "k_normal", "k_plane", "k_albedo",
                                    "eps_color", "pixel_spread", "reserved_"]
    Header = type("Header", (C.Structure,), {"_fields_": want})
    assert C.sizeof(Header) == C.sizeof(ptgpu.DenoiseParams) == 64
    for n, _ in want:
        assert getattr(Header, n).offset == getattr(ptgpu.DenoiseParams, n).offset, n
    assert ptgpu.DenoiseParams.follow_bounces.offset == 4 and ptgpu.DenoiseParams.k_color.offset == 8
    assert int(re.search(r"#define PTG_ABI_VERSION (\d+)", text).group(1)) == 2 == ptgpu.ABI_VERSION
    assert int(re.search(r"#define PTG_MAX_FOLLOW_BOUNCES (\d+)", text).group(1)) == 16
    for name in ("ptg_features_follow_device", "ptg_features_follow"):
        assert re.search(rf"^int {name}\(", text, re.M), name


def test_defaults_do_not_follow():
    k = ptgpu.denoise_defaults()
    assert k.follow_bounces == 0 and k.iterations == 5


def test_filter_entry_points_ignore_follow_bounces():
    c, v, f = denoise_ref.seeded_frame(8, 5, 3)
    k = ptgpu.denoise_defaults()
    want = ptgpu.denoise_host(c, v, f, k)
    k.follow_bounces = 99
    assert np.array_equal(ptgpu.denoise_host(c, v, f, k), want)


@pytest.mark.parametrize("bounces", [-1, 17])
def test_bounces_out_of_range_are_refused_before_the_device(bounces):
    L = ptgpu.lib()
    p = ptgpu.make_params(8, 8, 4, 2)
    buf = np.zeros(8 * 8 * 12, dtype=np.float32)
    # (no context: the range check comes first, and names the argument)
    assert L.ptg_features_follow_device(None, C.byref(p), bounces, buf.ctypes.data_as(C.c_void_p), None) == -1
    assert b"max_bounces" in L.ptg_last_error()
    scn = ptgpu.make_scene("box", 8, 8)
    sp, ca = scn.to_array(), ptgpu.camera.with_config(scn.camera_parameters).to_array()
    assert L.ptg_features_follow(sp.ctypes.data_as(C.c_void_p), len(sp), ca.ctypes.data_as(C.c_void_p), C.byref(p), 0,
                                 bounces, buf.ctypes.data_as(C.c_void_p)) == -1
    assert b"max_bounces" in L.ptg_last_error()
    assert (buf == 0).all()
