"""The a-trous filter's definition (include/ptgpu.h "denoising") restated in
numpy, in any float dtype, and seeded frames for the tests that need inputs
without the C++ check program.  Vectorised over the image: the sums over the
25 taps are taken tap by tap in the definition's (dy, dx) order, everything
else in numpy's own order -- a restatement, not a transcription."""
import numpy as np

H5 = (1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16)
Z_MIN = 1e-4


def _shift(a, dx, dy, fill=0):
    """out[y, x] = a[y + dy, x + dx] where that is inside, else fill."""
    H, W = a.shape[:2]
    out = np.full_like(a, fill)
    ys, ye = max(0, -dy), min(H, H - dy)
    xs, xe = max(0, -dx), min(W, W - dx)
    if ys < ye and xs < xe:
        out[ys:ye, xs:xe] = a[ys + dy:ye + dy, xs + dx:xe + dx]
    return out


def vbar(var):
    H, W = var.shape[:2]
    t = var.sum(axis=2)
    p = np.pad(t, 1, mode="edge")
    acc = np.zeros_like(t)
    for dy, ky in zip((0, 1, 2), (1, 2, 1)):
        for dx, kx in zip((0, 1, 2), (1, 2, 1)):
            acc = acc + t.dtype.type(ky * kx / 16) * p[dy:dy + H, dx:dx + W]
    return acc


def denoise(color, var, feat, k, dtype=np.float64, return_var=True):
    """k: an object with iterations, k_color, k_normal, k_plane, k_albedo,
    eps_color, pixel_spread (ptgpu.DenoiseParams)."""
    T = np.dtype(dtype).type
    c, v, f = (np.asarray(a, dtype=dtype) for a in (color, var, feat))
    H, W = c.shape[:2]
    n, z, P, hit, alb = f[..., 0:3], f[..., 3], f[..., 4:7], f[..., 7], f[..., 8:11]
    inside = np.ones((H, W), dtype=bool)
    kc, kn, kp, ka, eps, spread = (T(getattr(k, a)) for a in ("k_color", "k_normal", "k_plane", "k_albedo",
                                                            "eps_color", "pixel_spread"))
    for it in range(k.iterations):
        s = 1 << it
        vb = vbar(v)
        sw = np.zeros((H, W), dtype=dtype)
        sc = np.zeros((H, W, 3), dtype=dtype)
        sv = np.zeros((H, W, 3), dtype=dtype)
        zden = T(s) * spread * np.maximum(z, T(Z_MIN))
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                ok = _shift(inside, s * dx, s * dy, False)
                if not ok.any():
                    continue
                cq, vq, vbq = (_shift(a, s * dx, s * dy) for a in (c, v, vb))
                nq, Pq, hq, aq = (_shift(a, s * dx, s * dy) for a in (n, P, hit, alb))
                x = kc * ((c - cq) ** 2).sum(axis=2) / (vb + vbq + eps)
                geo = kn * np.maximum(T(0), T(1) - (n * nq).sum(axis=2))
                geo = geo + kp * np.abs((n * (Pq - P)).sum(axis=2)) / zden
                geo = geo + ka * ((alb - aq) ** 2).sum(axis=2)
                geo = geo + kn * np.abs(hit - hq)
                sky_p, sky_q = hit == 0, hq == 0
                x = np.where(sky_p, x, x + geo)
                if dx == 0 and dy == 0:
                    x = np.zeros_like(x)  # the centre tap by definition
                t = np.maximum(T(0), T(1) - x / T(8))
                w = T(H5[dx + 2] * H5[dy + 2]) * ((t * t) ** 2) ** 2
                w = np.where(ok & (sky_p == sky_q), w, T(0))
                sw = sw + w
                sc = sc + w[..., None] * cq
                sv = sv + (w * w)[..., None] * vq
        assert (sw > 0).all()
        c = sc / sw[..., None]
        v = sv / (sw * sw)[..., None]
    return (c, v) if return_var else c


def seeded_frame(W, H, seed):
    """Colour, variance and features [H, W, .] float32 of a frame with three
    vertical bands on different planes, a sky strip at the top and silhouette
    columns of fractional hit -- every term of the weight is at work."""
    r = np.random.default_rng(seed)
    bands = 3
    nrm = r.standard_normal((bands, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    alb = 0.25 + 0.5 * r.integers(0, 2, (bands, 3))
    base = r.random((bands, 3))
    depth = 2 + 6 * r.random(bands)
    yy, xx = np.mgrid[0:H, 0:W]
    b = (xx * bands) // W
    sky = yy * 6 < H
    edge = ~sky & (xx > 0) & (((xx - 1) * bands) // W != b)
    sd = 0.02 + 0.1 * r.random((H, W, 1))
    color = np.where(sky[..., None], 0.6, base[b]) + sd * (r.random((H, W, 3)) - 0.5)
    var = sd * sd / 12 * (0.5 + r.random((H, W, 3)))
    feat = np.zeros((H, W, 12))
    z = depth[b] + 0.01 * xx + 0.02 * yy
    feat[..., 0:3] = nrm[b] * np.where(edge, 0.9, 1.0)[..., None]
    feat[..., 3] = z
    feat[..., 4] = 0.01 * xx * z
    feat[..., 5] = 0.01 * yy * z
    feat[..., 6] = -z
    feat[..., 7] = np.where(edge, 0.25 * r.integers(1, 4, (H, W)), 1.0)
    feat[..., 8:11] = alb[b]
    feat[sky] = 0
    feat[sky, 8:11] = 1
    return tuple(np.ascontiguousarray(a, dtype=np.float32) for a in (color, var, feat))


# ---- first-hit features (ptg_features_device) restated -----------------
EPS, INF = 1e-4, 1e20  # constants.hpp


def first_hit(scn, cam, W, H, nsub, dtype=np.float64):
    """Per-pixel features [H, W, 12] in slab row order (row r is image row
    y = H - 1 - r) and the per-ray winner ids [H, W, nsub^2] (-1: sky), from
    camera rays through the sub-pixel centres (ptgpu/scene.py's camera, no
    lens offset) and sphere.cpp's quadratic over all spheres, closest root
    >= eps, strict < (main.cpp:30-42), all in `dtype`.

    In float32 the spheres of radius >= 100 take the same equation about the
    surface point facing the camera, A = C + R n0: with e = o - A,
    half_b = e.d + R (n0.d) and c = e.e + 2 R (e.n0) -- sphere.cpp's c =
    |o - C|^2 - R^2 cancels to nothing in fp32 at R = 1e6, which no fp32
    code can use -- and the roots as c / qq and qq / a with qq = sqrt(disc) +
    |half_b|, the same two numbers without the cancellation of -half_b -+ sqrt."""
    T = np.dtype(dtype).type
    sp = scn.to_array()
    ca = cam.to_array()[0]
    pos = ca["position"].astype(dtype)
    base = (ca["lower_left_corner"] - ca["position"]).astype(dtype)
    X, Y = ca["cam_x_axis"].astype(dtype), ca["cam_y_axis"].astype(dtype)
    rows, xs = np.mgrid[0:H, 0:W]
    ys = H - 1 - rows
    feat = np.zeros((H, W, 12), dtype=dtype)
    ids = np.full((H, W, nsub * nsub), -1, dtype=np.int64)
    acc_n = np.zeros((H, W, 3), dtype=dtype)
    acc_P = np.zeros((H, W, 3), dtype=dtype)
    acc_a = np.zeros((H, W, 3), dtype=dtype)
    acc_z = np.zeros((H, W), dtype=dtype)
    hits = np.zeros((H, W), dtype=dtype)
    for sy in range(nsub):
        for sx in range(nsub):
            fs = ((xs + (sx + 0.5) / nsub) / W).astype(dtype)
            ft = ((ys + (sy + 0.5) / nsub) / H).astype(dtype)
            d = base + fs[..., None] * X + ft[..., None] * Y
            a = (d * d).sum(-1)
            best = np.full((H, W), T(INF))
            win = np.full((H, W), -1, dtype=np.int64)
            for i, s in enumerate(sp):
                R = T(s["radius"])
                if dtype == np.float32 and s["radius"] >= 100.0:
                    n0 = ca["position"] - s["position"]
                    n0 = n0 / np.linalg.norm(n0)
                    A = (s["position"] + s["radius"] * n0).astype(dtype)
                    n0 = n0.astype(dtype)
                    e = pos - A
                    hb = (e * d).sum(-1) + R * (d * n0).sum(-1)
                    c = (e * e).sum() + T(2) * R * (e * n0).sum()
                else:
                    oc = pos - s["position"].astype(dtype)
                    hb = (oc * d).sum(-1)
                    c = (oc * oc).sum() - R * R
                disc = hb * hb - a * c
                ok = disc >= 0
                sq = np.sqrt(np.where(ok, disc, 0))
                if dtype == np.float32:  # the same roots without the cancellation of -hb -+ sq
                    qq = sq + np.abs(hb)
                    r1 = np.where(hb >= 0, -qq / a, c / qq)
                    r2 = np.where(hb >= 0, -c / qq, qq / a)
                else:
                    r1, r2 = (-hb - sq) / a, (-hb + sq) / a
                root = np.where(r1 < T(EPS), r2, r1)
                ok &= root >= T(EPS)
                take = ok & (root < best)
                best = np.where(take, root, best)
                win = np.where(take, i, win)
            ids[..., sy * nsub + sx] = win
            h = win >= 0
            w = np.maximum(win, 0)
            C = sp["position"][w].astype(dtype)
            p = pos + best[..., None] * d
            on = (p - C) / sp["radius"][w].astype(dtype)[..., None]
            nn = np.where(((on * d).sum(-1) < 0)[..., None], on, -on)
            m = h[..., None]
            acc_n += np.where(m, nn, 0)
            acc_P += np.where(m, p, 0)
            acc_a += np.where(m, sp["color"][w].astype(dtype), 0)
            acc_z += np.where(h, best * np.sqrt(a), 0)
            hits += h
    k = np.maximum(hits, 1)[..., None]
    feat[..., 0:3] = acc_n / k
    feat[..., 3] = acc_z / k[..., 0]
    feat[..., 4:7] = acc_P / k
    feat[..., 7] = hits / T(nsub * nsub)
    feat[..., 8:11] = np.where((hits > 0)[..., None], acc_a / k, 1)
    return feat, ids


def feature_differences(f, g):
    """Where two feature frames agree in hit and albedo: the largest |dn|,
    |dz| / z and |dP| / |P| (0 if nothing agrees); and the fraction of the
    pixels whose hit differs."""
    same_hit = f[..., 7] == g[..., 7]
    agree = same_hit & (np.abs(f[..., 8:11] - g[..., 8:11]).max(-1) <= 1e-6) & (f[..., 7] > 0)
    out = {"hit_differs": 1.0 - same_hit.mean(), "n": 0.0, "z": 0.0, "P": 0.0, "agree": agree}
    if agree.any():
        a, b = f[agree].astype(np.float64), g[agree].astype(np.float64)
        out["n"] = float(np.abs(a[:, 0:3] - b[:, 0:3]).max())
        out["z"] = float((np.abs(a[:, 3] - b[:, 3]) / b[:, 3]).max())
        out["P"] = float((np.linalg.norm(a[:, 4:7] - b[:, 4:7], axis=1) / np.linalg.norm(b[:, 4:7], axis=1)).max())
    return out
