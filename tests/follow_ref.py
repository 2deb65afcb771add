"""ptg_features_follow_device's definition (include/ptgpu.h "denoising")
restated in numpy, in float64 or float32, on tests/denoise_ref.first_hit's
conventions: the same camera rays, the same quadratic per sphere (sphere.cpp's
form in float64; in float32 the anchored form for the huge spheres and the
cancellation-free roots), closest root >= eps, strict < in scene order.  Every
segment of a ray runs that scan from the previous hit point.  A restatement
vectorised over the image, not a transcription of the kernel.

Besides the frame it returns, per ray, the chain of sphere ids and a decision
margin (meaningful in the float64 run, which is the only one the tests read it
from): the smallest, over the chain's segments, of
  * the relative gap between the winning root and the next candidate root of
    another sphere (inf when there is none);
  * |disc| / hb^2 of every sphere whose hit / miss decision the segment's
    result rests on: the winner's, and that of every sphere the ray misses
    whose closest approach -hb / a lies in [eps, the winning root) -- a miss
    further along than the winner, or a hit that does not win, changes nothing
    by flipping;
  * for a followed dielectric, |ratio sin(theta) - 1|.
A ray whose margin is small may take another chain in another arithmetic; the
tests exclude such rays by this number, never by looking at the kernel."""
import numpy as np

from denoise_ref import EPS, INF

DIFFUSE, SPECULAR, DIELECTRIC = 0, 1, 2
SKY, PAD = -1, -2  # chain entries: the ray left into the sky; no segment


def _dot(a, b):
    return (a * b).sum(-1)


def _scan(sp, anchors, o, d, dtype, want_margin):
    """Nearest root >= eps of every ray (o, d: [..., 3]) over the spheres in
    scene order: (root, winner id or -1, margin)."""
    T = np.dtype(dtype).type
    shape = d.shape[:-1]
    a = _dot(d, d)
    best = np.full(shape, T(INF))
    second = np.full(shape, T(INF))
    win = np.full(shape, -1, dtype=np.int64)
    dmargin = np.full(shape, np.inf)
    dms, tcas = [], []
    for i, s in enumerate(sp):
        R = T(s["radius"])
        if dtype == np.float32 and s["radius"] >= 100.0:
            A, n0 = anchors[i]
            e = o - A
            hb = _dot(e, d) + R * _dot(d, n0)
            c = _dot(e, e) + T(2) * R * _dot(e, n0)
        else:
            oc = o - s["position"].astype(dtype)
            hb = _dot(oc, d)
            c = _dot(oc, oc) - R * R
        disc = hb * hb - a * c
        ok = disc >= 0
        sq = np.sqrt(np.where(ok, disc, 0))
        if dtype == np.float32:
            qq = sq + np.abs(hb)
            with np.errstate(divide="ignore", invalid="ignore"):
                r1 = np.where(hb >= 0, -qq / a, c / qq)
                r2 = np.where(hb >= 0, -c / qq, qq / a)
        else:
            r1, r2 = (-hb - sq) / a, (-hb + sq) / a
        root = np.where(r1 < T(EPS), r2, r1)
        ok &= root >= T(EPS)
        take = ok & (root < best)
        if want_margin:
            # the runner-up among the other spheres' roots
            second = np.where(take, best, np.where(ok & (root < second), root, second))
            with np.errstate(divide="ignore", invalid="ignore"):
                dm = np.abs(disc) / (hb * hb)
            dms.append(np.where(np.isfinite(dm), dm, np.inf))
            tcas.append(np.where(disc < 0, -hb / a, np.inf))
        best = np.where(take, root, best)
        win = np.where(take, i, win)
    margin = dmargin
    if want_margin:
        for i in range(len(sp)):
            counts = (win == i) | ((tcas[i] >= T(EPS)) & (tcas[i] < best))
            margin = np.minimum(margin, np.where(counts, dms[i], np.inf))
        hit = win >= 0
        with np.errstate(invalid="ignore", over="ignore"):
            gap = np.where(hit & (second < T(INF)), (second - best) / best, np.inf)
        margin = np.minimum(margin, gap)
    return best, win, margin


def follow(scn, cam, W, H, nsub, max_bounces, dtype=np.float64):
    """(feat [H, W, 12], chains [H, W, nsub^2, max_bounces + 1], bounces
    [H, W, nsub^2] (-1: sky), margin [H, W, nsub^2]) in slab row order (row r
    is image row y = H - 1 - r)."""
    T = np.dtype(dtype).type
    sp = scn.to_array()
    ca = cam.to_array()[0]
    pos = ca["position"].astype(dtype)
    base = (ca["lower_left_corner"] - ca["position"]).astype(dtype)
    X, Y = ca["cam_x_axis"].astype(dtype), ca["cam_y_axis"].astype(dtype)
    anchors = {}
    for i, s in enumerate(sp):  # (denoise_ref.first_hit's anchor: the surface point facing the camera)
        if s["radius"] >= 100.0:
            n0 = ca["position"] - s["position"]
            n0 = n0 / np.linalg.norm(n0)
            anchors[i] = ((s["position"] + s["radius"] * n0).astype(dtype), n0.astype(dtype))
    rows, xs = np.mgrid[0:H, 0:W]
    ys = H - 1 - rows
    want_margin = dtype == np.float64
    nray = nsub * nsub
    chains = np.full((H, W, nray, max_bounces + 1), PAD, dtype=np.int64)
    bounces = np.full((H, W, nray), -1, dtype=np.int64)
    margins = np.full((H, W, nray), np.inf)
    acc_n = np.zeros((H, W, 3), dtype=dtype)
    acc_P = np.zeros((H, W, 3), dtype=dtype)
    acc_a = np.zeros((H, W, 3), dtype=dtype)
    acc_z = np.zeros((H, W), dtype=dtype)
    acc_b = np.zeros((H, W), dtype=dtype)
    hits = np.zeros((H, W), dtype=dtype)
    for sy in range(nsub):
        for sx in range(nsub):
            k = sy * nsub + sx
            fs = ((xs + (sx + 0.5) / nsub) / W).astype(dtype)
            ft = ((ys + (sy + 0.5) / nsub) / H).astype(dtype)
            d = base + fs[..., None] * X + ft[..., None] * Y
            o = np.broadcast_to(pos, d.shape).copy()
            Tr = np.ones((H, W, 3), dtype=dtype)
            zr = np.zeros((H, W), dtype=dtype)
            live = np.ones((H, W), dtype=bool)
            for b in range(max_bounces + 1):
                if not live.any():
                    break
                best, win, mg = _scan(sp, anchors, o, d, dtype, want_margin)
                margins[..., k] = np.where(live, np.minimum(margins[..., k], mg), margins[..., k])
                h = live & (win >= 0)
                chains[..., k, b] = np.where(live, np.where(h, win, SKY), chains[..., k, b])
                w = np.maximum(win, 0)
                C = sp["position"][w].astype(dtype)
                col = sp["color"][w].astype(dtype)
                mat = sp["material"][w]
                p = o + best[..., None] * d
                on = (p - C) / sp["radius"][w].astype(dtype)[..., None]
                front = _dot(on, d) < 0
                nn = np.where(front[..., None], on, -on)
                zr = np.where(h, zr + best * np.sqrt(_dot(d, d)), zr)
                stop = h & ((mat == DIFFUSE) | (b == max_bounces))
                m = stop[..., None]
                acc_n += np.where(m, nn, 0)
                acc_P += np.where(m, p, 0)
                acc_a += np.where(m, Tr * col, 0)
                acc_z += np.where(stop, zr, 0)
                acc_b += np.where(stop, b, 0)
                hits += stop
                bounces[..., k] = np.where(stop, b, bounces[..., k])
                go = h & ~stop
                # the next direction: mirror, or Snell with total internal reflection
                v1 = d / np.sqrt(_dot(d, d))[..., None]
                cth = np.minimum(T(1), -_dot(v1, nn))
                s2 = np.sqrt(np.maximum(T(0), T(1) - cth * cth))
                ratio = np.where(front, T(0.5), T(2))
                glass = go & (mat == DIELECTRIC)
                if want_margin:
                    margins[..., k] = np.where(glass, np.minimum(margins[..., k], np.abs(ratio * s2 - 1)),
                                               margins[..., k])
                refract = glass & ~(ratio * s2 > T(1))
                perp = (nn * cth[..., None] + v1) * ratio[..., None]
                s3 = np.sqrt(np.abs(T(1) - _dot(perp, perp)))
                d_refr = perp - nn * s3[..., None]
                d_refl = d - (T(2) * _dot(on, d))[..., None] * on
                d = np.where(go[..., None], np.where(refract[..., None], d_refr, d_refl), d)
                o = np.where(go[..., None], p, o)
                Tr = np.where(go[..., None], Tr * col, Tr)
                live = go
    feat = np.zeros((H, W, 12), dtype=dtype)
    kk = np.maximum(hits, 1)[..., None]
    feat[..., 0:3] = acc_n / kk
    feat[..., 3] = acc_z / kk[..., 0]
    feat[..., 4:7] = acc_P / kk
    feat[..., 7] = hits / T(nray)
    feat[..., 8:11] = np.where((hits > 0)[..., None], acc_a / kk, 1)
    feat[..., 11] = acc_b / kk[..., 0]
    return feat, chains, bounces, margins


def followed_differences(f, g, keep):
    """Over the pixels `keep` that stop somewhere: the largest |dn|, |dz| / z,
    |dP| / |P| and |d albedo| between two frames."""
    m = keep & (g[..., 7] > 0)
    out = {"n": 0.0, "z": 0.0, "P": 0.0, "a": 0.0}
    if m.any():
        a, b = f[m].astype(np.float64), g[m].astype(np.float64)
        out["n"] = float(np.abs(a[:, 0:3] - b[:, 0:3]).max())
        out["z"] = float((np.abs(a[:, 3] - b[:, 3]) / b[:, 3]).max())
        out["P"] = float((np.linalg.norm(a[:, 4:7] - b[:, 4:7], axis=1) / np.linalg.norm(b[:, 4:7], axis=1)).max())
        out["a"] = float(np.abs(a[:, 8:11] - b[:, 8:11]).max())
    return out
