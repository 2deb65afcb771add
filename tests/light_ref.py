"""PTG_FLAG_LIGHT_SAMPLING's estimator (include/ptgpu.h) and the path tracer
around it (the oracle's Mode A/xs: sphere.cpp's quadratic, the strict-<
linear scan, main.cpp's samplers and radiance loop, the counter RNG) restated
in numpy in any float dtype, vectorised over paths.  In float64 it follows the
oracle's per-path entry point (tests/test_oracle_light_sampling.py compares
them); in float32 every step is rounded to float, which is the yardstick for
what an fp32 implementation of the same definition may differ by
(tests/test_gpu_light_sampling.py, the per-path test).  A restatement, not a
transcription: numpy's own order inside a dot product, its sin / cos / power.
"""
import numpy as np

EPS, INF, DEPTH_LIMIT, RR_THRESHOLD = 1e-4, 1e20, 100, 4


def _mix64(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def sample_states(W, nsub, seed, coords):
    """The counter RNG's xorshift32 state of each record {x, y, sx, sy, sample} (DESIGN.md "RNG")."""
    c = np.asarray(coords).astype(np.uint64)
    x, y, sx, sy, k = (c[:, i] for i in range(5))
    ps = (y * np.uint64(W) + x) * np.uint64(nsub * nsub) + (sy * np.uint64(nsub) + sx)
    key = _mix64(np.uint64(seed) ^ _mix64(ps + np.uint64(1)))
    st = (_mix64(key + (k + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(32)).astype(np.uint32)
    return np.where(st == 0, np.uint32(0x6D2B79F5), st)


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _norm(a):
    return a * (a.dtype.type(1) / np.sqrt(_dot(a, a)))[..., None]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _basis(w):
    """main.cpp:52: u = norm((|w.x| > 0.1 ? y : x) x w), v = w x u."""
    T = w.dtype.type
    up = np.where((np.abs(w[:, 0]) > T(0.1))[:, None], np.array([0, 1, 0], dtype=w.dtype),
                  np.array([1, 0, 0], dtype=w.dtype))
    u = _norm(_cross(up, w))
    return u, _cross(w, u)


def trace(spheres, cam, W, H, nsub, seed, coords, lights, dtype):
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return _trace(spheres, cam, W, H, nsub, seed, coords, lights, dtype)


def _trace(spheres, cam, W, H, nsub, seed, coords, lights, dtype):
    """The radiance (n x 3, dtype) and the segment count (n) of each path
    record {x, y, sx, sy, sample} (y from the bottom), with the light list
    `lights` (scene indices; empty: the plain estimator).  spheres / cam: the
    oracle's structured arrays."""
    T = np.dtype(dtype).type
    coords = np.asarray(coords)
    n = len(coords)
    C = spheres["position"].astype(dtype)
    R2 = (spheres["radius"].astype(dtype)) ** 2
    Le, col, mat = spheres["emission"].astype(dtype), spheres["color"].astype(dtype), spheres["material"]
    on_list = np.zeros(len(spheres), dtype=bool)
    on_list[list(lights)] = True
    lights = np.asarray(list(lights), dtype=np.int64)
    L = len(lights)
    st = sample_states(W, nsub, seed, coords)

    def draw(idx):
        x = st[idx]
        x ^= x << np.uint32(13)
        x ^= x >> np.uint32(17)
        x ^= x << np.uint32(5)
        st[idx] = x
        return (x >> np.uint32(8)).astype(dtype) * T(2.0 ** -24)

    def scan(o, d):
        """Nearest hit of each ray over all spheres in index order: (t, id), id -1 on a miss."""
        oc = o[:, None, :] - C[None, :, :]
        a = _dot(d, d)[:, None]
        hb = _dot(oc, d[:, None, :])
        c = _dot(oc, oc) - R2[None, :]
        disc = hb * hb - a * c
        sq = np.sqrt(np.maximum(disc, T(0)))
        r0, r1 = (-hb - sq) / a, (-hb + sq) / a
        root = np.where(r0 < T(EPS), r1, r0)
        root = np.where((disc < 0) | (root < T(EPS)), T(INF), root)
        root = np.where(root < T(INF), root, T(INF))
        idn = np.argmin(root, axis=1)  # the first of equal minima: the lowest index, like the strict <
        t = root[np.arange(len(o)), idn]
        return t, np.where(t < T(INF), idn, -1)

    camv = {k: np.asarray(cam[k][0], dtype=dtype) for k in ("position", "lower_left_corner", "cam_x_axis",
                                                           "cam_y_axis")}
    lens = T(cam["lens_radius"][0])
    everyone = np.arange(n)
    sl = T(1) / T(nsub)
    xin = coords[:, 0].astype(dtype) + coords[:, 2].astype(dtype) * sl + (T(0) + (sl - T(0)) * draw(everyone))
    yin = coords[:, 1].astype(dtype) + coords[:, 3].astype(dtype) * sl + (T(0) + (sl - T(0)) * draw(everyone))
    s, t = xin / T(W), yin / T(H)
    disk = np.zeros((n, 3), dtype=dtype)
    todo = everyone
    while len(todo):  # camera.cpp:19-30
        px = T(-1) + T(2) * draw(todo)
        py = T(-1) + T(2) * draw(todo)
        disk[todo, 0], disk[todo, 1] = px, py
        todo = todo[px * px + py * py + T(0) >= T(1)]
    rd = disk * lens
    off = rd * s[:, None] + rd * t[:, None]
    d = (camv["lower_left_corner"] + camv["cam_x_axis"] * s[:, None] + camv["cam_y_axis"] * t[:, None]
         - camv["position"] - off)
    o = camv["position"] + off

    E = np.zeros((n, 3), dtype=dtype)
    Tp = np.ones((n, 3), dtype=dtype)
    segs = np.zeros(n, dtype=np.int64)
    sampled = np.zeros(n, dtype=bool)
    alive = everyone
    for depth in range(DEPTH_LIMIT):
        if not len(alive):
            break
        segs[alive] += 1
        oa, da = o[alive], d[alive]
        th, idh = scan(oa, da)
        miss = idh < 0
        if miss.any():  # main.cpp:115-120
            m = alive[miss]
            tt = T(0.5) * (_norm(da[miss])[:, 1] + T(1))
            bg = (T(1) - tt)[:, None] * np.ones(3, dtype=dtype) + tt[:, None] * np.array([0.5, 0.7, 1.0], dtype=dtype)
            E[m] = E[m] + Tp[m] * bg
        keep = ~miss
        alive, oa, da, th, idh = alive[keep], oa[keep], da[keep], th[keep], idh[keep]
        if not len(alive):
            break
        p = oa + da * th[:, None]
        on = _norm(p - C[idh])
        front = _dot(on, da) < 0
        nn = np.where(front[:, None], on, -on)
        skip = sampled[alive] & front & on_list[idh]  # step 4: a listed emitter's front face after a step
        E[alive] = E[alive] + np.where(skip[:, None], T(0), Tp[alive] * Le[idh])
        sampled[alive] = False
        color = col[idh]
        pr = color.max(axis=1)
        going = np.ones(len(alive), dtype=bool)
        if depth > RR_THRESHOLD:
            u = draw(alive)
            going = u < pr
            color = np.where(going[:, None], color * (T(1) / np.where(going, pr, T(1)))[:, None], color)
        alive, p, on, nn, front, da, idh, color = (a[going] for a in (alive, p, on, nn, front, da, idh, color))
        if not len(alive):
            break
        Tp[alive] = Tp[alive] * color
        m = mat[idh]
        nd = np.zeros_like(da)
        # ---- diffuse (main.cpp:44-58), the light-sampling step first
        di = np.nonzero(m == 0)[0]
        if len(di):
            g = alive[di]
            if L > 0 and depth + 1 < DEPTH_LIMIT:
                k = np.zeros(len(g), dtype=np.int64)
                if L > 1:
                    k = np.minimum(L - 1, np.floor(draw(g) * T(L)).astype(np.int64))
                u1, u2 = draw(g), draw(g)
                lid = lights[k]
                w = C[lid] - p[di]
                d2 = _dot(w, w)
                ok = (d2 > R2[lid]) & (idh[di] != lid)
                q = np.where(ok, R2[lid] / d2, T(0.5))
                omc = q / (T(1) + np.sqrt(T(1) - q))
                a = u1 * omc
                ct, sn, ph = T(1) - a, np.sqrt(a * (T(2) - a)), T(2 * np.pi) * u2
                sw = _norm(w)
                su, sv = _basis(sw)
                l = su * (np.cos(ph) * sn)[:, None] + sv * (np.sin(ph) * sn)[:, None] + sw * ct[:, None]
                cs = _dot(nn[di], l)
                ok &= cs > 0
                if ok.any():
                    segs[g[ok]] += 1
                    _, winner = scan(p[di][ok], l[ok])
                    lit = winner == lid[ok]
                    gl = g[ok][lit]
                    E[gl] = E[gl] + (Tp[gl] * Le[lid[ok][lit]]) * (cs[ok][lit] * T(2) * omc[ok][lit] * T(L))[:, None]
                sampled[g] = True
            phi = T(2 * np.pi) * draw(g)
            ra = draw(g)
            sth, cth = np.sqrt(ra), np.sqrt(T(1) - ra)
            bu, bv = _basis(nn[di])
            nd[di] = _norm(bu * (np.cos(phi) * sth)[:, None] + bv * (np.sin(phi) * sth)[:, None]
                           + nn[di] * cth[:, None])
        # ---- dielectric (main.cpp:69-97): reflect (then as a mirror) or refract
        reflect = m == 1
        gi = np.nonzero(m == 2)[0]
        if len(gi):
            ratio = np.where(front[gi], T(0.5), T(2))
            ud = _norm(da[gi])
            ct = np.minimum(T(1), _dot(-ud, nn[gi]))
            sth = np.sqrt(T(1) - ct * ct)
            refl = ratio * sth > T(1)
            r0 = ((T(1) - ratio) / (T(1) + ratio)) ** 2
            fres = r0 + (T(1) - r0) * np.power(T(1) - ct, T(5))
            free = np.nonzero(~refl)[0]  # (|| short-circuits the Fresnel draw)
            if len(free):
                refl[free] = fres[free] > draw(alive[gi][free])
            perp = (ud + nn[gi] * ct[:, None]) * ratio[:, None]
            par = nn[gi] * (-np.sqrt(np.abs(T(1) - _dot(perp, perp))))[:, None]
            nd[gi] = perp + par
            reflect[gi] = refl
        # ---- mirror (main.cpp:60-67): the fuzz draw is consumed and multiplied by 0
        ri = np.nonzero(reflect)[0]
        if len(ri):
            f = draw(alive[ri]) * T(0)
            nd[ri] = da[ri] - (on[ri] * T(2)) * _dot(on[ri], da[ri])[:, None] + f[:, None]
        o[alive], d[alive] = p, nd
    return E, segs
