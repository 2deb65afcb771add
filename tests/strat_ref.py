"""PTG_FLAG_STRATIFIED's sampler (include/ptgpu.h "Stratified sampling",
csrc/sobol_pairs.hpp) restated in numpy, and the path tracer with the replaced
draws: tests/light_ref.py's restatement (its helpers, its operations in its
order) in which pair 0 is the sub-pixel jitter, pair 1 the lens disk's first
try, pair 2 the diffuse (phi, r) of the camera ray's own hit and pair 3 that
hit's light-sampling (u1, u2).  A replaced draw does not advance the xorshift
state.  With stratified=False every operation is light_ref.trace's, bit for
bit (tests/test_stratified_host.py); in float64 it is the definition the GPU's
per-path results are compared against, in float32 the yardstick for what an
fp32 implementation may differ by (tests/test_gpu_stratified.py).
"""
import numpy as np

from light_ref import DEPTH_LIMIT, EPS, INF, RR_THRESHOLD, _basis, _dot, _mix64, _norm, sample_states

U32 = np.uint32


def brev(x):
    x = np.asarray(x, dtype=U32)
    x = ((x >> U32(1)) & U32(0x55555555)) | ((x & U32(0x55555555)) << U32(1))
    x = ((x >> U32(2)) & U32(0x33333333)) | ((x & U32(0x33333333)) << U32(2))
    x = ((x >> U32(4)) & U32(0x0F0F0F0F)) | ((x & U32(0x0F0F0F0F)) << U32(4))
    x = ((x >> U32(8)) & U32(0x00FF00FF)) | ((x & U32(0x00FF00FF)) << U32(8))
    return (x >> U32(16)) | (x << U32(16))


def lk(x, seed):
    x = np.asarray(x, dtype=U32) + np.asarray(seed, dtype=U32)
    for c in (0x6c50b47c, 0xb82f1e52, 0xc7afe638, 0x8d22f6e6):
        x = x ^ (x * U32(c))
    return x


def P(i):
    i = np.asarray(i, dtype=U32)
    for k, m in ((1, 0x55555555), (2, 0x33333333), (4, 0x0F0F0F0F), (8, 0x00FF00FF), (16, 0x0000FFFF)):
        i = i ^ ((i >> U32(k)) & U32(m))
    return i


def sobol_dim2(i):
    """The second Sobol' dimension bit by bit from its direction numbers (v = 1 << 31; v ^= v >> 1 per index bit)."""
    i = np.asarray(i, dtype=U32)
    r, v = np.zeros_like(i), U32(1 << 31)
    for b in range(32):
        r = r ^ np.where((i >> U32(b)) & U32(1), v, U32(0))
        v = v ^ (v >> U32(1))
    return r


def keys_of(W, nsub, seed, coords):
    c = np.asarray(coords).astype(np.uint64)
    ps = (c[:, 1] * np.uint64(W) + c[:, 0]) * np.uint64(nsub * nsub) + (c[:, 3] * np.uint64(nsub) + c[:, 2])
    return key_hash(seed, ps)


def key_hash(seed, pixel_sub):
    with np.errstate(over="ignore"):
        return _mix64(np.uint64(seed) ^ _mix64(np.asarray(pixel_sub, dtype=np.uint64) + np.uint64(1)))


def pairs_of_keys(key, sample):
    """[n, 4, 2] uint32: (m0, m1) of pairs 0..3 of sample `sample` under each key."""
    key = np.asarray(key, dtype=np.uint64)
    brs = brev(np.asarray(sample).astype(U32))
    out = np.zeros((len(key), 4, 2), dtype=U32)
    with np.errstate(over="ignore"):
        for j in range(4):
            h = _mix64(key ^ np.uint64(((j + 1) * 0xD1B54A32D192ED03) & (2**64 - 1)))
            sa, sb = (h >> np.uint64(32)).astype(U32), (h & np.uint64(0xFFFFFFFF)).astype(U32)
            sc = (_mix64(h) >> np.uint64(32)).astype(U32)
            i = brev(lk(brs, sa))
            out[:, j, 0] = brev(lk(i, sb)) >> U32(8)
            out[:, j, 1] = brev(lk(P(i), sc)) >> U32(8)
    return out


def pairs(W, nsub, seed, coords):
    """The four pairs of each path record {x, y, sx, sy, sample}: [n, 4, 2] uint32."""
    coords = np.asarray(coords)
    return pairs_of_keys(keys_of(W, nsub, seed, coords), coords[:, 4])


def is_02_sequence(m0, m1, max_m=8):
    """Every aligned block of 2^m consecutive points (m = 1..max_m) of the
    24-bit sequence (m0[s], m1[s]) has exactly one point in each elementary
    interval 2^-a x 2^-(m-a).  m0, m1: [..., n] with n a multiple of 2^max_m."""
    m0, m1 = np.asarray(m0, dtype=np.int64), np.asarray(m1, dtype=np.int64)
    n = m0.shape[-1]
    for m in range(1, max_m + 1):
        b0, b1 = m0.reshape(m0.shape[:-1] + (n >> m, 1 << m)), m1.reshape(m1.shape[:-1] + (n >> m, 1 << m))
        for a in range(m + 1):
            cell = ((b0 >> (24 - a)) << (m - a)) | (b1 >> (24 - (m - a)))
            if not (np.sort(cell, axis=-1) == np.arange(1 << m)).all():
                return False
    return True


def sincos_plain(a):
    """csrc/ref64.hpp's sincos_plain (the light-sampling estimator's own sin and cos, a in [0, 2 pi]) in float64
    numpy, operation for operation: (sin, cos)."""
    a = np.asarray(a, dtype=np.float64)
    k = np.floor(a * 6.36619772367581382433e-01 + 0.5)
    r = a - k * 1.57079632673412561417e+00
    w = k * 6.07710050630396597660e-11
    t = r
    r = t - w
    w = k * 2.02226624879595063154e-21 - ((t - r) - w)
    x = r - w
    y = (r - x) - w
    z = x * x
    v = z * x
    ps = 8.33333333332248946124e-03 + z * (-1.98412698298579493134e-04 + z * (2.75573137070700676789e-06 + z * (
        -2.50507602534068634195e-08 + z * 1.58969099521155010221e-10)))
    sn = x - ((z * (0.5 * y - v * ps) - y) - v * -1.66666666666666324348e-01)
    z2 = z * z
    pc = (z * (4.16666666666666019037e-02 + z * (-1.38888888888741095749e-03 + z * 2.48015872894767294178e-05))
          + (z2 * z2) * (-2.75573143513906633035e-07 + z * (2.08757232129817482790e-09
                                                            + z * -1.13596475577881948265e-11)))
    hz = 0.5 * z
    o = 1.0 - hz
    cs = o + (((1.0 - o) - hz) + (z * pc - x * y))
    quad = k.astype(np.int64) & 3
    return (np.choose(quad, [sn, cs, -sn, -cs]), np.choose(quad, [cs, -sn, -cs, sn]))


def sincos_rounded(a):
    """(sin, cos) of float64 a rounded from the long double value: the correctly rounded double but for the
    rare double rounding -- what csrc/sincos_cr.hpp computes for the plain estimator."""
    wide = np.asarray(a, dtype=np.float64).astype(np.longdouble)
    return np.sin(wide).astype(np.float64), np.cos(wide).astype(np.float64)


def trace(spheres, cam, W, H, nsub, seed, coords, lights, dtype, stratified=True, ref64_ops=False):
    """ref64_ops (float64 only): the two sampled directions in csrc/ref64.hpp's association, (u cos) sin
    instead of u (cos sin), and its sin / cos (sincos_plain with a light list, correctly rounded without) --
    the operations of PTG_FLAG_REFERENCE_F64, for comparing frames to the last bit.  Off, every operation is
    tests/light_ref.py's."""
    assert not ref64_ops or np.dtype(dtype) == np.float64
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return _trace(spheres, cam, W, H, nsub, seed, coords, lights, dtype, stratified, ref64_ops)


def _trace(spheres, cam, W, H, nsub, seed, coords, lights, dtype, stratified, ref64_ops):
    """light_ref._trace with the four pairs in place of their draws: the
    radiance (n x 3, dtype) and the segment count (n) of each path record."""
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
    q = pairs(W, nsub, seed, coords) if stratified else None

    def draw(idx):
        x = st[idx]
        x ^= x << np.uint32(13)
        x ^= x >> np.uint32(17)
        x ^= x << np.uint32(5)
        st[idx] = x
        return (x >> np.uint32(8)).astype(dtype) * T(2.0 ** -24)

    def pair_u(idx, j, k):
        return q[idx, j, k].astype(dtype) * T(2.0 ** -24)

    def direction(bu, bv, bw, ph, sn, ct):
        """bu cos(ph) sn + bv sin(ph) sn + bw ct"""
        if ref64_ops:
            sp_, cp_ = sincos_plain(ph) if L > 0 else sincos_rounded(ph)
            return (bu * cp_[:, None]) * sn[:, None] + (bv * sp_[:, None]) * sn[:, None] + bw * ct[:, None]
        return bu * (np.cos(ph) * sn)[:, None] + bv * (np.sin(ph) * sn)[:, None] + bw * ct[:, None]

    def scan(o, d):
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
        idn = np.argmin(root, axis=1)
        t = root[np.arange(len(o)), idn]
        return t, np.where(t < T(INF), idn, -1)

    camv = {k: np.asarray(cam[k][0], dtype=dtype) for k in ("position", "lower_left_corner", "cam_x_axis",
                                                           "cam_y_axis")}
    lens = T(cam["lens_radius"][0])
    everyone = np.arange(n)
    sl = T(1) / T(nsub)
    ju = pair_u(everyone, 0, 0) if stratified else draw(everyone)
    jv = pair_u(everyone, 0, 1) if stratified else draw(everyone)
    xin = coords[:, 0].astype(dtype) + coords[:, 2].astype(dtype) * sl + (T(0) + (sl - T(0)) * ju)
    yin = coords[:, 1].astype(dtype) + coords[:, 3].astype(dtype) * sl + (T(0) + (sl - T(0)) * jv)
    s, t = xin / T(W), yin / T(H)
    disk = np.zeros((n, 3), dtype=dtype)
    todo = everyone
    first_try = stratified
    while len(todo):  # camera.cpp:19-30
        px = T(-1) + T(2) * (pair_u(todo, 1, 0) if first_try else draw(todo))
        py = T(-1) + T(2) * (pair_u(todo, 1, 1) if first_try else draw(todo))
        first_try = False
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
        strat_hit = stratified and depth == 0
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
        skip = sampled[alive] & front & on_list[idh]
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
                u1 = pair_u(g, 3, 0) if strat_hit else draw(g)
                u2 = pair_u(g, 3, 1) if strat_hit else draw(g)
                lid = lights[k]
                w = C[lid] - p[di]
                d2 = _dot(w, w)
                ok = (d2 > R2[lid]) & (idh[di] != lid)
                qq = np.where(ok, R2[lid] / d2, T(0.5))
                omc = qq / (T(1) + np.sqrt(T(1) - qq))
                a = u1 * omc
                ct, sn, ph = T(1) - a, np.sqrt(a * (T(2) - a)), T(2 * np.pi) * u2
                sw = _norm(w)
                su, sv = _basis(sw)
                l = direction(su, sv, sw, ph, sn, ct)
                cs = _dot(nn[di], l)
                ok &= cs > 0
                if ok.any():
                    segs[g[ok]] += 1
                    _, winner = scan(p[di][ok], l[ok])
                    lit = winner == lid[ok]
                    gl = g[ok][lit]
                    E[gl] = E[gl] + (Tp[gl] * Le[lid[ok][lit]]) * (cs[ok][lit] * T(2) * omc[ok][lit] * T(L))[:, None]
                sampled[g] = True
            phi = T(2 * np.pi) * (pair_u(g, 2, 0) if strat_hit else draw(g))
            ra = pair_u(g, 2, 1) if strat_hit else draw(g)
            sth, cth = np.sqrt(ra), np.sqrt(T(1) - ra)
            bu, bv = _basis(nn[di])
            nd[di] = _norm(direction(bu, bv, nn[di], phi, sth, cth))
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
            free = np.nonzero(~refl)[0]
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
