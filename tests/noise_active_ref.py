"""numpy statement of ptg_noise_active_device (include/ptgpu.h "denoising
adaptive frames"): ptg_noise_device's variance and rho with each pixel's own
sample count n_p in place of samples_done.

Per pixel, from the exact sums S1, S2 (uint64 [H, W, nsub^2, 3]) and n_p, all
in double and in (sy, sx) order:
    m1 = S1 2^-32 / n_p, m2 = S2 2^-32 / n_p, v = max(0, m2 - m1 m1) / (n_p - 1)
    V_c = inv_sub2^2 sum_sub min(v, 1/4)          inv_sub2 = (float)1 / nsub^2
    rho = (float)(sqrt((V_r + V_g + V_b) / 3) / max((p_r + p_g + p_b) / 3, floor))
with p the pixel value resolved at n_p.  n_p < 2 is defined: rho = +inf and
V_c = (float)(inv_sub2^2 (nsub^2 0.25)), every sub-pixel at the clamp's bound.
"""
import numpy as np


def v_cap(nsub):
    """The variance of a pixel of which nothing is known: float32."""
    inv32 = np.float32(1.0) / np.float32(nsub * nsub)
    return np.float32((float(inv32) * float(inv32)) * (float(nsub * nsub) * 0.25))


def noise_active(S1, S2, counts, nsub, floor):
    """V [H, W, 3] float32, rho [H, W] float32."""
    counts = np.asarray(counts)
    known = counts >= 2
    n = np.where(known, counts, 2)[:, :, None, None].astype(np.float64)
    m1 = S1.astype(np.float64) * 2.0 ** -32 / n
    m2 = S2.astype(np.float64) * 2.0 ** -32 / n
    v = np.maximum(0.0, m2 - m1 * m1) / (n - 1.0)
    inv32 = np.float32(1.0) / np.float32(nsub * nsub)
    w = float(inv32) * float(inv32)
    vs = np.zeros(S1.shape[:2] + (3,))
    pix = np.zeros(S1.shape[:2] + (3,), dtype=np.float32)
    for j in range(nsub * nsub):  # (sy, sx) order
        vs = vs + np.minimum(v[:, :, j], 0.25)
        mean = np.clip(m1[:, :, j].astype(np.float32), np.float32(0), np.float32(1))
        # fmaf(mean, inv_sub2, pix): the product of two floats is exact in double
        pix = (mean.astype(np.float64) * float(inv32) + pix.astype(np.float64)).astype(np.float32)
    V = w * vs
    sigma = np.sqrt(V.sum(axis=2) / 3.0)
    mu = pix.astype(np.float64).sum(axis=2) / 3.0
    rho = (sigma / np.maximum(mu, floor)).astype(np.float32)
    V32 = np.where(known[:, :, None], V.astype(np.float32), v_cap(nsub)).astype(np.float32)
    return V32, np.where(known, rho, np.float32(np.inf)).astype(np.float32)
