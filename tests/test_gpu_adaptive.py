"""Adaptive sampling (ptg_set_active_mask_device, ptg_select_active_device,
ptg_accumulate_active_device, ptg_resolve_active_device,
ptg_read_sample_counts_device, ptg_render_adaptive) against its guarantee:

    after any sequence of adaptive passes a pixel with sample count n_p holds
    exactly samples [0, n_p) of each of its sub-pixels.

The method is tests/test_gpu_noise.py's: per-path radiance from the oracle
(pyoracle.sample_f32, Mode B: the exact mode's arithmetic), S1 / S2 / rho and
the pixel value restated in numpy -- here with a count per pixel -- plus the
dilation and the pass schedule (_simulate).  The GPU's rho is within
2^-20 rho + 2^-19 of numpy's (test_gpu_noise.py); the cases are chosen so that
no rho evaluated along a trajectory lies within 50 times that of its target
(_simulate asserts it), so every over / under decision is unambiguous and no
pixel is excluded from any comparison.  The closest approaches, measured on
the oracle: case C 1.70e-4 (81 times the tolerance of 2.1e-6 at rho = 0.2; its
last check, which changes no count), A 5.8e-4 (265 times), B 6.5e-4 (324
times), D to G 4.4e-3 or more (over 2000 times).  (The issue that introduced
these cases asks for a factor of 100 and quotes the same 1.7e-4 for case C,
which is 81 times the tolerance: the factor here is the largest round one the
stated cases admit; it guards the test's own premise, not the code.)
"""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import ptgpu  # noqa: E402
from test_gpu_noise import (EXACT, FLOOR, SEED, _cl, _noise_ref, _paths, _quant, _require_gpu,  # noqa: E402
                            _scene, _stats_of)

# scene, W, H, nsub, pass ends, target rho
CASES = {
    "A": ("box", 32, 24, 2, (4, 8, 16, 32), 0.3),
    "B": ("simple", 32, 24, 2, (4, 8, 16, 32), 0.1),
    "C": ("synthetic:300", 32, 18, 2, (2, 4, 8, 16), 0.2),  # > 64 spheres: the BVH kernel
    "D": ("box", 40, 12, 2, (2, 4, 8), 0.3),  # 2.5 pixel groups of 16
    "E": ("box", 14, 6, 3, (2, 4, 8), 0.3),  # 7 pixels x 9 sub-pixels: 63 slots
    "F": ("box", 70, 5, 1, (4, 8, 16), 0.3),  # 64 pixels per wave, a ragged row
    "G": ("simple", 1, 1, 2, (4, 8, 16), 0.1),  # a single pixel
}
CASE_DILATE = [(c, d) for c in CASES for d in (0, 1) if not (c == "G" and d == 1)]


def _E(case):
    name, W, H, nsub, ends, _ = CASES[case]
    return _paths(name, W, H, ends[-1], nsub)


@functools.lru_cache(maxsize=None)
def _prefix(case):
    """Exact prefix sums of q(c) and q(cl(c)^2) over the samples: uint64 [H, W, nsub^2, n + 1, 3], read-only."""
    c = _cl(_E(case))
    out = []
    for q in (_quant(c), _quant(c * c)):
        z = np.zeros(q.shape[:3] + (1, 3), dtype=np.uint64)
        a = np.concatenate([z, np.cumsum(q, axis=3, dtype=np.uint64)], axis=3)
        a.setflags(write=False)
        out.append(a)
    return tuple(out)


def _sums_at(case, counts):
    """S1, S2 over samples [0, counts[y, x]) of every sub-pixel: uint64 [H, W, nsub^2, 3]."""
    idx = np.asarray(counts, dtype=np.int64)[:, :, None, None, None]
    return tuple(np.take_along_axis(P, np.broadcast_to(idx, P.shape[:3] + (1, 3)), axis=3)[:, :, :, 0]
                 for P in _prefix(case))


def _rho_at(S1, S2, counts, nsub):
    """rho as ptg_noise_device defines it with each pixel's own count (n < 2: +inf): float32 [H, W]."""
    n = np.maximum(np.asarray(counts), 2)[:, :, None, None].astype(np.float64)
    rho = _noise_ref(S1, S2, n, nsub)[2]
    return np.where(np.asarray(counts) >= 2, rho, np.float32(np.inf)).astype(np.float32)


def _resolve_at(S1, counts, nsub):
    """The pixel values of resolve_kernel's arithmetic with each pixel's own count: float32 [H, W, 3]."""
    n = np.asarray(counts)[:, :, None, None].astype(np.float64)
    m1 = np.where(n > 0, S1.astype(np.float64) * 2.0 ** -32 / np.maximum(n, 1.0), 0.0)
    inv32 = np.float32(1.0) / np.float32(nsub * nsub)
    pix = np.zeros(S1.shape[:2] + (3,), dtype=np.float32)
    for j in range(nsub * nsub):  # (sy, sx) order; fmaf(mean, inv_sub2, pix): the product is exact in double
        mean = np.clip(m1[:, :, j].astype(np.float32), np.float32(0), np.float32(1))
        pix = (mean.astype(np.float64) * float(inv32) + pix.astype(np.float64)).astype(np.float32)
    return pix


def _dilate(over, d):
    """active = some pixel of the (2d+1)^2 window, clipped to the image, is over."""
    H, W = over.shape
    pad = np.zeros((H + 2 * d, W + 2 * d), dtype=bool)
    pad[d:d + H, d:d + W] = over
    out = np.zeros_like(over)
    for dy in range(2 * d + 1):
        for dx in range(2 * d + 1):
            out |= pad[dy:dy + H, dx:dx + W]
    return out


@functools.lru_cache(maxsize=None)
def _simulate(case, dilate, target=None, max_fraction=0.0):
    """ptg_render_adaptive's schedule in numpy: counts [H, W], per pass (over, active), the last rho."""
    name, W, H, nsub, ends, tgt = CASES[case]
    target = tgt if target is None else target
    counts = np.full((H, W), ends[0], dtype=np.int32)
    passes = []
    for k, e in enumerate(ends):
        S1, S2 = _sums_at(case, counts)
        rho = _rho_at(S1, S2, counts, nsub).astype(np.float64)
        fin = np.isfinite(rho)
        # the precondition: no decision within 50 times the GPU-vs-numpy tolerance of rho
        assert (np.abs(rho[fin] - target) > 50 * (2.0 ** -20 * rho[fin] + 2.0 ** -19)).all(), (case, k)
        over = rho > target
        active = _dilate(over, dilate)
        passes.append((int(over.sum()), int(active.sum())))
        if over.sum() <= max_fraction * W * H or k == len(ends) - 1:
            break
        counts = counts + np.where(active, ends[k + 1] - e, 0).astype(np.int32)
    counts.setflags(write=False)
    return counts, tuple(passes), rho.astype(np.float32)


def _params(case, flags=EXACT, **kw):
    name, W, H, nsub, ends, _ = CASES[case]
    return ptgpu.make_params(W, H, ends[-1], nsub, SEED, kw.pop("band_rows", 1), flags=flags, **kw)


def _rows(p):
    return ptgpu.shard_rows(p.height, p.band_rows, p.shard_count)


def _counts(ctx, p):
    t = torch.full((_rows(p) * p.width,), -1, dtype=torch.int32, device="cuda")
    ctx.read_sample_counts(p, t)
    torch.cuda.synchronize()
    return t.cpu().numpy().reshape(_rows(p), p.width)


def _moments(ctx, p):
    shape = (_rows(p), p.width, p.num_subpixels ** 2, 3)
    s1 = torch.full((int(np.prod(shape)),), -1, dtype=torch.int64, device="cuda")
    s2 = torch.full_like(s1, -1)
    ctx.read_moments(p, s1, s2)
    torch.cuda.synchronize()
    return s1.cpu().numpy().view(np.uint64).reshape(shape), s2.cpu().numpy().view(np.uint64).reshape(shape)


def _image(ctx, p):
    t = torch.full((_rows(p) * p.width * 3,), -7.0, dtype=torch.float32, device="cuda")
    ctx.resolve_active(t, p)
    torch.cuda.synchronize()
    return t.cpu().numpy().reshape(_rows(p), p.width, 3)


def _select(ctx, p, rel, dilate, floor=FLOOR):
    rho = torch.full((_rows(p) * p.width,), -7.0, dtype=torch.float32, device="cuda")
    stats = torch.zeros(6, dtype=torch.int64, device="cuda")
    ctx.select_active(p, rel, floor, dilate, rho, stats)
    torch.cuda.synchronize()
    return rho.cpu().numpy().reshape(_rows(p), p.width), stats.cpu().numpy().view(np.uint64)


def _run(ctx, p, ends, target, dilate, exact_units=True):
    """The driver's schedule through the device entry points (max_fraction 0); the per-pass stats."""
    ctx.reset_accumulation(p)
    ctx.set_active_mask(p)
    units, done, stats = 0, 0, []
    for k, e in enumerate(ends):
        ctx.accumulate_active(p, e - done, units if exact_units else 0)
        done = e
        rho, st = _select(ctx, p, target, dilate)
        stats.append(st)
        if st[0] == 0:
            break
        units = int(st[5])
    return stats, rho


@functools.lru_cache(maxsize=None)
def _device_frame(case, dilate, flags=EXACT, chunk=0, exact_units=True):
    """counts, S1, S2, image of the schedule run through the device entry points (read-only)."""
    name, W, H, nsub, ends, target = CASES[case]
    p = _params(case, flags=flags, chunk_samples=chunk)
    with ptgpu.Context(*_scene(name, W, H)) as ctx:
        _run(ctx, p, ends, target, dilate, exact_units)
        out = (_counts(ctx, p),) + _moments(ctx, p) + (_image(ctx, p),)
    for a in out:
        a.setflags(write=False)
    return out


# ---- 1. the driver against the numpy simulation ------------------------------
@pytest.mark.parametrize("case,dilate", CASE_DILATE)
def test_driver_matches_the_simulation(case, dilate):
    _require_gpu()
    name, W, H, nsub, ends, target = CASES[case]
    counts, passes, _ = _simulate(case, dilate)
    if case != "G":
        assert len(np.unique(counts)) > 1  # a mix of counts
    if dilate == 1 and case != "G":
        assert set(np.unique(counts).tolist()) - set(ends)  # ... and not only schedule ends: unequal n_p inside a unit
    img = np.zeros((H * W, 3))
    rep, got = ptgpu.render_adaptive(*_scene(name, W, H), img, W, H, ends[-1], rel_error=target, floor=FLOOR,
                                     max_fraction=0.0, min_samples=ends[0], dilate=dilate, num_subpixels=nsub,
                                     seed=SEED, flags=EXACT, sample_counts=True)
    print(f"{case} dilate {dilate}: counts {sorted(set(counts.reshape(-1).tolist()))}, passes {passes}, report {rep}")
    assert np.array_equal(got, counts)
    assert rep["passes"] == len(passes) and rep["pixels"] == W * H
    assert list(zip(rep["pass_over"], rep["pass_active"])) == list(passes)
    assert rep["pass_added"] == [ends[0]] + [ends[k] - ends[k - 1] for k in range(1, len(passes))]
    assert rep["total_samples"] == int(counts.sum(dtype=np.int64))
    assert rep["pixels_over"] == passes[-1][0] and rep["converged"] == int(passes[-1][0] == 0)
    assert rep["max_samples"] == int(counts.max())
    S1, _ = _sums_at(case, counts)
    assert np.array_equal(img.reshape(H, W, 3), _resolve_at(S1, counts, nsub).astype(np.float64))


# ---- 2. the sums, whatever the decisions ------------------------------------------
@pytest.mark.parametrize("case,dilate", CASE_DILATE)
def test_sums_are_the_first_n_p_samples(case, dilate):
    _require_gpu()
    counts, g1, g2, _ = _device_frame(case, dilate)
    assert counts.min() >= CASES[case][4][0] and counts.max() <= CASES[case][4][-1]
    S1, S2 = _sums_at(case, counts)
    assert np.array_equal(g1, S1)
    assert np.array_equal(g2, S2)
    assert np.array_equal(counts, _simulate(case, dilate)[0])


# ---- 3. the image against the plain kernel ----------------------------------------
@pytest.mark.parametrize("mode", [EXACT, 0], ids=["exact", "fast"])
@pytest.mark.parametrize("case", ["A", "C", "E", "F"])
def test_pixels_equal_the_plain_render_at_their_count(case, mode):
    _require_gpu()
    name, W, H, nsub, ends, target = CASES[case]
    counts, _, _, img = _device_frame(case, 1, flags=mode)
    assert len(np.unique(counts)) > 1
    with ptgpu.Context(*_scene(name, W, H)) as ctx:
        for n in np.unique(counts).tolist():
            out = torch.full((H * W * 3,), -7.0, dtype=torch.float32, device="cuda")
            ctx.render_device(out, ptgpu.make_params(W, H, n, nsub, SEED, flags=mode))
            torch.cuda.synchronize()
            plain = out.cpu().numpy().reshape(H, W, 3)
            assert np.array_equal(img[counts == n], plain[counts == n]), n


# ---- 4. list shapes through the mask entry point ------------------------------------
def _masks(W, H, ppw):
    m = {"empty": np.zeros((H, W), np.uint8)}
    m["corners"] = m["empty"].copy()
    m["corners"][0, 0] = m["corners"][H - 1, W - 1] = 1
    m["one_unit"] = m["empty"].copy()
    m["one_unit"][1, 1:1 + min(ppw, W - 1)] = 7  # exactly pixels_per_wave in a row (any non-zero byte)
    m["unit_plus_one"] = m["empty"].copy()
    m["unit_plus_one"][2, 0:min(ppw + 1, W)] = 1
    m["full_row"] = m["empty"].copy()
    m["full_row"][H - 2] = 1
    m["every_second"] = ((np.arange(W)[None, :] + np.arange(H)[:, None]) % 2).astype(np.uint8)
    m["alternate_rows"] = np.repeat((np.arange(H) % 2).astype(np.uint8)[:, None], W, axis=1)
    m["all"] = np.ones((H, W), np.uint8)
    return m


@pytest.mark.parametrize("case", ["D", "E", "C"])
def test_mask_list_shapes(case):
    """accumulate_active(3) under one mask, accumulate_active(2) under another:
    counts 3 m1 + 2 m2, the sums those of the first n_p samples, everything
    outside the masks untouched; d_info = pixels, sum over rows of ceil(row / pixels_per_wave)."""
    _require_gpu()
    name, W, H, nsub, ends, _ = CASES[case]
    ppw = 64 // (nsub * nsub)
    masks = _masks(W, H, ppw)
    names = list(masks)
    p = _params(case)
    with ptgpu.Context(*_scene(name, W, H)) as ctx:
        for i, first in enumerate(names):
            second = names[(i + 3) % len(names)]
            ctx.reset_accumulation(p)
            infos = []
            for key, add in ((first, 3), (second, 2)):
                m = masks[key]
                info = torch.full((2,), -1, dtype=torch.int64, device="cuda")
                ctx.set_active_mask(p, torch.from_numpy(m.reshape(-1).copy()).cuda(), info)
                ctx.accumulate_active(p, add)
                infos.append((info, m))
            counts, (g1, g2) = _counts(ctx, p), _moments(ctx, p)
            for info, m in infos:
                on = m != 0
                assert info.cpu().tolist() == [int(on.sum()), int(sum(-(-int(r.sum()) // ppw) for r in on))], first
            want = 3 * (masks[first] != 0).astype(np.int32) + 2 * (masks[second] != 0).astype(np.int32)
            assert np.array_equal(counts, want), (first, second)
            S1, S2 = _sums_at(case, want)
            assert np.array_equal(g1, S1) and np.array_equal(g2, S2), (first, second)
            assert not g1[want == 0].any() and not g2[want == 0].any()
        ctx.reset_accumulation(p)  # mask None: every pixel
        info = torch.zeros(2, dtype=torch.int64, device="cuda")
        ctx.set_active_mask(p, None, info)
        ctx.accumulate_active(p, 2)
        assert (_counts(ctx, p) == 2).all() and info.cpu().tolist() == [W * H, H * -(-W // ppw)]


# ---- 5. invariance --------------------------------------------------------------------
@pytest.mark.parametrize("chunk,exact_units", [(1, True), (3, True), (0, False)])
def test_frame_does_not_depend_on_chunking_or_the_unit_bound(chunk, exact_units):
    _require_gpu()
    ref = _device_frame("A", 1)
    got = _device_frame("A", 1, chunk=chunk, exact_units=exact_units)
    for a, b in zip(ref, got):
        assert np.array_equal(a, b)


def test_three_shards_with_dilate_0():
    """3 shards of 2-row bands, one context each: counts and sums are the frame's
    rows, the stats add over the shards (max for [2])."""
    _require_gpu()
    name, W, H, nsub, ends, target = CASES["A"]
    counts, S1, S2, _ = _device_frame("A", 0)
    with ptgpu.Context(*_scene(name, W, H)) as ctx:
        whole, _ = _run(ctx, _params("A"), ends, target, 0)
    total = [np.zeros(6, dtype=np.uint64) for _ in whole]
    for rank in range(3):
        ps = _params("A", band_rows=2, shard_rank=rank, shard_count=3)
        with ptgpu.Context(*_scene(name, W, H)) as ctx:
            stats, _ = _run(ctx, ps, ends, target, 0)
            c, (g1, g2) = _counts(ctx, ps), _moments(ctx, ps)
        m = ptgpu.slab_to_image_rows(H, 2, rank, 3)
        ok, rows = m >= 0, m[m >= 0]
        assert np.array_equal(c[ok], counts[rows]) and not c[~ok].any()
        assert np.array_equal(g1[ok], S1[rows]) and np.array_equal(g2[ok], S2[rows])
        assert not g1[~ok].any() and not g2[~ok].any()
        assert len(stats) == len(whole)  # (no shard converges before the frame does here)
        for t, st in zip(total, stats):
            t[[0, 1, 3, 4]] += st[[0, 1, 3, 4]]
            t[2] = max(t[2], st[2])
    for t, w in zip(total, whole):
        assert np.array_equal(t[:5], w[:5])


@pytest.mark.parametrize("case", ["D", "C"])
def test_segment_counters_of_an_adaptive_pass(case):
    """d_segments: the paths of an all-active pass are the plain pass's paths, so the scene scans
    counted are equal and no path's radiance is clipped; the driver's report carries the counters."""
    _require_gpu()
    name, W, H, nsub, ends, target = CASES[case]
    flags = EXACT | ptgpu.FLAG_COUNT_TESTS | ptgpu.FLAG_COUNT_NONFINITE
    p = _params(case, flags=flags)
    a, b = (torch.zeros(4, dtype=torch.int64, device="cuda") for _ in range(2))
    with ptgpu.Context(*_scene(name, W, H)) as ctx:
        ctx.reset_accumulation(p)
        ctx.set_active_mask(p)
        ctx.accumulate_active(p, 3, segments=a)
        ctx.accumulate_active(p, 1, segments=a)
        ctx.reset_accumulation(p)
        ctx.accumulate(p, 0, 4, segments=b)
        torch.cuda.synchronize()
    a, b = a.cpu().tolist(), b.cpu().tolist()
    assert a[0] == b[0] > W * H * nsub * nsub * 4 and a[1] > 0 and a[3] == b[3] == 0
    img = np.zeros((H * W, 3))
    rep = ptgpu.render_adaptive(*_scene(name, W, H), img, W, H, ends[-1], rel_error=1e9, floor=FLOOR,
                                max_fraction=0.0, min_samples=4, num_subpixels=nsub, seed=SEED, flags=flags)
    assert rep["counters"][0] == a[0] and rep["counters"][3] == 0


# ---- 6. limits ---------------------------------------------------------------------------
def _plain(name, W, H, samples, nsub, flags=EXACT):
    img = np.zeros((H * W, 3))
    ptgpu.render(*_scene(name, W, H), img, W, H, samples, nsub, SEED, flags=flags)
    return img


def test_huge_target_stops_after_the_first_pass():
    _require_gpu()
    name, W, H, nsub, ends, _ = CASES["E"]
    img = np.zeros((H * W, 3))
    rep, counts = ptgpu.render_adaptive(*_scene(name, W, H), img, W, H, ends[-1], rel_error=1e9, floor=FLOOR,
                                        max_fraction=0.0, min_samples=ends[0], dilate=1, num_subpixels=nsub,
                                        seed=SEED, flags=EXACT, sample_counts=True)
    assert (counts == ends[0]).all() and (rep["passes"], rep["converged"], rep["pass_over"]) == (1, 1, [0])
    assert rep["total_samples"] == ends[0] * W * H and rep["mean_samples"] == ends[0]
    assert np.array_equal(img, _plain(name, W, H, ends[0], nsub))


def test_zero_target_with_the_widest_window_runs_every_pixel_to_the_cap():
    _require_gpu()
    name, W, H, nsub, ends, _ = CASES["E"]
    img = np.zeros((H * W, 3))
    rep, counts = ptgpu.render_adaptive(*_scene(name, W, H), img, W, H, ends[-1], rel_error=0.0, floor=FLOOR,
                                        max_fraction=0.0, min_samples=ends[0], dilate=8, num_subpixels=nsub,
                                        seed=SEED, flags=EXACT, sample_counts=True)
    assert (counts == ends[-1]).all() and (rep["passes"], rep["converged"]) == (len(ends), 0)
    assert rep["pass_active"] == [W * H] * len(ends) and all(0 < o <= W * H for o in rep["pass_over"])
    assert np.array_equal(img, _plain(name, W, H, ends[-1], nsub))


def test_fewer_than_two_samples_is_infinitely_noisy_and_stats_match_the_rho_slab():
    _require_gpu()
    name, W, H, nsub, ends, target = CASES["D"]
    p = _params("D")
    mask = np.zeros((H, W), np.uint8)
    mask[:, ::3] = 1
    with ptgpu.Context(*_scene(name, W, H)) as ctx:
        ctx.reset_accumulation(p)
        rho, st = _select(ctx, p, target, 0)  # no sample anywhere
        assert np.isinf(rho).all() and st.tolist()[:1] + st.tolist()[3:5] == [W * H] * 3
        ctx.set_active_mask(p, torch.from_numpy(mask.reshape(-1).copy()).cuda())
        ctx.accumulate_active(p, 1)  # one sample: still no variance
        ctx.set_active_mask(p, torch.from_numpy((1 - mask).reshape(-1).copy()).cuda())
        ctx.accumulate_active(p, 4)
        rho, st = _select(ctx, p, target, 0)
        counts = _counts(ctx, p)
    assert np.array_equal(counts, np.where(mask != 0, 1, 4))
    assert np.isinf(rho[mask != 0]).all() and np.isfinite(rho[mask == 0]).all()
    assert np.array_equal(st[:4], _stats_of(rho, target))
    over = rho.astype(np.float64) > target
    assert over[mask != 0].all() and st[4] == over.sum()
    S1, S2 = _sums_at("D", counts)
    ref = _rho_at(S1, S2, counts, nsub).astype(np.float64)
    fin = np.isfinite(ref)
    assert (np.abs(rho[fin].astype(np.float64) - ref[fin]) <= 2.0 ** -20 * ref[fin] + 2.0 ** -19).all()


# ---- 7. errors -----------------------------------------------------------------------------
def test_adaptive_errors():
    _require_gpu()
    name, W, H, nsub, ends, target = CASES["D"]
    p = _params("D")
    n = H * W
    slab = torch.zeros(n * 3, dtype=torch.float32, device="cuda")
    cnt = torch.zeros(n, dtype=torch.int32, device="cuda")
    with ptgpu.Context(*_scene(name, W, H)) as ctx, ptgpu.Context(*_scene(name, W, H)) as fresh:
        ctx.reset_accumulation(p)
        with pytest.raises(ptgpu.PtgError, match=r"\(-1\).*no active list"):
            ctx.accumulate_active(p, 2)
        ctx.set_active_mask(p)
        with pytest.raises(ptgpu.PtgError, match=r"\(-1\).*add_samples"):
            ctx.accumulate_active(p, -1)
        with pytest.raises(ptgpu.PtgError, match=r"\(-1\).*another frame"):
            ctx.accumulate_active(ptgpu.make_params(W, H - 1, 8, nsub, SEED, flags=EXACT), 2)
        for d in (-1, 9):
            with pytest.raises(ptgpu.PtgError, match=r"\(-1\).*dilate"):
                ctx.select_active(p, target, FLOOR, d)
        with pytest.raises(ptgpu.PtgError, match=r"\(-4\).*dilate"):
            ctx.select_active(_params("D", band_rows=2, shard_rank=0, shard_count=2), target, FLOOR, 1)
        with pytest.raises(ptgpu.PtgError, match=r"\(-1\).*floor"):
            ctx.select_active(p, target, 0.0, 0)
        with pytest.raises(ptgpu.PtgError, match=r"\(-1\).*floor"):
            ctx.select_active(p, -0.1, FLOOR, 0)
        with pytest.raises(ptgpu.PtgError, match=r"\(-4\)"):
            ctx.set_active_mask(_params("D", flags=ptgpu.FLAG_REFERENCE_F64))
        L, P = ptgpu.lib(), __import__("ctypes").byref(p)
        assert L.ptg_resolve_active_device(ctx._h, P, None, None) == -1 and b"NULL" in L.ptg_last_error()
        assert L.ptg_read_sample_counts_device(ctx._h, P, None, None) == -1 and b"NULL" in L.ptg_last_error()
        assert L.ptg_set_active_mask_device(None, P, None, None, None) == -1 and b"NULL" in L.ptg_last_error()
        assert L.ptg_select_active_device(None, P, 0.1, 0.01, 0, None, None, None) == -1
        assert L.ptg_accumulate_active_device(None, P, 1, 0, None, None) == -1
        # the count bound: the host tracks the sum of the adds since the reset (an empty list: nothing runs)
        ctx.set_active_mask(p, torch.zeros(n, dtype=torch.uint8, device="cuda"))
        ctx.accumulate_active(p, 2 ** 30 - 1)
        ctx.accumulate_active(p, 1)
        with pytest.raises(ptgpu.PtgError, match=r"\(-1\).*2\^30"):
            ctx.accumulate_active(p, 1)
        # after adaptive passes the entry points that take one n refuse ...
        ctx.reset_accumulation(p)
        ctx.set_active_mask(p)
        ctx.accumulate_active(p, 2)
        for call in (lambda: ctx.accumulate(p, 2, 4), lambda: ctx.resolve(slab, p, 2),
                     lambda: ctx.noise(p, 2, 0.1, FLOOR)):
            with pytest.raises(ptgpu.PtgError, match=r"\(-1\).*adaptive passes since the last reset"):
                call()
        ctx.read_moments(p, torch.zeros(n * nsub * nsub * 3, dtype=torch.int64, device="cuda"),
                         torch.zeros(n * nsub * nsub * 3, dtype=torch.int64, device="cuda"))  # keeps working
        # ... and the adaptive ones after a uniform pass
        ctx.reset_accumulation(p)
        ctx.accumulate(p, 0, 2)
        for call in (lambda: ctx.set_active_mask(p), lambda: ctx.select_active(p, target, FLOOR),
                     lambda: ctx.accumulate_active(p, 2), lambda: ctx.resolve_active(slab, p),
                     lambda: ctx.read_sample_counts(p, cnt)):
            with pytest.raises(ptgpu.PtgError, match=r"\(-1\).*ptg_accumulate_device pass since the last reset"):
                call()
        # a reset clears both records: the plain entry points give a fresh context's output
        ctx.reset_accumulation(p)
        ctx.set_active_mask(p)
        ctx.accumulate_active(p, 3)
        ctx.reset_accumulation(p)
        a, b = torch.zeros_like(slab), torch.zeros_like(slab)
        for c, out in ((ctx, a), (fresh, b)):
            c.reset_accumulation(p)
            c.accumulate(p, 0, 4)
            c.resolve(out, p, 4)
        ctx.reset_accumulation(p)
        ctx.read_sample_counts(p, cnt)
        torch.cuda.synchronize()
        assert a.cpu().numpy().max() > 0 and torch.equal(a, b) and not cnt.any()


# ---- 8. the CLI -------------------------------------------------------------------------------
def test_cli_adaptive_writes_the_drivers_image_and_count_map(tmp_path):
    _require_gpu()
    cli = os.path.join(os.path.dirname(ptgpu.LIB_PATH), "pt_render_gpu")
    W, H, spp, target = 32, 24, 128, 0.3
    out, spm = tmp_path / "o.ppm", tmp_path / "spp.pgm"
    r = subprocess.run([cli, "--scene", "box", "--width", str(W), "--height", str(H), "--format", "p6", "--out",
                        str(out), "--spp", str(spp), "--noise-target", str(target), "--noise-fraction", "0",
                        "--min-spp", "16", "--exact-math", "--adaptive", "--dilate", "1", "--spp-map", str(spm)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    img = np.zeros((H * W, 3))
    rep, counts = ptgpu.render_adaptive(*_scene("box", W, H), img, W, H, spp // 4, rel_error=target, floor=0.01,
                                        max_fraction=0.0, min_samples=4, dilate=1, flags=EXACT, sample_counts=True)
    assert np.array_equal(counts, _simulate("A", 1)[0])  # (case A's frame)
    head = f"P5\n{W} {H}\n255\n".encode()
    assert spm.read_bytes() == head + counts.astype(np.uint8).tobytes()
    m = re.search(r"^noise: adaptive, at most (\d+) spp after (\d+) passes, (\d+)/(\d+) pixels above (\S+), max (\S+), "
                  r"mean (\S+), converged ([01]), mean samples per sub-pixel (\S+)$", r.stderr, re.M)
    assert m, r.stderr
    assert (int(m.group(1)), int(m.group(2)), int(m.group(3)), int(m.group(4)), int(m.group(8))) == \
        (4 * rep["max_samples"], rep["passes"], rep["pixels_over"], W * H, rep["converged"])
    assert float(m.group(9)) == pytest.approx(rep["mean_samples"], rel=1e-5)
    import pyoracle as po
    want = po.tonemap(img).astype(np.uint8).tobytes()
    assert out.read_bytes() == f"P6\n{W} {H}\n255\n".encode() + want
    r = subprocess.run([cli, "--adaptive", "--width", "8", "--height", "8"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--noise-target" in r.stderr
