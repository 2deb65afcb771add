"""Filtered adaptive frames and filtered frames on several GPUs
(include/ptgpu.h "denoising adaptive frames and frames on several GPUs"):

1. ptg_noise_active_device at uniform counts against ptg_noise_device,
2. at mixed counts against ptg_noise_device selected per pixel, the numpy
   statement, the n_p < 2 rule and the rows of a sharded slab,
3. ptg_render_adaptive_denoised against its pieces and the host filter,
4. the three multi-device drivers against the three one-device drivers,
5. a failing gather, 6. the state the pieces keep, 7. acceptance, 8. the tool.

Every comparison called "equal" is for bit equality.  Shapes: the adaptive
suite's cases A (box 32x24), C (synthetic:300, the BVH kernel) and F (70x5,
nsub 1), and the denoise suite's 70x37 and 33x21 (70 columns cross a 64-column
tile of the filter, 5 iterations reach step 16).
"""
import functools
import os
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import noise_active_ref  # noqa: E402
import ptgpu  # noqa: E402
from test_gpu_adaptive import CASES, _counts, _image, _moments, _rows, _run  # noqa: E402
from test_gpu_noise import EXACT, FLOOR, SEED, _noise_ref, _require_gpu, _scene  # noqa: E402

MOM = ptgpu.FLAG_MOMENTS
LS = ptgpu.FLAG_LIGHT_SAMPLING
DEV = "cuda:0"

# scene, W, H, nsub, pass ends, target rho: the adaptive suite's, and the denoise suite's two sizes
FRAMES = {c: CASES[c] for c in "ACF"}
FRAMES["70x37"] = ("simple", 70, 37, 2, (2, 4, 8), 0.1)
FRAMES["33x21"] = ("simple", 33, 21, 2, (2, 4, 8), 0.1)


def _p(case, flags=EXACT, samples=None, **kw):
    name, W, H, nsub, ends, _ = FRAMES[case]
    return ptgpu.make_params(W, H, samples or ends[-1], nsub, SEED, kw.pop("band_rows", 1), flags=flags, **kw)


def _noise_active(ctx, p, floor=FLOOR, fill=-7.0):
    """var [rows, W, 3], rho [rows, W] of ptg_noise_active_device over buffers pre-filled with `fill`."""
    var = torch.full((_rows(p) * p.width * 3,), fill, dtype=torch.float32, device=DEV)
    rho = torch.full((_rows(p) * p.width,), fill, dtype=torch.float32, device=DEV)
    ctx.noise_active(p, floor, var, rho)
    torch.cuda.synchronize()
    return var.cpu().numpy().reshape(_rows(p), p.width, 3), rho.cpu().numpy().reshape(_rows(p), p.width)


def _noise_uniform(ctx, p, n, floor=FLOOR):
    """var, rho of ptg_noise_device for the uniform PTG_FLAG_MOMENTS frame of n samples."""
    var = torch.full((_rows(p) * p.width * 3,), -7.0, dtype=torch.float32, device=DEV)
    rho = torch.full((_rows(p) * p.width,), -7.0, dtype=torch.float32, device=DEV)
    ctx.reset_accumulation(p)
    ctx.accumulate(p, 0, n)
    ctx.noise(p, n, 0.0, floor, var, rho)
    torch.cuda.synchronize()
    return var.cpu().numpy().reshape(_rows(p), p.width, 3), rho.cpu().numpy().reshape(_rows(p), p.width)


# ---- 1. uniform counts ------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [EXACT, 0], ids=["exact", "fast"])
@pytest.mark.parametrize("n", [2, 16])
@pytest.mark.parametrize("case", ["A", "C"])
def test_uniform_counts_equal_noise_device(case, n, flags):
    _require_gpu()
    name, W, H, nsub, _, _ = FRAMES[case]
    pa, pm = _p(case, flags, n), _p(case, flags | MOM, n)
    with ptgpu.Context(*_scene(name, W, H)) as ctx:
        ctx.reset_accumulation(pa)
        ctx.set_active_mask(pa)
        ctx.accumulate_active(pa, n)
        var, rho = _noise_active(ctx, pa)
        want_var, want_rho = _noise_uniform(ctx, pm, n)
    assert np.array_equal(var, want_var) and np.array_equal(rho, want_rho)
    assert (var > 0).any() and np.isfinite(rho).all()


# ---- 2. mixed counts ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mixed_frame():
    """Case A's adaptive passes on a context: counts, S1, S2, var, rho (read-only), and per distinct count
    the uniform frame's var and rho from ptg_noise_device."""
    name, W, H, nsub, ends, target = FRAMES["A"]
    p, pm = _p("A"), _p("A", EXACT | MOM)
    with ptgpu.Context(*_scene(name, W, H)) as ctx:
        _run(ctx, p, ends, target, 1)
        counts = _counts(ctx, p)
        S1, S2 = _moments(ctx, p)
        var, rho = _noise_active(ctx, p)
        uniform = {int(c): _noise_uniform(ctx, pm, int(c)) for c in np.unique(counts)}
    for a in (counts, S1, S2, var, rho):
        a.setflags(write=False)
    return counts, S1, S2, var, rho, uniform


def test_mixed_counts_equal_noise_device_per_pixel():
    _require_gpu()
    counts, _, _, var, rho, uniform = _mixed_frame()
    assert len(uniform) >= 2 and min(uniform) >= 2  # at least two distinct counts occur
    want_var, want_rho = np.zeros_like(var), np.zeros_like(rho)
    for c, (v, r) in uniform.items():
        want_var[counts == c] = v[counts == c]
        want_rho[counts == c] = r[counts == c]
    assert np.array_equal(var, want_var) and np.array_equal(rho, want_rho)


def test_mixed_counts_against_the_numpy_statement():
    """The tolerances of tests/test_gpu_noise.py's variance and rho slabs (that suite has no equality for
    rho against numpy: the square root is the GPU's)."""
    _require_gpu()
    nsub = FRAMES["A"][3]
    counts, S1, S2, var, rho, _ = _mixed_frame()
    V, want_rho = noise_active_ref.noise_active(S1, S2, counts, nsub, FLOOR)
    V64, tol, _ = _noise_ref(S1, S2, counts[:, :, None, None].astype(np.float64), nsub)
    assert np.array_equal(V, V64.astype(np.float32))  # (the two numpy statements agree here too)
    dv, dr = np.abs(var.astype(np.float64) - V64), np.abs(rho.astype(np.float64) - want_rho.astype(np.float64))
    print("var: max |d| / tol", float((dv / np.maximum(tol, 1e-300)).max()), "rho: max |d|", float(dr.max()))
    assert (dv <= tol).all()
    assert (dr <= 2.0 ** -20 * want_rho + 2.0 ** -19).all()


def test_pixels_below_two_samples_carry_the_cap():
    _require_gpu()
    name, W, H, nsub, _, _ = FRAMES["A"]
    p = _p("A")
    one = np.zeros((H, W), np.uint8)
    one[2:9, 3:20] = 1
    more = np.zeros((H, W), np.uint8)
    more[5:9, 10:30] = 1  # overlaps `one`: 0, 1, 3 and 4 samples occur
    want = one.astype(np.int32) + 3 * more.astype(np.int32)
    with ptgpu.Context(*_scene(name, W, H)) as ctx:
        ctx.reset_accumulation(p)
        for mask, add in ((one, 1), (more, 3)):
            ctx.set_active_mask(p, torch.from_numpy(mask).to(DEV))
            ctx.accumulate_active(p, add)
        counts = _counts(ctx, p)
        S1, S2 = _moments(ctx, p)
        var, rho = _noise_active(ctx, p)
    assert np.array_equal(counts, want) and sorted(np.unique(counts)) == [0, 1, 3, 4]
    unknown = counts < 2
    assert (var[unknown] == noise_active_ref.v_cap(nsub)).all() and np.isposinf(rho[unknown]).all()
    _, want_rho = noise_active_ref.noise_active(S1, S2, counts, nsub, FLOOR)
    V64, tol, _ = _noise_ref(S1, S2, np.maximum(counts, 2)[:, :, None, None].astype(np.float64), nsub)
    assert np.isfinite(rho[~unknown]).all()
    assert (np.abs(var - V64) <= tol)[~unknown].all()
    assert (np.abs(rho[~unknown] - want_rho[~unknown]) <= 2.0 ** -20 * want_rho[~unknown] + 2.0 ** -19).all()


def test_sharded_slab_rows_past_the_image_stay_untouched():
    """9 rows in bands of 2 on 3 shards: slabs of 4 rows, shard 1's last and shard 2's last two lie past
    the image.  Every shard's rows equal the one-device frame's."""
    _require_gpu()
    W, H, nsub, n = 20, 9, 2, 4
    scn, cam = _scene("box", W, H)
    whole = ptgpu.make_params(W, H, n, nsub, SEED, flags=EXACT)
    past = 0
    with ptgpu.Context(scn, cam) as ctx:
        ctx.reset_accumulation(whole)
        ctx.set_active_mask(whole)
        ctx.accumulate_active(whole, n)
        full_var, full_rho = _noise_active(ctx, whole)
        for rank in range(3):
            q = ptgpu.make_params(W, H, n, nsub, SEED, 2, rank, 3, flags=EXACT)
            ctx.reset_accumulation(q)
            ctx.set_active_mask(q)
            ctx.accumulate_active(q, n)
            var, rho = _noise_active(ctx, q, fill=-7.0)
            rows = ptgpu.slab_to_image_rows(H, 2, rank, 3)
            assert len(rows) == 4
            ok = rows >= 0
            assert np.array_equal(var[ok], full_var[rows[ok]]) and np.array_equal(rho[ok], full_rho[rows[ok]])
            assert (var[~ok] == -7.0).all() and (rho[~ok] == -7.0).all()
            past += int((~ok).sum())
    assert past == 3


# ---- 3. the one-device driver = its pieces = the host filter ------------------------------------
def _filter_params(cam, W, H, iterations):
    k = ptgpu.denoise_defaults()
    k.iterations = iterations
    k.pixel_spread = ptgpu.pixel_spread(cam, W, H)
    return k


def _driver(case, flags, k=None, dilate=1, counts=True):
    name, W, H, nsub, ends, target = FRAMES[case]
    img = np.zeros((H, W, 3))
    out = ptgpu.render_adaptive_denoised(*_scene(name, W, H), img, W, H, ends[-1], target, FLOOR, 0.0, ends[0], dilate,
                                         nsub, SEED, 0, flags, sample_counts=counts, params=k)
    return (img,) + (out if counts else (out,))


@pytest.mark.parametrize("case,flags", [(c, f) for c in ("A", "C", "F", "70x37") for f in (0, EXACT)] + [("A", LS)],
                         ids=lambda v: v if isinstance(v, str) else {0: "fast", EXACT: "exact", LS: "ls"}[v])
def test_adaptive_driver_equals_its_pieces_and_the_host_filter(case, flags):
    _require_gpu()
    name, W, H, nsub, ends, target = FRAMES[case]
    scn, cam = _scene(name, W, H)
    p = _p(case, flags)
    with ptgpu.Context(scn, cam, device=0) as ctx:
        _run(ctx, p, ends, target, 1)
        counts = _counts(ctx, p)[:H]
        color = torch.zeros((_rows(p), W, 3), dtype=torch.float32, device=DEV)
        var = torch.zeros_like(color)
        ctx.resolve_active(color, p)
        ctx.noise_active(p, 1.0, var)
        feat = ctx.features(p)
        by_hand = {it: ptgpu.denoise(color[:H], var[:H], feat[:H], _filter_params(cam, W, H, it)) for it in (1, 3, 5)}
        torch.cuda.synchronize()
        by_hand = {it: t.cpu().numpy() for it, t in by_hand.items()}
        color, var, feat = color[:H].cpu().numpy(), var[:H].cpu().numpy(), feat[:H].cpu().numpy()
    assert len(np.unique(counts)) >= 2  # the frame is an adaptive one
    for it in (1, 3, 5):
        k = _filter_params(cam, W, H, it)
        img, rep, got_counts = _driver(case, flags, None if it == 5 else k)  # 5: the defaults, params NULL
        assert np.array_equal(got_counts, counts)
        assert np.array_equal(img, by_hand[it].astype(np.float64)), it
        assert np.array_equal(by_hand[it], ptgpu.denoise_host(color, var, feat, k)), it
    assert not np.array_equal(by_hand[1], color)


@pytest.mark.parametrize("case,flags", [("A", 0), ("C", EXACT)])
def test_adaptive_driver_iterations_0_is_render_adaptive(case, flags):
    _require_gpu()
    name, W, H, nsub, ends, target = FRAMES[case]
    scn, cam = _scene(name, W, H)
    want = np.zeros((H, W, 3))
    want_rep, want_counts = ptgpu.render_adaptive(scn, cam, want, W, H, ends[-1], target, FLOOR, 0.0, ends[0], 1, nsub,
                                                  SEED, 0, flags | ptgpu.FLAG_COUNT_TESTS, sample_counts=True)
    img, rep, counts = _driver(case, flags | ptgpu.FLAG_COUNT_TESTS, _filter_params(cam, W, H, 0))
    assert np.array_equal(img, want) and np.array_equal(counts, want_counts) and rep == want_rep
    assert rep["counters"][0] > 0 and rep["passes"] >= 2
    img2 = np.ones((H, W, 3))
    ptgpu.render_adaptive_denoised(scn, cam, img2, W, H, ends[-1], target, FLOOR, 0.0, ends[0], 1, nsub, SEED, 0,
                                   flags, params=_filter_params(cam, W, H, 0))
    assert np.array_equal(img2, 1.0 + want)  # it adds


# ---- 4. several devices = one device ----------------------------------------------------------------
FRAC = {"A": 0.3, "C": 0.05, "33x21": 0.3}  # the noise-target driver's stop fraction (several passes run)


@functools.lru_cache(maxsize=None)
def _one_device(case, kind, dilate=0, flags=EXACT):
    """The one-device drivers' results (read-only): image [H*W, 3], then the report (and counts)."""
    name, W, H, nsub, ends, target = FRAMES[case]
    scn, cam = _scene(name, W, H)
    img = np.zeros((H * W, 3))
    if kind == "plain":
        ptgpu.render_denoised(scn, cam, img, W, H, ends[-1], nsub, SEED, 0, flags)
        rest = ()
    elif kind == "to_noise":
        rest = (ptgpu.render_to_noise_denoised(scn, cam, img, W, H, ends[-1], target, FLOOR, FRAC[case], ends[0], nsub,
                                               SEED, 0, flags),)
    else:
        rest = ptgpu.render_adaptive_denoised(scn, cam, img, W, H, ends[-1], target, FLOOR, 0.0, ends[0], dilate, nsub,
                                              SEED, 0, flags, sample_counts=True)
        rest[1].setflags(write=False)
    img.setflags(write=False)
    return (img,) + tuple(rest)


def _multi_equals_one_device(m, case, br, dilates, flags=EXACT):
    name, W, H, nsub, ends, target = FRAMES[case]
    p = _p(case, flags, band_rows=br)
    got = np.zeros((H * W, 3))
    m.render_denoised(got, p)
    assert np.array_equal(got, _one_device(case, "plain", 0, flags)[0]), "render_denoised"
    got = np.zeros((H * W, 3))
    rep = m.render_to_noise_denoised(got, p, target, FLOOR, FRAC[case], ends[0])
    want = _one_device(case, "to_noise", 0, flags)
    assert rep == want[1] and np.array_equal(got, want[0]), "render_to_noise_denoised"
    for d in dilates:
        got = np.zeros((H * W, 3))
        rep, counts = m.render_adaptive_denoised(got, p, target, FLOOR, 0.0, ends[0], d, sample_counts=True)
        want = _one_device(case, "adaptive", d, flags)
        assert np.array_equal(counts, want[2]) and rep == want[1], ("render_adaptive_denoised", d)
        assert np.array_equal(got, want[0]), ("render_adaptive_denoised", d)


@pytest.mark.parametrize("case,L,br", [(c, L, br) for c in ("A", "C") for L in (1, 2, 3) for br in (1, 4)]
                         + [("33x21", L, 2) for L in (1, 2, 3)])
def test_multi_drivers_equal_the_one_device_drivers(case, L, br):
    """Every local shard count, band_rows and dilate: the filtered images of the three multi-device drivers
    equal the one-device drivers', and the adaptive driver's counts and every report field do."""
    _require_gpu()
    name, W, H, nsub, ends, target = FRAMES[case]
    want = _one_device(case, "adaptive", 1)
    assert want[1]["passes"] >= 2 and want[2].min() < want[2].max()  # the comparison proves something
    assert not np.array_equal(want[0], _one_device(case, "plain")[0])
    with ptgpu.MultiContext(*_scene(name, W, H), [0], local_shards=L) as m:
        _multi_equals_one_device(m, case, br, (0, 1, 8))


def test_multi_drivers_fast_mode_light_sampling_and_a_second_frame():
    _require_gpu()
    name, W, H, nsub, ends, target = FRAMES["A"]
    with ptgpu.MultiContext(*_scene(name, W, H), [0], local_shards=3) as m:
        for flags in (0, LS):
            _multi_equals_one_device(m, "A", 2, (1,), flags)
        # a frame of another size on the same context (its buffers grow), then the first size again
        scn, cam = _scene(name, W, H)
        want, got = np.zeros((21 * 33, 3)), np.zeros((21 * 33, 3))
        ptgpu.render_denoised(scn, cam, want, 33, 21, 8, nsub, SEED, 0, EXACT)
        m.render_denoised(got, ptgpu.make_params(33, 21, 8, nsub, SEED, 2, flags=EXACT))
        assert np.array_equal(got, want)
        acc = np.zeros((H * W, 3))
        for k in (1, 2):  # the drivers ADD
            m.render_denoised(acc, _p("A", band_rows=4))
            assert np.array_equal(acc, k * np.asarray(_one_device("A", "plain")[0]))


def test_one_rank_communicator_runs_the_gathers():
    _require_gpu()
    name, W, H, _, _, _ = FRAMES["A"]
    with ptgpu.MultiContext(*_scene(name, W, H), [0]) as m:
        assert m.comm_info() == [(1, 0, 0)]  # a real communicator: ncclGather, not device copies
        _multi_equals_one_device(m, "A", 1, (1,))
        assert m.comm_info() == [(1, 0, 0)]


def test_two_devices():
    _require_gpu()
    if torch.cuda.device_count() < 2:
        pytest.skip(f"needs 2 GPUs, {torch.cuda.device_count()} visible")
    name, W, H, _, _, _ = FRAMES["A"]
    try:
        for cur in (1, 0):  # the caller's device is restored
            torch.cuda.set_device(cur)
            with ptgpu.MultiContext(*_scene(name, W, H), [0, 1]) as m:
                assert [r for r, _, _ in m.comm_info()] == [2, 2]
                _multi_equals_one_device(m, "A", 1, (0, 1, 8))
                assert torch.cuda.current_device() == cur
    finally:
        torch.cuda.set_device(0)


# ---- 5. a failing gather ----------------------------------------------------------------------------
def test_gather_fault_breaks_the_context_as_the_frame_gathers_does():
    _require_gpu()
    name, W, H, nsub, ends, target = FRAMES["A"]
    scn, cam = _scene(name, W, H)
    p = _p("A")
    m = ptgpu.MultiContext(scn, cam, [0])
    img = np.zeros((H * W, 3))
    m.render_denoised(img, p)  # a good frame first
    assert np.array_equal(img, _one_device("A", "plain")[0])
    m.inject_gather_fault_(0)
    with pytest.raises(ptgpu.PtgError, match="ncclGather"):
        m.render_denoised(img, p)
    for call in (lambda: m.render_denoised(img, p), lambda: m.render_adaptive_denoised(img, p, target),
                 lambda: m.resolve_active_denoised(np.zeros((H, W, 3), np.float32), p)):
        with pytest.raises(ptgpu.PtgError, match="aborted"):
            call()
    m.close()
    again = np.zeros((H * W, 3))  # the device is still usable
    ptgpu.render_denoised(scn, cam, again, W, H, ends[-1], nsub, SEED, 0, EXACT)
    assert np.array_equal(again, _one_device("A", "plain")[0])


# ---- 6. the pieces keep the state -----------------------------------------------------------------------
@pytest.mark.parametrize("L,br", [(3, 2), (2, 1)])
def test_resolve_active_denoised_keeps_the_adaptive_state(L, br):
    """The root's own context computes the whole frame's features with shard_count 1 parameters between the
    passes of ITS shard: its list, counts and sums survive."""
    _require_gpu()
    name, W, H, nsub, ends, target = FRAMES["A"]
    scn, cam = _scene(name, W, H)
    p = _p("A", band_rows=br)
    res = []
    for with_call in (False, True):
        with ptgpu.MultiContext(scn, cam, [0], local_shards=L) as m:
            m.reset_accumulation(p)
            m.set_active_mask(p)
            m.accumulate_active(p, 4)
            st = [m.select_active(p, target, FLOOR, 1)]
            mid = np.zeros((H, W, 3), np.float32)
            if with_call:
                m.resolve_active_denoised(mid, p)
                assert mid.mean() > 0
            m.accumulate_active(p, 4)  # the list built before the call
            if with_call:
                m.resolve_active_denoised(mid, p)
            st.append(m.select_active(p, target, FLOOR, 1))
            m.accumulate_active(p, 8)
            img = m.resolve_active(np.zeros((H, W, 3), np.float32), p)
            res.append((m.read_sample_counts(p), img, np.stack(st)))
    assert len(np.unique(res[0][0])) >= 3 and res[0][0].max() == 16  # the later passes were adaptive ones
    for a, b in zip(*res):
        assert np.array_equal(a, b)


def test_noise_active_keeps_the_adaptive_state():
    _require_gpu()
    name, W, H, nsub, ends, target = FRAMES["A"]
    p = _p("A")
    res = []
    for with_call in (False, True):
        with ptgpu.Context(*_scene(name, W, H)) as ctx:
            ctx.reset_accumulation(p)
            ctx.set_active_mask(p)
            ctx.accumulate_active(p, 4)
            ctx.select_active(p, target, FLOOR, 1)
            if with_call:
                _noise_active(ctx, p)
            ctx.accumulate_active(p, 4)
            if with_call:
                _noise_active(ctx, p)
            ctx.select_active(p, target, FLOOR, 1)
            ctx.accumulate_active(p, 8)
            res.append((_counts(ctx, p), _image(ctx, p)) + _moments(ctx, p))
    assert len(np.unique(res[0][0])) >= 3 and res[0][0].max() == 16  # the later passes were adaptive ones
    for a, b in zip(*res):
        assert np.array_equal(a, b)


def test_pieces_errors_and_state_rules():
    _require_gpu()
    name, W, H, nsub, ends, target = FRAMES["A"]
    scn, cam = _scene(name, W, H)
    p, pm = _p("A", band_rows=2), _p("A", EXACT | MOM, band_rows=2)
    f32 = np.zeros((H, W, 3), np.float32)
    with ptgpu.Context(scn, cam) as ctx:
        ctx.reset_accumulation(pm)
        ctx.accumulate(pm, 0, 4)
        with pytest.raises(ptgpu.PtgError, match=r"\(-1\).*ptg_accumulate_device pass"):
            ctx.noise_active(pm, FLOOR)  # after a uniform pass, until the next reset
        ctx.reset_accumulation(p)
        with pytest.raises(ptgpu.PtgError, match=r"\(-1\).*floor"):
            ctx.noise_active(p, 0.0)
        ctx.set_active_mask(p)
        ctx.accumulate_active(p, 2)
        with pytest.raises(ptgpu.PtgError, match=r"\(-1\).*adaptive passes"):
            ctx.noise(p, 2, 0.0, FLOOR)  # ptg_noise_device keeps refusing adaptive sums
    with ptgpu.MultiContext(scn, cam, [0], local_shards=3) as m:
        m.reset_accumulation(pm)
        m.accumulate(pm, 0, 4)
        with pytest.raises(ptgpu.PtgError, match=r"\(-1\).*samples"):
            m.resolve_denoised(f32, pm, 1)
        with pytest.raises(ptgpu.PtgError, match=r"\(-1\).*ptg_accumulate_device pass"):
            m.resolve_active_denoised(f32, pm)
        want = m.resolve(np.zeros_like(f32), pm, 4)
        k0 = ptgpu.denoise_defaults()
        k0.iterations, k0.pixel_spread = 0, 0.0
        assert np.array_equal(m.resolve_denoised(f32, pm, 4, k0), want)  # iterations 0: the resolve
        a = m.resolve_denoised(np.zeros_like(f32), pm, 4).copy()
        assert not np.array_equal(a, want)
        m.accumulate(pm, 4, 8)  # the sums were kept
        img = np.zeros((H * W, 3))
        ptgpu.render_denoised(scn, cam, img, W, H, 8, nsub, SEED, 0, EXACT)
        assert np.array_equal(m.resolve_denoised(f32, pm, 8).reshape(-1, 3).astype(np.float64), img)
        m.reset_accumulation(p)
        m.set_active_mask(p)
        m.accumulate_active(p, 2)
        with pytest.raises(ptgpu.PtgError, match=r"\(-1\).*adaptive passes"):
            m.resolve_denoised(f32, pm, 2)
        with pytest.raises(ptgpu.PtgError, match=r"\(-1\).*iterations"):
            bad = ptgpu.denoise_defaults()
            bad.iterations = 9
            m.resolve_active_denoised(f32, p, bad)


# ---- 7. acceptance ------------------------------------------------------------------------------------------
# Box 64x48, nsub 2, the plain estimator, the filter's defaults.  The settings were fixed on the CPU first
# (DESIGN.md "Denoising": oracle sums through tests/test_gpu_adaptive.py's simulation, the host filter).
# Passes end at 4, 8 and 16 samples per sub-pixel; counts of 4, 8, 12 and 16 occur.
ACCEPT = dict(samples=16, rel_error=0.3, floor=FLOOR, max_fraction=0.0, min_samples=4, dilate=1)


def test_filtered_adaptive_frame_is_nearer_the_converged_frame():
    """RMSE against ptg_render_device's frame at 4096 samples per sub-pixel with light sampling (the existing
    acceptance reference): the filtered adaptive frame's is below the unfiltered one's."""
    _require_gpu()
    W, H, nsub = 64, 48, 2
    scn = ptgpu.make_scene("box", W, H)
    cam = ptgpu.camera.with_config(scn.camera_parameters)
    with ptgpu.Context(scn, cam, device=0) as ctx:
        ref = torch.zeros((H, W, 3), dtype=torch.float32, device=DEV)
        ctx.render_device(ref, ptgpu.make_params(W, H, 4096, nsub, flags=LS))
        torch.cuda.synchronize()
        ref = ref.cpu().numpy().astype(np.float64)
    noisy, den = np.zeros((H, W, 3)), np.zeros((H, W, 3))
    kw = dict(ACCEPT, num_subpixels=nsub, device=0, sample_counts=True)
    rep, counts = ptgpu.render_adaptive(scn, cam, noisy, W, H, **kw)
    rep2, counts2 = ptgpu.render_adaptive_denoised(scn, cam, den, W, H, **kw)
    assert rep == rep2 and np.array_equal(counts, counts2) and len(np.unique(counts)) >= 2
    rmse = lambda a: float(np.sqrt(((a - ref) ** 2).mean()))  # noqa: E731
    print(f"adaptive box: mean samples {rep['mean_samples']:.2f}, RMSE noisy {rmse(noisy):.5f} filtered "
          f"{rmse(den):.5f} ratio {rmse(den) / rmse(noisy):.3f}")
    assert rmse(den) < rmse(noisy)


# ---- 8. the command-line tool -------------------------------------------------------------------------------
def test_cli_filter(tmp_path):
    _require_gpu()
    cli = os.path.join(os.path.dirname(ptgpu.LIB_PATH), "pt_render_gpu")
    W, H, spp = 64, 48, 64

    def run(tag, *extra):
        out = tmp_path / f"{tag}.ppm"
        r = subprocess.run([cli, "--scene", "box", "--width", str(W), "--height", str(H), "--format", "p6",
                            "--spp", str(spp), "--out", str(out), *extra], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        return out.read_bytes(), r.stderr

    head = len(f"P6\n{W} {H}\n255\n")
    # --filter alone writes byte for byte what --denoise writes, also with an iteration count and a listed device
    assert run("f", "--filter")[0] == run("d", "--denoise")[0]
    assert run("f3", "--filter", "--denoise-iterations", "3")[0] == run("d3", "--denoise", "--denoise-iterations", "3")[0]
    assert run("fl", "--filter", "--devices", "0")[0] == run("d", "--denoise")[0]
    assert run("fn", "--filter", "--noise-target", "1000", "--min-spp", "16")[0] == \
        run("dn", "--denoise", "--noise-target", "1000", "--min-spp", "16")[0]
    # --filter --noise-target 0.1 --adaptive --spp-map runs and writes both files
    spm = tmp_path / "map.pgm"
    more = ("--spp", "256", "--min-spp", "16")  # passes of 4, 8, ... 64 samples per sub-pixel
    got, err = run("fa", "--filter", "--noise-target", "0.1", "--adaptive", "--spp-map", str(spm), *more)
    assert len(got) == head + W * H * 3 and "noise: adaptive" in err
    # ... and the image is ptgpu.render_adaptive_denoised's after the tool's output conversion (compared as
    # tests/test_gpu_denoise.py's CLI test compares: equal up to one 8-bit step where two pow() round a tie apart)
    scn = ptgpu.make_scene("box", W, H)
    cam = ptgpu.camera.with_config(scn.camera_parameters)
    want = np.zeros((H, W, 3))
    rep, counts = ptgpu.render_adaptive_denoised(scn, cam, want, W, H, 64, 0.1, 0.01, 0.01, 4, 1, 2, device=0,
                                                 sample_counts=True)
    assert len(np.unique(counts)) >= 2
    v = np.round(np.clip(want, 0, 1) ** (1 / 2.2) * 255).astype(np.int16).reshape(-1)
    d = np.abs(np.frombuffer(got[head:], dtype=np.uint8).astype(np.int16) - v)
    assert d.max() <= 1 and (d != 0).sum() <= 2
    assert counts.max() <= 255 and spm.read_bytes() == f"P5\n{W} {H}\n255\n".encode() + counts.astype(np.uint8).tobytes()
    assert got != run("a", "--noise-target", "0.1", "--adaptive", *more)[0]  # the filter did something
