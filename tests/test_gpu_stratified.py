"""PTG_FLAG_STRATIFIED (scrambled Sobol' pairs for the jitter, the lens and the
first hit, include/ptgpu.h "Stratified sampling") on the GPU.

1. The sequence to the bit: Context.sampler_pairs on every path of a 64x48
   frame, nsub 2, samples 0..63, against the numpy restatement
   (tests/strat_ref.py); the (0,2) property of the GPU's integers; no
   dependence on shard_count and band_rows.
2. The identities, bit for bit, 64x48 at 8 samples, box / simple /
   synthetic:300, fast and exact, with and without light sampling: the flagged
   one-shot frame equals progressive passes [0,3) + [3,8) without and with
   PTG_FLAG_MOMENTS, any chunk_samples, 3 shards, a ptg_multi of one device
   and an adaptive frame whose mask keeps every pixel; after an adaptive frame
   with a real mask a pixel with count n equals the flagged frame at n
   samples; and the flagged frame differs from the unflagged one.
3. Against the definition: trace_samples in exact mode on simple and
   zoo:sixteen, 32x24, 4 samples (12,288 paths), with and without the light
   list, by test_exact_mode_paths_against_the_oracle's criterion with
   strat_ref in float64 as the definition and strat_ref in float32 as the
   yardstick; and REFERENCE_F64 | STRATIFIED frames of the same scenes against
   strat_ref in float64 by check_matches_mode_a_xs's criterion.
4. Unbiased, and worth having: flagged against plain kernels on raw sums, 16
   seeds per side, the scenes and sample counts of
   tests/test_stratified_host.py, fast mode, through two_sample_check; the
   median variance ratio plain / flagged is printed per scene, and on simple
   it is at least 0.6 of the figure strat_ref reproduces on the CPU.  box:
   its figure is printed, nothing asserted.

Measured on an MI355X (`pytest -s` prints each line).  Per path against the
definition, max |diff| where the segment counts agree (the float32
restatement's in brackets), no path with another count: simple 2.5e-5
(1.6e-4), simple + lights 4.1e-5 (6.7e-3), sixteen 4.5e-5 (4.1e-4), sixteen +
lights 3.0e-4 (4.6e-2).  REFERENCE_F64 | STRATIFIED: max |diff| 0, every pixel
identical, on all four.  Variance plain / stratified, median (sum): simple
2.38 (2.54) against the CPU's 2.37 (2.54), beside 4.29 (7.56), sixteen 1.82
(1.19), box 1.07 (1.38); two_sample_check: frac 0, mean z +0.011, -0.006,
+0.010.
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import light_zoo as zoo  # noqa: E402
import ptgpu  # noqa: E402
import strat_ref  # noqa: E402
import test_stratified_host as host  # noqa: E402
from test_gpu_statistical import two_sample_check  # noqa: E402

SEED = 0x5EED0001
EXACT = ptgpu.FLAG_EXACT_MATH
MOM = ptgpu.FLAG_MOMENTS
LS = ptgpu.FLAG_LIGHT_SAMPLING
ST = ptgpu.FLAG_STRATIFIED
MODES = pytest.mark.parametrize("mode", [0, EXACT], ids=["fast", "exact"])
SIDES = pytest.mark.parametrize("ls", [0, LS], ids=["plain", "ls"])


def _require_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a visible MI355X")


@functools.lru_cache(maxsize=None)
def _scene(name, W, H):
    if name.startswith("zoo:"):
        assert W * zoo.H == H * zoo.W
        scn = zoo.CASES[name[4:]]()
    else:
        scn = ptgpu.make_scene(name, W, H)
    return scn, ptgpu.camera.with_config(scn.camera_parameters)


def _rows(p):
    return ptgpu.shard_rows(p.height, p.band_rows, p.shard_count)


def _frame(ctx, p):
    out = torch.full((_rows(p) * p.width * 3,), -7.0, dtype=torch.float32, device="cuda")
    ctx.render_device(out, p)
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(_rows(p), p.width, 3)


def _resolved(ctx, p, n):
    out = torch.full((_rows(p) * p.width * 3,), -7.0, dtype=torch.float32, device="cuda")
    ctx.resolve(out, p, n)
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(_rows(p), p.width, 3)


def _s1(ctx, p):
    shape = (_rows(p), p.width, p.num_subpixels ** 2, 3)
    s1 = torch.full((int(np.prod(shape)),), -1, dtype=torch.int64, device="cuda")
    ctx.read_moments(p, s1, None)
    torch.cuda.synchronize()
    return s1.cpu().numpy().view(np.uint64).reshape(shape)


def _coords(W, H, nsub, n):
    """Every path of the frame in the order (row, x, sy, sx, sample): x, y (from the bottom), sx, sy, sample."""
    row, x, sy, sx, k = np.meshgrid(np.arange(H), np.arange(W), np.arange(nsub), np.arange(nsub), np.arange(n),
                                    indexing="ij")
    return np.stack([x, H - 1 - row, sx, sy, k], axis=-1).reshape(-1, 5).astype(np.int32)


# ---- 1: the sequence --------------------------------------------------------------------
def test_sampler_pairs_equal_the_definition_to_the_bit():
    _require_gpu()
    W, H, nsub, n = 64, 48, 2, 64
    coords = _coords(W, H, nsub, n)
    ref = strat_ref.pairs(W, nsub, SEED, coords)
    with ptgpu.Context(*_scene("box", W, H)) as ctx:
        dev = torch.from_numpy(coords).cuda()
        got = ctx.sampler_pairs(dev, ptgpu.make_params(W, H, n, nsub, SEED, flags=ST))
        cut = ctx.sampler_pairs(dev, ptgpu.make_params(W, H, n, nsub, SEED, 2, 1, 3, flags=ST))
        other = ctx.sampler_pairs(dev, ptgpu.make_params(W, H, n, nsub, SEED + 1, flags=ST))
        torch.cuda.synchronize()
    got = got.cpu().numpy().view(np.uint32)
    assert np.array_equal(got, ref)
    assert np.array_equal(cut.cpu().numpy().view(np.uint32), got)  # shard_count 3, band_rows 2: the same integers
    assert not np.array_equal(other.cpu().numpy().view(np.uint32), got)
    q = got.reshape(H * W * nsub * nsub, n, 4, 2)
    assert q.max() < 1 << 24
    for j in range(4):  # every sub-pixel's pair j over samples 0..63: blocks of 2..64
        assert strat_ref.is_02_sequence(q[:, :, j, 0], q[:, :, j, 1], max_m=6), j
    assert len({q[:, :, j, 0].tobytes() for j in range(4)}) == 4  # the pair numbers differ


# ---- 2: the identities ------------------------------------------------------------------
W2, H2, N2 = 64, 48, 8


@MODES
@SIDES
@pytest.mark.parametrize("name", ["box", "simple", "synthetic:300"])
def test_flagged_frame_does_not_depend_on_how_it_is_cut(name, ls, mode):
    _require_gpu()
    f = mode | ls | ST

    def params(flags=f, n=N2, **kw):
        return ptgpu.make_params(W2, H2, n, 2, SEED, kw.pop("band_rows", 1), flags=flags, **kw)

    scn, cam = _scene(name, W2, H2)
    with ptgpu.Context(scn, cam) as ctx:
        one = _frame(ctx, params())
        assert one.min() >= 0.0
        assert not np.array_equal(one, _frame(ctx, params(mode | ls)))  # the flag did something
        for flags in (f, f | MOM):  # progressive passes
            p = params(flags)
            ctx.reset_accumulation(p)
            ctx.accumulate(p, 0, 3)
            ctx.accumulate(p, 3, N2)
            assert np.array_equal(one, _resolved(ctx, p, N2)), flags
        ctx.reset_accumulation(params())
        for chunk in (1, 3, 5):
            assert np.array_equal(one, _frame(ctx, params(chunk_samples=chunk))), chunk
        whole = np.full((H2, W2, 3), -7.0, dtype=np.float32)
        for rank in range(3):
            p = params(band_rows=2, shard_rank=rank, shard_count=3)
            rows = ptgpu.slab_to_image_rows(H2, 2, rank, 3)
            whole[rows[rows >= 0]] = _frame(ctx, p)[rows >= 0]
        assert np.array_equal(one, whole)
        # adaptive, every pixel active: two passes
        p = params()
        ctx.reset_accumulation(p)
        ctx.set_active_mask(p)
        ctx.accumulate_active(p, 3)
        ctx.accumulate_active(p, N2 - 3)
        img = torch.full((H2 * W2 * 3,), -7.0, dtype=torch.float32, device="cuda")
        ctx.resolve_active(img, p)
        torch.cuda.synchronize()
        assert np.array_equal(one, img.cpu().numpy().reshape(H2, W2, 3))
        # adaptive with a real mask: a pixel holding n samples equals the flagged frame at n samples
        checker = ((np.arange(W2)[None, :] + np.arange(H2)[:, None]) % 2).astype(np.uint8)
        ctx.reset_accumulation(p)
        ctx.set_active_mask(p)
        ctx.accumulate_active(p, 3)
        ctx.set_active_mask(p, torch.from_numpy(checker.reshape(-1).copy()).cuda())
        ctx.accumulate_active(p, 5)
        counts = torch.full((H2 * W2,), -1, dtype=torch.int32, device="cuda")
        ctx.read_sample_counts(p, counts)
        ctx.resolve_active(img, p)
        torch.cuda.synchronize()
        counts = counts.cpu().numpy().reshape(H2, W2)
        got = img.cpu().numpy().reshape(H2, W2, 3)
        assert np.array_equal(counts, 3 + 5 * checker.astype(np.int32))
        ctx.reset_accumulation(p)
        assert np.array_equal(got[counts == 8], one[counts == 8])
        three = _frame(ctx, params(n=3))
        assert np.array_equal(got[counts == 3], three[counts == 3])
        assert not np.array_equal(three, _frame(ctx, params(mode | ls, n=3)))
    with ptgpu.MultiContext(scn, cam, [0]) as m:  # a ptg_multi of one device
        img64 = np.zeros((H2 * W2, 3))
        m.render(img64, params())
    assert np.array_equal(one, img64.reshape(H2, W2, 3).astype(np.float32))


# ---- 3: against the definition ------------------------------------------------------------
PATH_SAMPLES = 4
PATH_CASES = [("simple", False), ("simple", True), ("sixteen", False), ("sixteen", True)]


def _path_scene(name):
    """(scene, camera, the scene's light list) of a per-path case at 32x24."""
    if name == "simple":
        scn, cam = _scene("simple", zoo.W, zoo.H)
        return scn, cam, tuple(ptgpu.light_list(scn, cam))
    scn, cam, ls = zoo.make(name)
    return scn, cam, tuple(ls)


@functools.lru_cache(maxsize=None)
def _definition(name, listed):
    """coords, then the definition's radiance and segment count per path (strat_ref in float64), then the
    float32 restatement's.  Read-only."""
    scn, cam, ls = _path_scene(name)
    sp, ca = zoo.oracle_arrays(scn, cam)
    coords = _coords(zoo.W, zoo.H, zoo.NSUB, PATH_SAMPLES)
    lights = ls if listed else ()
    E, segs = strat_ref.trace(sp, ca, zoo.W, zoo.H, zoo.NSUB, SEED, coords, lights, np.float64)
    E32, segs32 = strat_ref.trace(sp, ca, zoo.W, zoo.H, zoo.NSUB, SEED, coords, lights, np.float32)
    for a in (coords, E, segs, E32, segs32):
        a.setflags(write=False)
    return coords, E, segs, E32, segs32


@pytest.mark.parametrize("name,listed", PATH_CASES)
def test_exact_mode_paths_against_the_definition(name, listed):
    """The criterion of tests/test_gpu_light_sampling.py's per-path test: over the paths whose segment counts
    agree the kernel differs from the definition by at most 4 times what the float32 restatement does, and at
    most 0.5 % of the paths end with another segment count.  Float32 restatement alone, on the CPU: simple
    with lights 0.081 % of the paths differ in the count; the kernel's figures are printed."""
    _require_gpu()
    coords, E, segs, E32, segs32 = _definition(name, listed)
    ok32 = segs32 == segs
    err, share = float(np.abs(E32.astype(np.float64) - E)[ok32].max()), float(1.0 - ok32.mean())
    assert share <= 0.005, share  # the yardstick alone
    scn, cam, ls = _path_scene(name)
    assert bool(ls)
    p = ptgpu.make_params(zoo.W, zoo.H, PATH_SAMPLES, zoo.NSUB, SEED, 1, flags=EXACT | ST | (LS if listed else 0))
    with ptgpu.Context(scn, cam) as ctx:
        got, gsegs = ctx.trace_samples(torch.from_numpy(coords.copy()).cuda(), p)
        torch.cuda.synchronize()
    got, gsegs = got.cpu().numpy().astype(np.float64), gsegs.cpu().numpy()
    agree = gsegs == segs
    d = float(np.abs(got - E)[agree].max())
    print(f"{name}{' + light sampling' if listed else ''}: kernel against the definition per path: max |diff| {d:.3e} "
          f"where the segment counts agree (float32 restatement {err:.3e}, bound 4x), "
          f"{100 * (1 - agree.mean()):.3f} % of {len(segs)} paths differ in the count (restatement "
          f"{100 * share:.3f} %)")
    assert 1.0 - agree.mean() <= 0.005
    assert d <= 4.0 * err, (d, err)


@pytest.mark.parametrize("name,listed", PATH_CASES)
def test_reference_f64_matches_the_definition(name, listed):
    """REFERENCE_F64 | STRATIFIED against strat_ref in float64 by check_matches_mode_a_xs's criterion: the
    frame (each sub-pixel's r += c / samps in sample order, clamped, the sub-pixels added with weight
    1 / nsub^2) within 1e-9 everywhere, more than 99 % of the pixels identical, segment counts equal."""
    _require_gpu()
    W, H, nsub, n = zoo.W, zoo.H, zoo.NSUB, PATH_SAMPLES
    coords, _, segs, _, _ = _definition(name, listed)
    scn, cam, ls = _path_scene(name)
    sp, ca = zoo.oracle_arrays(scn, cam)
    # (the definition in the reference-arithmetic mode's own association and sin / cos: to the last bit)
    E, segs64 = strat_ref.trace(sp, ca, W, H, nsub, SEED, coords, ls if listed else (), np.float64, ref64_ops=True)
    assert np.array_equal(segs64, segs)
    flags = ptgpu.FLAG_REFERENCE_F64 | ST | (LS if listed else 0)
    c = E.reshape(H, W, nsub * nsub, n, 3)
    acc = np.zeros((H, W, nsub * nsub, 3))
    for k in range(n):
        acc = acc + c[:, :, :, k] * (1.0 / n)
    ref = np.zeros((H, W, 3))
    for j in range(nsub * nsub):
        ref = ref + np.clip(acc[:, :, j], 0.0, 1.0) * (1.0 / (nsub * nsub))
    img = np.zeros((H * W, 3))
    ptgpu.render(scn, cam, img, W, H, n, nsub, SEED, flags=flags)
    d = np.abs(img.reshape(H, W, 3) - ref)
    same = float((d.max(axis=2) == 0).mean())
    print(f"{name}{' + light sampling' if listed else ''}: max |diff| {d.max():.3e}, pixels bit-identical "
          f"{100 * same:.2f} %")
    out = torch.zeros(H * W * 3, dtype=torch.float32, device="cuda")
    sg = torch.zeros(1, dtype=torch.int64, device="cuda")
    with ptgpu.Context(scn, cam) as ctx:
        ctx.render_device(out, ptgpu.make_params(W, H, n, nsub, SEED, flags=flags), sg)
        torch.cuda.synchronize()
    assert d.max() <= 1e-9, d.max()
    assert same > 0.99
    assert int(sg.item()) == int(segs.sum())


# ---- 4: unbiased, and worth having ---------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gpu_seed_stats(name, W, H, n):
    """Per side (plain: seeds 0..15, flagged: the disjoint seeds 32..47): mean and variance over the seeds of
    the raw per-pixel-channel mean sum_sub S1 2^-32 / (n nsub^2).  Fast mode, the scene with the light list
    tests/test_stratified_host.py gives it.  Read-only."""
    if name in host.SCENES:
        scn, cam, ls = host.scene(name)
    else:
        (scn, cam), ls = _scene(name, W, H), ()
    out = []
    with ptgpu.Context(scn, cam) as ctx:
        for side, runs in ((0, host.PLAIN_A), (ST, host.FLAGGED)):
            means = []
            for r in runs:
                p = ptgpu.make_params(W, H, n, 2, host.run_seed(r), flags=MOM | side | (LS if ls else 0))
                ctx.reset_accumulation(p)
                ctx.accumulate(p, 0, n)
                means.append(_s1(ctx, p).astype(np.float64).sum(axis=2) * 2.0 ** -32 / (n * 4))
            ctx.reset_accumulation(p)
            g = np.stack(means)
            out.append((g.mean(0), g.var(0, ddof=1)))
    for m, v in out:
        m.setflags(write=False)
        v.setflags(write=False)
    return tuple(out)


@pytest.mark.parametrize("name", host.SCENES)
def test_unbiased_against_the_plain_kernels(name):
    _require_gpu()
    (mp, vp), (ms, vs) = _gpu_seed_stats(name, host.W, host.H, host.SAMPLES[name])
    assert not np.array_equal(ms, mp)
    med, tot = host.variance_ratio(vp, vs)
    print(f"{name} at {host.SAMPLES[name]} samples: variance plain / stratified, median {med:.3f}, sum {tot:.3f}")
    print(name, two_sample_check(ms, vs, mp, vp, host.RUNS))


def test_variance_drops_on_simple():
    """The GPU's median variance ratio on simple is at least 0.6 of what the definition gives on the CPU with
    the same seeds and sample count (a ratio of two 16-run variances per channel is noisy, its median over
    2,304 channels is not): a sampler that silently fell back to xorshift gives 1 and fails."""
    _require_gpu()
    cpu_med, cpu_tot = host.cpu_variance_ratio("simple")
    assert 2.0 <= cpu_med <= 3.2, cpu_med  # the prototype's 2.5, reproduced (tests/test_stratified_host.py)
    (_, vp), (_, vs) = _gpu_seed_stats("simple", host.W, host.H, host.SAMPLES["simple"])
    med, tot = host.variance_ratio(vp, vs)
    print(f"simple: variance plain / stratified on the GPU, median {med:.3f}, sum {tot:.3f}; the definition on the "
          f"CPU: {cpu_med:.3f}, {cpu_tot:.3f}")
    assert med >= 0.6 * cpu_med, (med, cpu_med)


def test_variance_of_box_is_reported():
    _require_gpu()
    (_, vp), (_, vs) = _gpu_seed_stats("box", 32, 24, 64)
    med, tot = host.variance_ratio(vp, vs)
    print(f"box 32x24 at 64 samples: variance plain / stratified, median {med:.3f}, sum {tot:.3f} (nothing asserted)")
