"""Exact ties in the nearest-hit scan, on every kernel.

include/ptgpu.h (ptg_scene_layout): when two spheres give exactly the same
root, a linear scene (64 spheres or fewer) keeps the sphere visited first and
a BVH scene the lowest scene index.  The scenes of tests/tie_scenes.py hold
spheres of equal geometry that look different -- pasted twice, a lamp's shell
on a body of the same radius -- so a kernel with the rule wrong shows another
picture on 36 .. 99 % of the pixels (tests/test_tie_scenes_host.py, on the
oracle).  The code that exists for the rule alone: update_lex's (t == tb) &
(sid < best) clause, leaf_spheres reading a scene index on t <= tb, the merge
of the helpers' results in bvh_leaf_split, the huge spheres' loop of
bvh_start, the strict cross-multiplied compare of the linear scan and the
strict < of ref64.hpp.

1. Exact mode: image and segment count against the oracle's Mode B,
   max |diff| == 0; launch info and the counter identities of
   tests/test_gpu_scene_shapes.py.
2. The trace kernel: 1,000 seeded paths of a 160x120 frame against
   po.sample_f32, bytes and segment counts.
3. Render kernel == trace kernel (tests/test_gpu_fast_paths.py's identity) in
   both arithmetic modes: render_kernel and moments_kernel.
4. The active-list path (gather_kernel): one masked pass, the sums against the
   oracle's per-path values.
5. Order independence on the device (BVH cases): a permutation of the sphere
   list that keeps the order inside every group of equal geometry gives a
   bit-identical frame in exact and in fast mode -- the fast BVH kernels have
   no bit-exact oracle, this is their tie test -- and the same permutation
   with the groups reversed does not.  Nothing of the kind is claimed for
   linear scenes (near-ties below an ulp may move).
6. PTG_FLAG_REFERENCE_F64 against Mode A/xs (tests/test_gpu_ref64.py's check;
   it is the test that found the device math library's sin / cos a last bit
   off glibc's too often: csrc/sincos_cr.hpp).
7. The lamp cases with PTG_FLAG_REFERENCE_F64 | PTG_FLAG_LIGHT_SAMPLING
   against the oracle's light-list mode, every pixel identical.  (Both fp32
   modes against that definition and the pool kernels against the trace
   kernel: the lamp entries of tests/test_gpu_light_sampling.py.)

The `near_*` cases (twins 1 or 8 float32 ulps apart in radius: no ties) run
under 1 to 3 against Mode B only.  Fast against exact per path and the
first-hit features: the tie entries of tests/test_gpu_fast_paths.py and
tests/test_gpu_denoise.py.
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import light_zoo as zoo  # noqa: E402
import ptgpu  # noqa: E402
import pyoracle as po  # noqa: E402
import tie_scenes as ts  # noqa: E402
from test_gpu_fast_paths import check_render_equals_trace  # noqa: E402
from test_gpu_noise import _quant, _sums  # noqa: E402
from test_gpu_ref64 import NT, check_matches_mode_a_xs  # noqa: E402

SEED = 0x5EED0001
EXACT = ptgpu.FLAG_EXACT_MATH
SAMPS, NSUB = 4, 2


def _require_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a visible MI355X")


def _image(ctx, p, counters=None):
    rows = ptgpu.shard_rows(p.height, p.band_rows, 1)
    out = torch.full((rows * p.width * 3,), -7.0, dtype=torch.float32, device="cuda")
    ctx.render_device(out, p, counters)
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(rows, p.width, 3)[:p.height]


# ---- 1. the exact mode against Mode B ---------------------------------------------
@functools.lru_cache(maxsize=None)
def _rendered(name):
    """One exact-mode frame of the case: (image, [nseg, ntest, nbox], launch
    info in exact mode, in fast mode, the oracle's image, its segments)."""
    W, H = ts.frame(name)
    scn, cam = ts.make(name, W, H)
    p = ptgpu.make_params(W, H, SAMPS, NSUB, SEED, flags=EXACT | ptgpu.FLAG_COUNT_TESTS)
    cnt = torch.zeros(3, dtype=torch.int64, device="cuda")
    with ptgpu.Context(scn, cam) as ctx:
        info = ctx.launch_info(p)
        fast = ctx.launch_info(ptgpu.make_params(W, H, SAMPS, NSUB, SEED))
        img = _image(ctx, p, cnt)
    ref, rsegs = po.render_xs_f32(*ts.oracle_arrays(scn, cam), W, H, SAMPS, NSUB, SEED)
    return img, cnt.cpu().tolist(), info, fast, ref, rsegs


@pytest.mark.parametrize("name", list(ts.CASES))
def test_image_and_segments_bitexact(name):
    _require_gpu()
    img, (nseg, _, _), _, _, ref, rsegs = _rendered(name)
    assert img.shape == ref.shape
    diff = np.abs(img.astype(np.float64) - ref.astype(np.float64))
    assert float(diff.max()) == 0.0, (float(diff.max()), int((diff > 0).sum()))
    assert nseg == rsegs
    assert float(ref.mean()) > 0.0


@pytest.mark.parametrize("name", list(ts.CASES))
def test_launch_info(name):
    _require_gpu()
    _, _, info, fast, _, _ = _rendered(name)
    assert info["bvh"] == fast["bvh"] == (1 if name in ts.BVH else 0)
    if name in ts.LINEAR:
        box, pairs = ts.LINEAR_LAUNCH[name]
        assert (info["box_mode"], info["wall_pairs"]) == (box, pairs)
        # the fast mode runs box mode only where no ray starts inside a wall; these walls are diffuse and
        # farther from the camera than their radius + the lens
        assert fast["box_mode"] == fast["box_walls_out"] == info["box_walls_out"] == box


@pytest.mark.parametrize("name", list(ts.CASES))
def test_counter_identities(name):
    """tests/test_gpu_scene_shapes.py's identities; twin_wall is the shape that
    module does not have: pairs without box mode.  Its x and y pairs cost one
    or two wall tests per segment each, the two z walls two."""
    _require_gpu()
    W, H = ts.frame(name)
    _, (nseg, ntest, nbox), info, _, _, _ = _rendered(name)
    n = ts.COUNTS[name]
    print(f"{name}: n {n}, nseg {nseg}, ntest {ntest}, nbox {nbox}")
    assert nseg >= W * H * NSUB * NSUB * SAMPS  # at least one segment per path
    if name in ts.BVH:
        assert 0 < ntest < n * nseg
    elif info["box_mode"]:
        assert ntest - nbox == (n - 5) * nseg and nseg <= nbox
    elif name == "twin_wall":
        assert ntest - nbox == 4 * nseg and 4 * nseg <= nbox <= 6 * nseg
    else:  # no pair: every sphere, every segment; one huge sphere (the floor)
        assert ntest == n * nseg and nbox == nseg


# ---- 2. the trace kernel ------------------------------------------------------------------
TRACE = ["twins_lin_low", "twins_room_low", "twins_bvh_low", "stack9_b", "twin_floor", "near_up1", "near_down1"]


@pytest.mark.parametrize("name", TRACE)
def test_per_path_radiance_bitexact(name):
    _require_gpu()
    W, H, n = 160, 120, 1000
    scn, cam = ts.make(name, W, H)
    rng = np.random.default_rng(7)
    coords = np.stack([rng.integers(0, W, n), rng.integers(0, H, n), rng.integers(0, 2, n),
                       rng.integers(0, 2, n), rng.integers(0, 1 << 20, n)], axis=1).astype(np.int32)
    p = ptgpu.make_params(W, H, 1, 2, SEED, flags=EXACT)
    with ptgpu.Context(scn, cam) as ctx:
        out, segs = ctx.trace_samples(torch.from_numpy(coords).cuda(), p)
        torch.cuda.synchronize()
    out = out.cpu().numpy()
    segs = segs.cpu().numpy()
    sp, ca = ts.oracle_arrays(scn, cam)
    lit = 0
    for i in range(n):
        x, y, sx, sy, s = (int(v) for v in coords[i])
        ref, rs = po.sample_f32(sp, ca, W, H, 2, SEED, x, y, sx, sy, s)
        assert segs[i] == rs, (i, coords[i])
        assert out[i].tobytes() == ref.tobytes(), (i, coords[i], out[i], ref)
        lit += bool(ref.max() > 0)
    assert lit > 0


# ---- 3. render kernel == trace kernel ---------------------------------------------------
RENDER_TRACE = {"twins_room": (37, 23), "twins_bvh_low": (48, 32), "stack9_c": (48, 32), "near_up8": (48, 32)}


@pytest.mark.parametrize("flags", [0, EXACT], ids=["fast", "exact"])
@pytest.mark.parametrize("name", list(RENDER_TRACE))
def test_render_kernel_equals_trace_kernel(name, flags):
    _require_gpu()
    W, H = RENDER_TRACE[name]
    check_render_equals_trace(name, W, H, SAMPS, NSUB, [(0, 1), (1, SAMPS)], flags=flags)


# ---- 4. the active-list path ----------------------------------------------------------------
def test_active_list_pass_holds_the_oracles_paths():
    """set_active_mask with a checkerboard + accumulate_active(3) on
    twins_bvh_low: the masked pixels hold samples [0, 3) of the oracle's
    paths (S1, S2 bit for bit), the others nothing."""
    _require_gpu()
    name, W, H, n = "twins_bvh_low", 32, 24, 3
    scn, cam = ts.make(name, W, H)
    sp, ca = ts.oracle_arrays(scn, cam)
    E = np.zeros((H, W, NSUB * NSUB, n, 3), dtype=np.float32)
    for y in range(H):  # sample_f32's y counts from the bottom: image row H - 1 - y
        for x in range(W):
            for sy in range(NSUB):
                for sx in range(NSUB):
                    for s in range(n):
                        E[H - 1 - y, x, sy * NSUB + sx, s], _ = po.sample_f32(sp, ca, W, H, NSUB, SEED, x, y, sx, sy, s)
    S1, S2 = _sums(E, 0, n)
    assert np.array_equal(S1, _quant(E).sum(axis=3, dtype=np.uint64)) and (S1 > 0).mean() > 0.05
    mask = ((np.arange(W)[None, :] + np.arange(H)[:, None]) % 2).astype(np.uint8)
    p = ptgpu.make_params(W, H, n, NSUB, SEED, 1, flags=EXACT)
    shape = (H, W, NSUB * NSUB, 3)
    with ptgpu.Context(scn, cam) as ctx:
        ctx.reset_accumulation(p)
        ctx.set_active_mask(p, torch.from_numpy(mask.reshape(-1).copy()).cuda())
        ctx.accumulate_active(p, n)
        counts = torch.full((H * W,), -1, dtype=torch.int32, device="cuda")
        ctx.read_sample_counts(p, counts)
        s1 = torch.full((int(np.prod(shape)),), -1, dtype=torch.int64, device="cuda")
        s2 = torch.full_like(s1, -1)
        ctx.read_moments(p, s1, s2)
        torch.cuda.synchronize()
        ctx.reset_accumulation(p)
    on = mask != 0
    assert np.array_equal(counts.cpu().numpy().reshape(H, W), n * mask.astype(np.int32))
    g1, g2 = (t.cpu().numpy().view(np.uint64).reshape(shape) for t in (s1, s2))
    assert np.array_equal(g1[on], S1[on]) and np.array_equal(g2[on], S2[on])
    assert not g1[~on].any() and not g2[~on].any()


# ---- 5. order independence on the device -------------------------------------------------------
@pytest.mark.parametrize("flags", [0, EXACT], ids=["fast", "exact"])
@pytest.mark.parametrize("name", ts.BVH_TIES)
def test_frame_does_not_depend_on_the_order_outside_the_groups(name, flags):
    _require_gpu()
    W, H = 48, 32
    p = ptgpu.make_params(W, H, SAMPS, NSUB, SEED, flags=flags)
    frames = []
    for scn, cam in (ts.make(name, W, H), ts.permuted(name, W, H, True), ts.permuted(name, W, H, False)):
        with ptgpu.Context(scn, cam) as ctx:
            assert ctx.launch_info(p)["bvh"] == 1
            frames.append(_image(ctx, p))
    first, kept, reversed_ = frames
    changed = int((np.abs(first - reversed_).max(axis=2) > 0).sum())
    print(f"{name} {'exact' if flags else 'fast'}: the order-keeping permutation changes "
          f"{int((np.abs(first - kept).max(axis=2) > 0).sum())} pixels, with the groups reversed {changed} of {W * H}")
    assert np.array_equal(first, kept)
    assert changed >= 0.25 * W * H  # (tests/test_tie_scenes_host.py: the oracle's share)
    if flags:
        assert np.array_equal(first, _rendered(name)[0])


# ---- 6. the reference arithmetic ------------------------------------------------------------------
@pytest.mark.parametrize("name", ["twins_lin_low", "twins_bvh_low"])
def test_reference_f64_matches_mode_a_xs(name):
    """tests/test_gpu_ref64.py's criterion: max |diff| <= 1e-9 on the double
    image, more than 99 % of the pixels bit-identical, the segment counts and
    the float slab equal.  ref64.hpp's scan with <= moves the image by 0.98.

    This test found that the 99 % clause was out of reach of the sky-lit
    clusters, ties or no ties: with the device math library's sin / cos
    twins_bvh_low had 17 of 1,536 pixels a last bit off Mode A/xs (98.89 %),
    the same 17 as the scene without the spheres that lose their ties;
    cluster_scene(60), (70), (200) alone 19, 17, 19, cluster_scene(40) 13 and
    twins_lin_low 10.  A diffuse bounce whose sin or cos is an ulp off leaves
    in a direction an ulp off, and a path that ends in the sky carries that
    into its value.  With csrc/sincos_cr.hpp (correctly rounded, as glibc's is
    on all but 0.15 % of the angles) every one of these frames equals Mode
    A/xs in every pixel; at 2 and 8 samples twins_bvh_low differs on 1 and 2
    pixels (13 and 34 before)."""
    _require_gpu()
    W, H = 48, 32
    check_matches_mode_a_xs(name, W, H, SAMPS, NSUB, scene=ts.make(name, W, H)[0])


# ---- 7. the lamp cases in the reference arithmetic with the light list -------------------------------
@pytest.mark.parametrize("name", ts.LAMPS)
def test_reference_f64_light_sampling_equals_the_oracle(name):
    """A listed light with a twin of lower index is occluded by it
    (lamp_dark_first: every shadow ray ends on the dark twin), one with its
    twin at a higher index is not.  max |diff| == 0 on the double image, the
    segment counts and the float slab, as every scene of tests/light_zoo.py
    measures today."""
    _require_gpu()
    W, H, samps = zoo.W, zoo.H, 8
    flags = ptgpu.FLAG_REFERENCE_F64 | ptgpu.FLAG_LIGHT_SAMPLING
    scn, cam = ts.make(name, W, H)
    sp, ca = ts.oracle_arrays(scn, cam)
    lights = ptgpu.light_list(scn, cam)
    assert lights == ([5, 6, 7] if name == "lamp_dark_first" else [2, 3, 4])
    img = np.zeros((H * W, 3))
    ptgpu.render(scn, cam, img, W, H, samps, NSUB, SEED, flags=flags)
    ref, rsegs = po.render_xs_f64_ls(sp, ca, W, H, samps, lights, NSUB, SEED, nthreads=NT)
    plain, _ = po.render_xs_f64(sp, ca, W, H, samps, NSUB, SEED, nthreads=NT)
    d = np.abs(img.reshape(H, W, 3) - ref)
    print(f"{name} L = {len(lights)}: max |diff| {d.max():.3e}")
    assert d.max() == 0.0
    assert not np.array_equal(ref, plain)
    segs = torch.zeros(1, dtype=torch.int64, device="cuda")
    with ptgpu.Context(scn, cam) as ctx:
        out = _image(ctx, ptgpu.make_params(W, H, samps, NSUB, SEED, flags=flags), segs)
    assert int(segs.item()) == rsegs
    assert np.array_equal(out, ref.astype(np.float32))
