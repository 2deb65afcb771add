"""The frame axis: every sub-pixel count and every unit-level kind on both
render kernels (tests/test_gpu_scene_shapes.py covers the scene axis).

num_subpixels decides how render_unit maps lanes to pixels and sub-pixels
(64 // nsub^2 pixels per wave: 64, 16, 7, 4, 2, 1, 1, 1 at nsub 1 .. 8, with
64, 64, 63, 64, 50, 36, 49, 64 valid slots), which unit level a row falls into
(csrc/launch_plan.hpp) and which epilogue produces a pixel: the in-wave
resolve, the cooperative LDS-reduced one, or HBM accumulation + resolve_kernel.

(a) whole small frames at nsub 1 .. 8 on box (linear, box mode), simple
    (linear, no wall pair) and synthetic:300 (BVH), rows ending in a partial
    pixel group, through resolve_kernel (auto chunk) and through the in-wave
    resolve (chunk_samples = samples); 2-way shards of 3-row bands at nsub 5
    and 8, whose slab rows past the image must stay untouched;
(b) frames of a few million paths that reach every level kind away from
    nsub 2; their plans are rows of tests/golden/launch_plans.json
    (tests/launch_plan_check.cpp checks them on the CPU);
(c) units of 1 .. 50 valid slots at the largest chunk (divmod_nv);
(d) the trace kernel at every nsub, and the fast render kernel against it;
(e) noise_kernel at nsub 5 and the reference-arithmetic kernel at nsub 1, 3,
    5 and 8, under their own modules' criteria.

Every image comparison in the exact mode is max |diff| == 0 with the oracle's
Mode B (oracle/pt_oracle.c).
"""
import functools
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import ptgpu  # noqa: E402
import pyoracle as po  # noqa: E402
import shape_scenes as ss  # noqa: E402
from conftest import GOLDEN  # noqa: E402
from test_gpu_fast_paths import check_render_equals_trace  # noqa: E402
from test_gpu_noise import MOM, check_slabs  # noqa: E402
from test_gpu_ref64 import check_matches_mode_a_xs  # noqa: E402

SEED = 0x5EED0001
EXACT = ptgpu.FLAG_EXACT_MATH
NT = max(1, min(16, int(os.environ.get("OMP_NUM_THREADS", "8"))))
SCENES = ["box", "simple", "synthetic:300"]


def _require_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a visible MI355X")


@functools.lru_cache(maxsize=None)
def _scene(name, W, H):
    """(scene, camera, oracle spheres, oracle camera)"""
    scn = ptgpu.make_scene(name, W, H)
    cam = ptgpu.camera.with_config(scn.camera_parameters)
    return (scn, cam) + ss.oracle_arrays(scn, cam)


def _slab(ctx, p, count=False):
    """The slab of a one-shot frame (pre-filled with -7) and, with `count`, its segments."""
    rows = ptgpu.shard_rows(p.height, p.band_rows, p.shard_count)
    out = torch.full((rows * p.width * 3,), -7.0, dtype=torch.float32, device="cuda")
    segs = torch.zeros(1, dtype=torch.int64, device="cuda") if count else None
    ctx.render_device(out, p, segs)
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(rows, p.width, 3), (int(segs.item()) if count else None)


def _progressive(ctx, p, passes):
    """The slab (pre-filled with -7) resolved after the sample passes [a, b)."""
    rows = ptgpu.shard_rows(p.height, p.band_rows, p.shard_count)
    out = torch.full((rows * p.width * 3,), -7.0, dtype=torch.float32, device="cuda")
    ctx.reset_accumulation(p)
    for a, b in passes:
        ctx.accumulate(p, a, b)
    ctx.resolve(out, p, p.samples)
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(rows, p.width, 3)


def _ragged(W, nsub):
    """The row's last pixel group is partial; from nsub 6 on (one pixel per wave) the width is odd."""
    ppw = 64 // (nsub * nsub)
    return W % ppw != 0 if ppw > 1 else W % 2 == 1


def _same(a, b):
    return float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max()) == 0.0 and np.array_equal(a, b)


# ---- (a) every sub-pixel count, whole small frames -----------------------------
# nsub -> W: two or more pixel groups of 64 // nsub^2 pixels and a partial last one
WIDTHS = {1: 70, 2: 21, 3: 17, 4: 11, 5: 7, 6: 5, 7: 5, 8: 5}
HA, NA = 6, 8


@functools.lru_cache(maxsize=None)
def _ref_image(name, W, H, n, nsub):
    _, _, sp, ca = _scene(name, W, H)
    ref, segs = po.render_xs_f32(sp, ca, W, H, n, nsub, SEED, nthreads=NT)
    ref.setflags(write=False)
    return ref, segs


@pytest.mark.parametrize("nsub", range(1, 9))
@pytest.mark.parametrize("name", SCENES)
def test_every_subpixel_count_is_exact(name, nsub):
    _require_gpu()
    W, H, n = WIDTHS[nsub], HA, NA
    assert _ragged(W, nsub)
    ref, rsegs = _ref_image(name, W, H, n, nsub)
    assert ref.mean() > 0
    scn, cam, _, _ = _scene(name, W, H)
    with ptgpu.Context(scn, cam) as ctx:
        # auto chunk: a frame this small runs one sample per unit, resolve_kernel finishes it
        auto = ptgpu.make_params(W, H, n, nsub, SEED, flags=EXACT)
        info = ctx.launch_info(auto)
        assert info["resolve_pass"] == 1 and info["bvh"] == (name == "synthetic:300")
        img, segs = _slab(ctx, auto, count=True)
        # one unit holds every sample of its pixels: the in-wave resolve
        whole = ptgpu.make_params(W, H, n, nsub, SEED, chunk_samples=n, flags=EXACT)
        assert ctx.launch_info(whole)["resolve_pass"] == 0
        img_w, segs_w = _slab(ctx, whole, count=True)
        img_p, _ = _slab(ctx, whole)  # the kernel without counters
    d = [float(np.abs(g.astype(np.float64) - ref).max()) for g in (img, img_w, img_p)]
    print(f"{name} nsub {nsub} {W}x{H}x{n}: max |diff| {d}, segments {segs} {segs_w} / {rsegs}, mean {ref.mean():.4f}")
    assert d == [0.0, 0.0, 0.0]
    assert segs == rsegs and segs_w == rsegs


# 3-row bands over 2 shards, H no multiple of 6: both ranks end on slab rows past the image
SHARD_FRAMES = {5: (13, 20), 8: (9, 20)}


@pytest.mark.parametrize("nsub", [5, 8])
@pytest.mark.parametrize("name", SCENES)
def test_shards_of_three_row_bands_are_exact(name, nsub):
    _require_gpu()
    (W, H), n = SHARD_FRAMES[nsub], 4
    assert H % 6 != 0
    ref, rsegs = _ref_image(name, W, H, n, nsub)
    assert ref.mean() > 0
    scn, cam, _, _ = _scene(name, W, H)
    total = {0: 0, n: 0}
    with ptgpu.Context(scn, cam) as ctx:
        for rank in range(2):
            m = ptgpu.slab_to_image_rows(H, 3, rank, 2)
            assert (m < 0).any()  # a slab row past the image
            for chunk in (0, n):
                p = ptgpu.make_params(W, H, n, nsub, SEED, 3, rank, 2, chunk, flags=EXACT)
                slab, segs = _slab(ctx, p, count=True)
                total[chunk] += segs
                assert _same(slab[m >= 0], ref[m[m >= 0]]), (rank, chunk)
                assert (slab[m < 0] == -7.0).all(), (rank, chunk)
            p = ptgpu.make_params(W, H, n, nsub, SEED, 3, rank, 2, flags=EXACT)
            prog = _progressive(ctx, p, [(0, 1), (1, n)])
            assert _same(prog[m >= 0], ref[m[m >= 0]]) and (prog[m < 0] == -7.0).all(), rank
    assert total == {0: rsegs, n: rsegs}


# ---- (b) every unit-level kind away from nsub 2 ---------------------------------
# The plan of each frame at 8,192 wave slots (256 CUs) is a row of
# tests/golden/launch_plans.json; here: scene, nsub, W, H, samples, shard
# (rank, count), the kind-defining fields (levels, resolve_pass) and the slab
# rows compared with the oracle -- the first slab row, the rows either side of
# the level boundary, the last slab row (slab row j of an unsharded frame is
# image row j).  Every one of these rows is lit in both scenes (synthetic:300's
# sky emits), which the test asserts.
KINDS = {
    # split tail, accumulating; exactly at the 12,288-group threshold
    "lin_nsub8_tail_acc": ("box", 8, 128, 96, 8, None, 2, 1, None),
    # one row below the threshold: a single level, 2 chunks of 4 (no boundary: a middle row instead)
    "lin_nsub8_single": ("box", 8, 128, 95, 8, None, 1, 1, (0, 47, 94)),
    "lin_nsub8_coop": ("box", 8, 256, 160, 8, None, 2, 0, None),  # cooperative tail, 1 pixel per wave
    "lin_nsub5_coop": ("box", 5, 513, 160, 8, None, 2, 0, None),  # cooperative tail, 50 and 25 valid slots
    "lin_nsub5_tail_acc": ("box", 5, 257, 96, 8, None, 2, 1, None),  # accumulating tail, 50 / 25 slots
    "lin_nsub3_tail_acc": ("box", 3, 701, 122, 8, None, 2, 1, None),  # accumulating tail, 63 / 9 slots
    "lin_nsub6_tail_acc": ("box", 6, 127, 97, 9, None, 2, 1, None),  # tail chunks 2, 2, 2, 2, 1; 36 slots
    "lin_nsub7_tail_acc": ("box", 7, 129, 96, 8, None, 2, 1, None),  # 49 slots
    # ... and as rank 1 of two shards of 129x191: the last slab row is outside the image
    "lin_nsub7_tail_acc_shard": ("box", 7, 129, 191, 8, (1, 2), 2, 1, None),
    "lin_nsub1_tail_acc": ("box", 1, 1000, 768, 8, None, 2, 1, None),  # the last group of a row: 40 of 64 pixels
    "bvh_nsub3_tail_acc": ("synthetic:300", 3, 700, 246, 8, None, 2, 1, None),  # a tail that cannot pixel-split (7 < 8)
    "bvh_nsub3_psplit5": ("synthetic:300", 3, 700, 246, 9, None, 2, 0, None),  # pixel split, 5 parts of 7 pixels
    "bvh_nsub3_psplit7": ("synthetic:300", 3, 700, 246, 13, None, 2, 0, None),  # pixel split, 7 of 7
    "bvh_nsub1_psplit8": ("synthetic:300", 1, 1000, 1536, 8, None, 2, 0, None),  # 8 of 64, ragged last group
    "bvh_nsub8_tail_acc": ("synthetic:300", 8, 192, 128, 8, None, 2, 1, None),  # accumulating tail, 1 pixel per wave
    "bvh_nsub8_head_tail": ("synthetic:300", 8, 96, 64, 16, None, 2, 1, None),  # plan_bvh_head_tail
}
FAST_TOO = ("lin_nsub8_coop", "bvh_nsub3_psplit5")


@functools.lru_cache(maxsize=None)
def _recorded_plans():
    with open(os.path.join(GOLDEN, "launch_plans.json")) as f:
        return {p["name"]: p for p in json.load(f)["plans"]}


def _plan_of(case):
    name, nsub, W, H, n, shard, _, _, _ = KINDS[case]
    key = f"n{300 if name.startswith('synthetic') else 9} {W}x{H}x{n} nsub{nsub}"
    if shard:
        key += f" shard {shard[0] + 1}/{shard[1]}"
    return _recorded_plans()[key]


@pytest.mark.parametrize("case", list(KINDS))
def test_unit_level_kinds_are_exact(case):
    _require_gpu()
    name, nsub, W, H, n, shard, levels, resolve_pass, rows = KINDS[case]
    rank, count = shard or (0, 1)
    plan = _plan_of(case)
    assert (plan["n_levels"], plan["needs_resolve"]) == (levels, resolve_pass)
    bvh = name.startswith("synthetic")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    scn, cam, sp, ca = _scene(name, W, H)

    def params(chunk=0, flags=EXACT):
        return ptgpu.make_params(W, H, n, nsub, SEED, 1, rank, count, chunk, flags=flags)

    with ptgpu.Context(scn, cam) as ctx:
        info = ctx.launch_info(params())
        print(f"{case}: {cus} CUs, {info}")
        assert (info["bvh"], info["levels"], info["resolve_pass"]) == (int(bvh), levels, resolve_pass), \
            f"{case}: the plan on a device of {cus} CUs is not of the kind under test: {info}"
        if cus == 256:
            assert (info["units"], info["workgroups"]) == (plan["n_units"], plan["grid"])
        auto, _ = _slab(ctx, params())
        chunked, _ = _slab(ctx, params(chunk=3))
        prog = _progressive(ctx, params(), [(0, 3), (3, n)])
        if case in FAST_TOO:
            fast, _ = _slab(ctx, params(flags=0))
            fast_chunked, _ = _slab(ctx, params(chunk=3, flags=0))
    assert _same(auto, chunked)
    assert _same(auto, prog)
    if case in FAST_TOO:
        assert fast.min() >= 0.0 and fast.mean() > 0.0 and _same(fast, fast_chunked)
    m = ptgpu.slab_to_image_rows(H, 1, rank, count)
    assert (auto[m < 0] == -7.0).all() and (prog[m < 0] == -7.0).all()
    last = int(np.nonzero(m >= 0)[0][-1])
    if shard:
        assert last == len(m) - 2  # the last slab row lies outside the image
    if rows is None:
        b = plan["lvl_group"][1] // plan["waves_per_row"]  # the tail's first slab row
        assert 0 < b - 1 and b < last
        rows = (0, b - 1, b, last)
    for j in rows:
        y = H - 1 - int(m[j])
        ref, _ = po.render_xs_rect(sp, ca, W, H, n, nsub, SEED, rows=(y, y + 1, 1), nthreads=NT)
        d = float(np.abs(auto[j].astype(np.float64) - ref[int(m[j])]).max())
        print(f"{case}: slab row {j} (y {y}): oracle mean {ref[int(m[j])].mean():.5f}, max |diff| {d}")
        assert ref[int(m[j])].mean() > 0, j
        assert d == 0.0, j


# ---- (c) small valid-slot counts at the largest chunk ----------------------------
# W, nsub -> nv = W nsub^2 valid slots: divmod_nv's one correction step over it < nv 2^16
SLOTS = [(1, 1), (2, 3), (1, 5), (1, 6), (1, 7), (2, 5)]


@pytest.mark.parametrize("W,nsub", SLOTS, ids=[f"nv{w * s * s}" for w, s in SLOTS])
def test_few_valid_slots_with_the_largest_chunk(W, nsub):
    """65,537 samples with chunk_samples 2^20 (capped at 2^16): one unit of
    65,536 samples and one of 1 (tests/test_gpu_multi.py has 63 slots)."""
    _require_gpu()
    H, n = 1, 65537
    scn, cam, sp, ca = _scene("box", W, H)
    p = ptgpu.make_params(W, H, n, nsub, SEED, chunk_samples=1 << 20, flags=EXACT)
    with ptgpu.Context(scn, cam) as ctx:
        info = ctx.launch_info(p)
        assert (info["units"], info["levels"], info["resolve_pass"]) == (2, 1, 1)
        gpu, _ = _slab(ctx, p)
    b, _ = po.render_xs_rect(sp, ca, W, H, n, nsub, SEED, nthreads=16)
    assert b.mean() > 0
    assert _same(gpu, b)


# ---- (d) the trace kernel and the fast render kernel at every nsub ------------------
TW, TH, N_TRACE = 160, 120, 800


@pytest.mark.parametrize("name", ["box", "synthetic:300"])
def test_trace_kernel_at_every_subpixel_count(name):
    _require_gpu()
    rng = np.random.default_rng(11)
    nsubs = rng.integers(1, 9, N_TRACE)
    u = rng.random((N_TRACE, 2))
    coords = np.stack([rng.integers(0, TW, N_TRACE), rng.integers(0, TH, N_TRACE), (u[:, 0] * nsubs).astype(np.int64),
                       (u[:, 1] * nsubs).astype(np.int64), rng.integers(0, 1 << 20, N_TRACE)], axis=1).astype(np.int32)
    assert (coords[:, 2] < nsubs).all() and (coords[:, 3] < nsubs).all()
    assert sorted(set(nsubs.tolist())) == list(range(1, 9))
    scn, cam, sp, ca = _scene(name, TW, TH)
    lit = 0
    with ptgpu.Context(scn, cam) as ctx:
        for nsub in range(1, 9):
            sel = coords[nsubs == nsub]
            out, segs = ctx.trace_samples(torch.from_numpy(sel).cuda(), ptgpu.make_params(TW, TH, 1, nsub, SEED, flags=EXACT))
            torch.cuda.synchronize()
            out, segs = out.cpu().numpy(), segs.cpu().numpy()
            for i, (x, y, sx, sy, s) in enumerate(sel.tolist()):
                ref, rs = po.sample_f32(sp, ca, TW, TH, nsub, SEED, x, y, sx, sy, s)
                assert segs[i] == rs, (nsub, sel[i])
                assert out[i].tobytes() == ref.tobytes(), (nsub, sel[i], out[i], ref)
                lit += bool(ref.max() > 0)
    assert lit > N_TRACE // 50


# scene, W, H, samples, nsub, passes: ragged widths, at most 12,288 paths each
FAST_FRAMES = {
    "box_nsub1": ("box", 70, 6, 8, 1, [(0, 3), (3, 8)]),
    "box_nsub4": ("box", 11, 6, 4, 4, [(0, 4)]),
    "box_nsub5": ("box", 7, 6, 4, 5, [(0, 1), (1, 4)]),
    "box_nsub6": ("box", 5, 6, 4, 6, [(0, 4)]),
    "box_nsub7": ("box", 5, 6, 4, 7, [(0, 2), (2, 4)]),
    "box_nsub8": ("box", 5, 6, 4, 8, [(0, 4)]),
    "bvh_nsub5": ("synthetic:300", 7, 6, 4, 5, [(0, 3), (3, 4)]),
    "bvh_nsub8": ("synthetic:300", 5, 6, 4, 8, [(0, 1), (1, 4)]),
}


@pytest.mark.parametrize("case", list(FAST_FRAMES))
def test_fast_render_kernel_equals_fast_trace_kernel_at_every_subpixel_count(case):
    _require_gpu()
    name, W, H, n, nsub, passes = FAST_FRAMES[case]
    assert W * H * nsub * nsub * n <= 12288 and _ragged(W, nsub)
    check_render_equals_trace(name, W, H, n, nsub, passes)


# ---- (e) the other kernels that index by nsub ---------------------------------------
def test_noise_kernel_at_five_subpixels():
    """W = 5 at nsub 5: pixel groups of 2, 2 and 1 pixels, 25 sums per pixel."""
    _require_gpu()
    W, H, n, nsub = 5, 4, 8, 5
    check_slabs("box_nsub5", "box", W, H, n, nsub, ptgpu.make_params(W, H, n, nsub, SEED, 1, flags=EXACT | MOM))


@pytest.mark.parametrize("nsub", [1, 3, 5, 8])
def test_reference_f64_at_other_subpixel_counts(nsub):
    _require_gpu()
    check_matches_mode_a_xs("box", 37, 23, 4, nsub)
