"""The render loop's path start and path end, bit for bit.

The loop state of render_unit -- which lanes hold a path (a wave mask), where a
starting path takes T, E, depth and its slot from -- decides only which
instructions set that state, never a path's arithmetic or the order of its
draws.  So every small frame below must keep its bits:

  exact mode  against the oracle's Mode B (po.render_xs_f32);
  fast mode   against tests/golden/path_start.npz, this project's own output
              recorded with the library of the commit before the lane mask
              (`python tests/test_gpu_path_start.py --record` on an MI355X
              writes the file from whatever library is loaded).

Frames (4 sub-pixels; spp = 4 x samples; a pixel group is 16 pixels = 64 slots;
chunk_samples = samples, so one unit holds every sample of its pixel group):

  box_40x6_4     the last pixel group of a row has 8 pixels: nv = 32, the
                 divmod_nv slot path; total <= 64: no lane ever holds a
                 prefetched ray
  box_32x4_8     total = 128 exactly: the pool is empty right after the first
                 prefetch (refill's `next < total` else-branch)
  box_32x4_36    several refill batches, waiting lanes (wmask), the end of
                 the pool
  simple_48x4_16 sky paths end in shade()'s early return
  syn200_32x4_16 the BVH loop's act / fresh masks

and box_32x4_36 three more ways: through the moments kernel (the raw sums S1,
S2), with PTG_FLAG_LIGHT_SAMPLING (the image), both in both modes against the
recorded fixtures (the oracle has no bit-exact light-sampling mode), and as two
accumulation passes through the HBM accumulator and resolve_kernel, which must
give the one-shot image.
"""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

if __name__ == "__main__":  # --record: the paths tests/conftest.py sets
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for _p in (os.path.join(_root, "cpu-path-tracing_amd"), os.path.join(_root, "oracle"), os.path.dirname(__file__)):
        sys.path.insert(0, _p)

import ptgpu  # noqa: E402
import pyoracle as po  # noqa: E402
import shape_scenes as ss  # noqa: E402

SEED = 0x5EED0001
NSUB = 2
EXACT = ptgpu.FLAG_EXACT_MATH
MOM = ptgpu.FLAG_MOMENTS
LS = ptgpu.FLAG_LIGHT_SAMPLING
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "path_start.npz")

# name -> scene, W, H, samples
FRAMES = {
    "box_40x6_4": ("box", 40, 6, 1),
    "box_32x4_8": ("box", 32, 4, 2),
    "box_32x4_36": ("box", 32, 4, 9),
    "simple_48x4_16": ("simple", 48, 4, 4),
    "syn200_32x4_16": ("synthetic:200", 32, 4, 4),
}
POOL = "box_32x4_36"
MODES = pytest.mark.parametrize("mode", [0, EXACT], ids=["fast", "exact"])


def _require_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a visible MI355X")


def _scene(name, W, H):
    scn = ptgpu.make_scene(name, W, H)
    return scn, ptgpu.camera.with_config(scn.camera_parameters)


def _params(frame, flags):
    _, W, H, n = FRAMES[frame]
    # chunk_samples = n: a unit holds every sample of its pixel group (the auto
    # chunk would cut so small a frame into one-sample units, which never refill)
    return ptgpu.make_params(W, H, n, NSUB, SEED, chunk_samples=n, flags=flags)


def _ctx(frame):
    name, W, H, _ = FRAMES[frame]
    return ptgpu.Context(*_scene(name, W, H))


def _shot(ctx, p):
    out = torch.full((p.height * p.width * 3,), -7.0, dtype=torch.float32, device="cuda")
    ctx.render_device(out, p)
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(p.height, p.width, 3)


def _moments(ctx, p, passes):
    shape = (p.height, p.width, NSUB * NSUB, 3)
    s1 = torch.full((int(np.prod(shape)),), -1, dtype=torch.int64, device="cuda")
    s2 = torch.full_like(s1, -1)
    ctx.reset_accumulation(p)
    for a, b in passes:
        ctx.accumulate(p, a, b)
    ctx.read_moments(p, s1, s2)
    torch.cuda.synchronize()
    return s1.cpu().numpy().view(np.uint64).reshape(shape), s2.cpu().numpy().view(np.uint64).reshape(shape)


def _two_pass(ctx, p):
    n = p.samples
    out = torch.full((p.height * p.width * 3,), -7.0, dtype=torch.float32, device="cuda")
    ctx.reset_accumulation(p)
    ctx.accumulate(p, 0, 4)
    ctx.accumulate(p, 4, n)
    ctx.resolve(out, p, n)
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(p.height, p.width, 3)


def _outputs():
    """Every array the fixtures hold, from the loaded library."""
    out = {}
    for frame in FRAMES:
        with _ctx(frame) as ctx:
            out[f"{frame}/fast"] = _shot(ctx, _params(frame, 0))
    with _ctx(POOL) as ctx:
        for tag, mode in (("fast", 0), ("exact", EXACT)):
            out[f"{POOL}/ls/{tag}"] = _shot(ctx, _params(POOL, mode | LS))
            out[f"{POOL}/s1/{tag}"], out[f"{POOL}/s2/{tag}"] = _moments(ctx, _params(POOL, mode | MOM), [(0, 9)])
    return out


_golden_cache = {}


def _golden(key):
    if not _golden_cache:
        with np.load(GOLDEN) as z:
            _golden_cache.update({k: z[k] for k in z.files})
    return _golden_cache[key]


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("frame", list(FRAMES))
def test_exact_frame_is_the_oracles(frame):
    _require_gpu()
    name, W, H, n = FRAMES[frame]
    with _ctx(frame) as ctx:
        got = _shot(ctx, _params(frame, EXACT))
    sp, ca = ss.oracle_arrays(*_scene(name, W, H))
    ref, _ = po.render_xs_f32(sp, ca, W, H, n, NSUB, SEED)
    assert got.mean() > 0.0
    assert np.array_equal(got.astype(np.float64), ref)


@pytest.mark.parametrize("frame", list(FRAMES))
def test_fast_frame_keeps_its_bits(frame):
    _require_gpu()
    with _ctx(frame) as ctx:
        got = _shot(ctx, _params(frame, 0))
    assert got.mean() > 0.0
    assert _same_bits(got, _golden(f"{frame}/fast"))


@MODES
def test_moments_kernel_keeps_its_sums(mode):
    _require_gpu()
    tag = "exact" if mode else "fast"
    with _ctx(POOL) as ctx:
        s1, s2 = _moments(ctx, _params(POOL, mode | MOM), [(0, 9)])
    assert (s1 > 0).mean() > 0.01
    assert _same_bits(s1, _golden(f"{POOL}/s1/{tag}")) and _same_bits(s2, _golden(f"{POOL}/s2/{tag}"))


@MODES
def test_light_sampling_frame_keeps_its_bits(mode):
    _require_gpu()
    tag = "exact" if mode else "fast"
    with _ctx(POOL) as ctx:
        got = _shot(ctx, _params(POOL, mode | LS))
        plain = _shot(ctx, _params(POOL, mode))
    assert not np.array_equal(got, plain)  # (the flag took effect: shadow segments draw)
    assert _same_bits(got, _golden(f"{POOL}/ls/{tag}"))


@MODES
def test_two_passes_through_hbm_equal_the_one_shot_frame(mode):
    _require_gpu()
    _, W, H, n = FRAMES[POOL]
    with _ctx(POOL) as ctx:
        p = _params(POOL, mode)
        shot = _shot(ctx, p)
        two = _two_pass(ctx, p)
    assert _same_bits(two, shot)
    if mode:
        sp, ca = ss.oracle_arrays(*_scene("box", W, H))
        ref, _ = po.render_xs_f32(sp, ca, W, H, n, NSUB, SEED)
        assert np.array_equal(two.astype(np.float64), ref)
    else:
        assert _same_bits(two, _golden(f"{POOL}/fast"))


if __name__ == "__main__":
    if "--record" not in sys.argv:
        sys.exit("usage: python tests/test_gpu_path_start.py --record")
    arrays = _outputs()
    np.savez_compressed(GOLDEN, **arrays)
    print(f"wrote {GOLDEN}: {sorted(arrays)} from {ptgpu.lib()._name}")
