"""The exact mode at every scene shape of tests/shape_scenes.py, bit for bit
against the oracle's Mode B: linear scenes of 0, 1, 5 .. 64 spheres (box mode
with 0, 1, 2, 3, 4, 5, 16 and 59 small spheres, rooms with walls missing, one
with curved walls and a sphere beyond a wall's tangent plane, five general
anchors and nothing else), the smallest BVH scenes (65, 66, 70)
and a thin lens through both kernels.

Besides the image and the segment count, each case pins how the frame is
launched (ptg_launch_info against scene_prep.hpp's rules: BVH above 64
spheres; box mode when every wall is axis-anchored, clear of the camera and
some axis has a pair) and the test counters, which scene_scan's test_geo
counts before any cull:
    box mode            ntest - nbox == n_small nseg (every small sphere once per
                        segment), nseg <= nbox (at least one wall per segment)
    linear, no pair     ntest == n nseg (every sphere once per segment)
    BVH                 0 < ntest < n nseg
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import ptgpu  # noqa: E402
import pyoracle as po  # noqa: E402
import shape_scenes as ss  # noqa: E402

SEED = 0x5EED0001
EXACT = ptgpu.FLAG_EXACT_MATH
SAMPS, NSUB = 4, 2


def _require_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a visible MI355X")


def _frame(name):
    return (37, 23) if name == "room5" else (48, 32)  # ragged: no multiple of the 16-pixel group


def _is_huge(s, cam):
    """kernel_args.hpp is_huge."""
    d = ptgpu.length(tuple(cam.position[c] - s.position[c] for c in range(3)))
    return s.radius >= 1000.0 or s.radius > 16.0 * (abs(d - s.radius) + 1.0)


@functools.lru_cache(maxsize=None)
def _rendered(name):
    """One exact-mode frame of the case: (image, [nseg, ntest, nbox], launch
    info in exact mode, in fast mode, the oracle's image, its segments)."""
    W, H = _frame(name)
    scn, cam = ss.make(name, W, H)
    p = ptgpu.make_params(W, H, SAMPS, NSUB, SEED, flags=EXACT | ptgpu.FLAG_COUNT_TESTS)
    rows = ptgpu.shard_rows(H, p.band_rows, 1)
    out = torch.full((rows * W * 3,), -7.0, dtype=torch.float32, device="cuda")
    cnt = torch.zeros(3, dtype=torch.int64, device="cuda")
    with ptgpu.Context(scn, cam) as ctx:
        info = ctx.launch_info(p)
        fast = ctx.launch_info(ptgpu.make_params(W, H, SAMPS, NSUB, SEED))
        ctx.render_device(out, p, cnt)
        torch.cuda.synchronize()
    img = out.cpu().numpy().reshape(rows, W, 3)[:H]
    ref, rsegs = po.render_xs_f32(*ss.oracle_arrays(scn, cam), W, H, SAMPS, NSUB, SEED)
    return img, cnt.cpu().tolist(), info, fast, ref, rsegs


@pytest.mark.parametrize("name", list(ss.CASES))
def test_image_and_segments_bitexact(name):
    _require_gpu()
    img, (nseg, _, _), _, _, ref, rsegs = _rendered(name)
    assert img.shape == ref.shape
    diff = np.abs(img.astype(np.float64) - ref.astype(np.float64))
    assert float(diff.max()) == 0.0, (float(diff.max()), int((diff > 0).sum()))
    assert nseg == rsegs
    assert float(ref.mean()) > 0.0


@pytest.mark.parametrize("name", list(ss.CASES))
def test_launch_info(name):
    _require_gpu()
    _, _, info, fast, _, _ = _rendered(name)
    n = len(ss.CASES[name](*_frame(name)).spheres)
    assert info["bvh"] == fast["bvh"] == (1 if n > 64 else 0)
    box = 1 if name in ss.BOX_MODE else 0  # outside0, empty, single, clusters: no axis pair / general anchors
    assert info["box_mode"] == box
    # the fast mode runs box mode only where no ray starts inside a wall
    assert fast["box_mode"] == fast["box_walls_out"] == info["box_walls_out"]
    # every wall here is diffuse and farther from the camera than its radius + the lens: outside_only
    assert fast["box_walls_out"] == box
    pairs = sum(1 << (a - 3) for a in set(ss.LAYOUTS.get(name, [])) if a >= 3)
    if n <= 64 and name in ss.LAYOUTS:
        assert info["wall_pairs"] == pairs


@pytest.mark.parametrize("name", list(ss.CASES))
def test_counter_identities(name):
    _require_gpu()
    W, H = _frame(name)
    _, (nseg, ntest, nbox), info, _, _, _ = _rendered(name)
    scn, cam = ss.make(name, W, H)
    n = len(scn.spheres)
    axis, _ = po.scan_layout(*ss.oracle_arrays(scn, cam))
    print(f"{name}: n {n}, nseg {nseg}, ntest {ntest}, nbox {nbox}")
    assert nseg >= W * H * NSUB * NSUB * SAMPS  # at least one segment per path
    if n > 64:
        assert 0 < ntest < n * nseg
    elif name in ss.BOX_MODE:
        assert info["box_mode"] == 1
        assert ntest - nbox == ss.BOX_MODE[name] * nseg and nseg <= nbox
    else:
        assert not any(a >= 3 for a in axis)  # no pair: every sphere, every segment
        assert ntest == n * nseg
        n_huge = sum(1 for s in scn.spheres if _is_huge(s, cam))
        assert nbox == n_huge * nseg


TRACE = ["room2", "room59", "inside0", "open_0234", "sliver", "cluster64_lens", "cluster65_lens"]


@pytest.mark.parametrize("name", TRACE)
def test_per_path_radiance_bitexact(name):
    """The one-path-per-thread trace kernel at the new shapes: 1,000 random
    paths of a 160x120 frame, radiance bytes and segment counts."""
    _require_gpu()
    W, H, n = 160, 120, 1000
    scn, cam = ss.make(name, W, H)
    rng = np.random.default_rng(7)
    coords = np.stack([rng.integers(0, W, n), rng.integers(0, H, n), rng.integers(0, 2, n),
                       rng.integers(0, 2, n), rng.integers(0, 1 << 20, n)], axis=1).astype(np.int32)
    p = ptgpu.make_params(W, H, 1, 2, SEED, flags=EXACT)
    with ptgpu.Context(scn, cam) as ctx:
        out, segs = ctx.trace_samples(torch.from_numpy(coords).cuda(), p)
        torch.cuda.synchronize()
    out = out.cpu().numpy()
    segs = segs.cpu().numpy()
    sp, ca = ss.oracle_arrays(scn, cam)
    lit = 0
    for i in range(n):
        x, y, sx, sy, s = (int(v) for v in coords[i])
        ref, rs = po.sample_f32(sp, ca, W, H, 2, SEED, x, y, sx, sy, s)
        assert segs[i] == rs, (i, coords[i])
        assert out[i].tobytes() == ref.tobytes(), (i, coords[i], out[i], ref)
        lit += bool(ref.max() > 0)
    assert lit > 0  # (a dark room's lamp is found by few of 1,000 single paths: 8 in open_0234)
