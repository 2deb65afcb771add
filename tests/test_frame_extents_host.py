"""The premises of tests/test_gpu_frame_extents.py (no GPU): every frame of
tests/extent_cases.py crosses the threshold its table names, with the
thresholds read from the kernels' source; the sharded frame's slab rows past
the image are where the GPU tests expect them; the hand-made over bytes'
bound on rho; and the ragged pattern fills every row tile and wave unevenly."""
import os
import re

import numpy as np
import pytest

import ptgpu
import extent_cases as ec
from conftest import PKG
from test_gpu_noise import FLOOR, _noise_ref
from test_multi_adaptive_host import units_of

CSRC = os.path.join(PKG, "csrc")


def _text(name):
    with open(os.path.join(CSRC, name), encoding="utf-8") as f:
        return f.read()


def _kernel(text, name):
    """(launch bound, body) of the __global__ kernel `name`."""
    m = re.search(rf"__global__ __launch_bounds__\((\d+)\) void {name}\(", text)
    assert m, f"{name}: not found with a launch bound"
    end = text.find("__global__", m.end())
    return int(m.group(1)), text[m.end():end if end > 0 else len(text)]


def _one(pattern, text, what):
    found = re.findall(pattern, text)
    assert len(found) == 1, f"{what}: {pattern!r} found {len(found)} times"
    return int(found[0])


def _source_steps():
    """extent_cases.STEP, from the source."""
    acc, host = _text("accum_kernels.hpp"), _text("ptg_render.hip")
    noise_blocks = _one(r"constexpr int kNoiseBlocks = (\d+);", acc, "kNoiseBlocks")
    steps = {}
    for name, loop in (("list_rows_kernel", r"for \(int x0 = 0; x0 < A\.W; x0 \+= (\d+)\)"),
                       ("list_rows_gathered_kernel", r"for \(int x0 = 0; x0 < A\.W; x0 \+= (\d+)\)"),
                       ("list_units_kernel", r"for \(int r0 = 0; r0 < slab_rows; r0 \+= (\d+)\)"),
                       ("list_fill_kernel", r"for \(int k = threadIdx\.x; k \* ppw < cnt; k \+= (\d+)\)")):
        bound, body = _kernel(acc, name)
        steps[name] = _one(loop, body, name)
        assert steps[name] == bound, name  # a tile is one item per thread of the workgroup
        launch = {"list_units_kernel": rf"{name}<<<1, (\d+), 0, s>>>"}.get(name, rf"{name}<<<A\.slab_rows, (\d+), 0, s>>>")
        for threads in re.findall(launch, host) or [None]:
            assert threads is not None and int(threads) == bound, f"{name}: launch"
    # list_units_kernel's scan: 64 rows a wave, the waves' sums through LDS
    _, body = _kernel(acc, "list_units_kernel")
    wave = _one(r"__shfl_up\(incl, off, (\d+)\)", body, "list_units_kernel's scan")
    assert _one(r"if \(lane == (\d+)\)\s+wave_sum\[wv\] = incl;", body, "wave_sum") == wave - 1
    assert re.search(rf"threadIdx\.x & {wave - 1}, wv = threadIdx\.x >> {wave.bit_length() - 1};", body)
    steps["list_units_kernel:wave"] = wave
    # the grid-stride kernels: strided_blocks(items, per_block) blocks, at most kNoiseBlocks
    default = _one(r"unsigned strided_blocks\(long long items, int per_block = (\d+)\)", host, "strided_blocks")
    assert re.search(r"return \(unsigned\)\(blocks < kNoiseBlocks \? blocks : kNoiseBlocks\);", host)
    for name in ("noise_kernel", "select_over_kernel", "noise_active_kernel"):
        bound, body = _kernel(acc, name)
        per_thread = _one(r"const long long stride = \(long long\)gridDim\.x \* (\d+);", body, name)
        assert _one(r"i = \(long long\)blockIdx\.x \* (\d+) \+ threadIdx\.x; i < total; i \+= stride", body, name) == bound
        launches = re.findall(rf"{name}<<<strided_blocks\(pixels\), (\d+), 0, s>>>", host)
        assert launches and all(int(t) == bound for t in launches), name
        assert per_thread == bound == default, name
        steps[name] = noise_blocks * bound
    bound, body = _kernel(acc, "bump_counts_kernel")
    per_block = _one(r"bump_counts_kernel<<<strided_blocks\(bound, /\*per_block=\*/(\d+)\), (?:\d+), 0, s>>>", host,
                     "bump_counts_kernel's launch")
    assert _one(r"bump_counts_kernel<<<strided_blocks\(bound, /\*per_block=\*/\d+\), (\d+), 0, s>>>", host,
                "bump_counts_kernel's block") == bound
    assert _one(r"u = \(long long\)blockIdx\.x \* (\d+) \+ \(threadIdx\.x >> 6\)", body, "bump start") == per_block
    assert _one(r"u \+= \(long long\)gridDim\.x \* (\d+)\)", body, "bump stride") == per_block == bound // 64
    steps["bump_counts_kernel"] = noise_blocks * per_block
    return steps, noise_blocks, per_block


def test_constants_are_where_the_table_says():
    steps, noise_blocks, per_block = _source_steps()
    assert steps == ec.STEP
    assert (noise_blocks, per_block, steps["list_rows_kernel"]) == (ec.NOISE_BLOCKS, ec.BUMP_PER_BLOCK, ec.TILE)


@pytest.mark.parametrize("case,kernel,extent,passes", ec.CROSSINGS,
                         ids=[f"{c}-{k}".replace(" ", "_") for c, k, _, _ in ec.CROSSINGS])
def test_every_frame_crosses_its_threshold(case, kernel, extent, passes):
    """The loop of `kernel` makes `passes` passes over `extent`, by the step read from the source."""
    step = _source_steps()[0][kernel]
    assert -(-extent // step) == passes, (case, kernel, extent, step)


def test_the_table_covers_every_loop_twice_over():
    """Every kernel has a frame with a second pass; the column kernels also one that ends on a tile
    (W = 256 k) and one with a one-column last tile."""
    most = {}
    for _, kernel, extent, passes in ec.CROSSINGS:
        most[kernel] = max(most.get(kernel, 0), passes)
    assert set(most) == set(ec.STEP) and all(p >= 2 for p in most.values()), most
    assert most["list_rows_gathered_kernel"] >= 3 and most["list_units_kernel"] >= 3
    for frames in (ec.COLUMN_FRAMES, ec.GATHERED_FRAMES):
        widths = {W for W, _, _ in frames}
        assert any(W % ec.TILE == 0 for W in widths) and any(W % ec.TILE == 1 and W > ec.TILE for W in widths)
    W, H, nsub = ec.LONG_ROWS
    assert ec.pixels_per_wave(nsub) == 1 and ec.units_per_row(W, nsub) == 300 and H * 300 == 9000
    for nsub in (6, 7, 8):
        assert ec.pixels_per_wave(nsub) == 1
    assert ec.pixels_per_wave(2) == 16 and ec.pixels_per_wave(3) == 7 and ec.pixels_per_wave(1) == 64


def test_grid_frames_put_rows_past_the_image_in_the_second_pass():
    W, H, _ = ec.GRID_U
    first = ec.NOISE_BLOCKS * ec.TILE  # pixels of the first grid pass
    assert W * H - first == W  # the second pass is the last row
    W, H, _ = ec.GRID_S
    br, n = ec.GRID_S_BAND, ec.GRID_S_SHARDS
    assert ptgpu.shard_rows(H, br, n) == 520 == ec.slab_rows(H, br, n)
    assert first == 512 * W and 520 * W == 532480  # the second pass: slab rows 512..519
    m0, m1 = (ptgpu.slab_to_image_rows(H, br, k, n) for k in range(n))
    assert list(range(1024, 1032)) == [(512 // br * n + 0) * br + j for j in range(8)]  # shard 0's rows 512..519
    assert m0[512:].tolist() == [1024, 1025, 1026, -1, -1, -1, -1, -1] and (m0[:512] >= 0).all()
    assert (m1[512:] == -1).all() and (m1[:512] >= 0).all() and m1[511] == 1023
    W, H, _ = ec.ROW_SHARDED
    assert ptgpu.shard_rows(H, 1, 2) == 300
    a, b = ec.grid_count_masks(1024, m0[m0 >= 0])
    assert not a[-1].any() and not a[:, 1000:].any() and a[:-1, :1000].all() and 0 < b.sum() < a.sum()
    assert b[0, 0] and not b[0, 64] and not b[1, 0] and b[1, 64]


def test_two_samples_bound_rho_below_the_hand_made_target():
    """The hand-made over bytes rest on: a pixel with 2 samples has rho <= 0.5 / (nsub floor) = 50 / nsub
    < 1e3.  Worst case: every sub-pixel's variance at the 1/4 cap and a mean of 0 (S1 = 0 cannot come
    with S2 > 0 from real paths; the noise arithmetic does not know that)."""
    for nsub in (1, 2, 3, 6, 8):
        shape = (1, 1, nsub * nsub, 3)
        S1 = np.zeros(shape, dtype=np.uint64)
        S2 = np.full(shape, 2 ** 62, dtype=np.uint64)  # m2 = 2^29: far over the cap
        V, _, rho = _noise_ref(S1, S2, 2, nsub, FLOOR)
        inv32 = float(np.float32(1.0) / np.float32(nsub * nsub))
        assert np.allclose(V, inv32 * inv32 * nsub * nsub * 0.25, rtol=1e-12, atol=0)
        bound = 0.5 / (nsub * FLOOR)
        assert abs(float(rho[0, 0]) - bound) <= 1e-6 * bound and bound == pytest.approx(50.0 / nsub)
        assert float(rho[0, 0]) < 1e3
        # any other sums give less: a larger mean, a smaller variance
        S1b = np.full(shape, 2 ** 32, dtype=np.uint64)
        assert float(_noise_ref(S1b, S2, 2, nsub, FLOOR)[2][0, 0]) < float(rho[0, 0])


@pytest.mark.parametrize("W,H,nsub", ec.ROW_FRAMES + [ec.ROW_SHARDED, ec.LONG_ROWS])
def test_ragged_fills_every_row_tile_and_wave_unevenly(W, H, nsub):
    """Every full tile of 256 rows and every full wave of 64 rows holds empty rows and non-empty rows
    of unequal unit counts; the rows left over at the end hold a non-empty row, so their row_unit0
    depends on the carry and on the waves before them."""
    ppw = ec.pixels_per_wave(nsub)
    m = ec.ragged(W, H)
    assert m.sum(axis=1).tolist() == [(5 * y) % (W + 1) for y in range(H)]
    units = np.array([-(-int(r.sum()) // ppw) for r in m])
    assert units.sum() == units_of(m, ppw)
    for span in (ec.WAVE, ec.TILE):
        for r0 in range(0, H, span):
            u = units[r0:r0 + span]
            if len(u) == span:
                assert (u == 0).any() and len(set(u[u > 0].tolist()) | {0}) >= 2, (span, r0)
                if max(-(-W // ppw), 1) > 1:
                    assert len(set(u.tolist())) >= 3, (span, r0)  # 0 and two unequal counts
            else:
                assert (u > 0).any(), (span, r0)
    if (W, H) == ec.ROW_SHARDED[:2]:  # each shard of 1-row bands takes every second row
        for k in range(2):
            assert (units[k::2] == 0).any() and len(set(units[k::2].tolist())) >= 3


def test_patterns_touch_every_seam():
    for W, H, _ in ec.COLUMN_FRAMES + ec.GATHERED_FRAMES:
        pats = ec.column_patterns(W, H)
        for x in (254, 255, 256, 257, 511, 512, 513, 767, 768, W - 1):
            if x < W:
                assert any(m.sum() == 1 and m[H // 2, x] for m in pats.values()), (W, x)
        assert {"none", "all", "full_row", "every_second", "corners"} <= set(pats)
        assert ("column256" in pats) == (W > 256)
    for W, H, _ in ec.ROW_FRAMES:
        pats = ec.row_patterns(W, H)
        assert set(pats) == {"ragged", "rows", "alternate_rows", "all", "none"}
        assert sorted(np.nonzero(pats["rows"].any(axis=1))[0].tolist()) == \
            sorted({y for y in (63, 64, 255, 256, H - 1) if y < H})
