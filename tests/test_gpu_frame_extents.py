"""The kernels that read the exact accumulators (csrc/accum_kernels.hpp: the
noise estimates, the over bytes, the active-list builders, the count bump and
the per-count resolve) on frames past one tile of 256 columns or rows, one
wave of 64 rows, 256 units a row, 8,192 units and 2048 x 256 slab pixels --
where each kernel's loop, cross-wave step or grid stride runs a second time
(tests/extent_cases.py; tests/test_frame_extents_host.py ties the frames to
the constants in the source).

No reference here is the CPU oracle (too slow at these sizes).  Every kernel
is compared with
  1. numpy applied to what the GPU itself read back (the sums, the counts,
     the rho slab);
  2. the plain kernels the rest of the suite ties to the oracle: accumulate
     under FLAG_MOMENTS for the sums, render_device for pixel values;
  3. hand-made patterns.
Every over / under decision is taken from the GPU's own float32 rho as
(double)rho > rel_error, the kernel's expression, so no pixel is near a
threshold and none is excluded.  rho is within 2^-20 rho + 2^-19 of numpy's
and the variance within _noise_ref's tol (tests/test_gpu_noise.py); everything
else is compared for equality.

Hand-made over bytes on one device (set_active_mask takes no dilate): counts
of 0 and 2 make select_active's over bytes the pattern.  A pixel with fewer
than 2 samples has rho = +inf; one with 2 samples has rho <= 0.5 / (nsub
floor) = 50 / nsub < 1e3 (the 1/4 cap; test_frame_extents_host.py).
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import ptgpu  # noqa: E402
import extent_cases as ec  # noqa: E402
from test_gpu_adaptive import _counts, _image, _resolve_at, _rho_at, _select  # noqa: E402
from test_gpu_noise import EXACT, FLOOR, MOM, SEED, _noise, _noise_ref, _read, _require_gpu, _scene, _stats_of  # noqa: E402
from test_multi_adaptive_host import dilate_clipped, join_rank_major, split_rank_major, units_of  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _drop_the_modules_read_backs():
    """The cached frames hold some hundred MB of sums: freed when the module is done."""
    yield
    for f in (_plain_sums, _grid_frame, _pieces):
        f.cache_clear()


SAMPLES = 8  # params.samples: the bound of accumulate's sample range
HAND_TARGET = 1e3
INF_BITS = 0x7F800000


def _params(W, H, nsub, flags=EXACT, band_rows=1, rank=0, shards=1):
    return ptgpu.make_params(W, H, SAMPLES, nsub, SEED, band_rows, rank, shards, flags=flags)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).copy()).cuda()


def _info():
    return torch.full((2,), -1, dtype=torch.int64, device="cuda")


@functools.lru_cache(maxsize=None)
def _plain_sums(scene, W, H, nsub, n, mode=EXACT, band_rows=1, rank=0, shards=1):
    """S1, S2 of accumulate(p, 0, n) under FLAG_MOMENTS on a context of its own (read-only)."""
    p = _params(W, H, nsub, mode | MOM, band_rows, rank, shards)
    with ptgpu.Context(*_scene(scene, W, H)) as ctx:
        ctx.reset_accumulation(p)
        ctx.accumulate(p, 0, n)
        out = _read(ctx, p)
    for a in out:
        a.setflags(write=False)
    return out


def _check_sums(ctx, p, counts, scene, key, mode=EXACT):
    """Pixel by pixel the context's sums are the plain sums at that pixel's count; zero where the count is 0."""
    g1, g2 = _read(ctx, p)
    for n in np.unique(counts).tolist():
        at = counts == n
        if n == 0:
            assert not g1[at].any() and not g2[at].any(), key
            continue
        S1, S2 = _plain_sums(scene, p.width, p.height, p.num_subpixels, n, mode, p.band_rows, p.shard_rank,
                             p.shard_count)
        assert np.array_equal(g1[at], S1[at]) and np.array_equal(g2[at], S2[at]), (key, n)
    return g1, g2


def _hand_made_select(ctx, p, pattern, d):
    """Counts of 2 off the pattern, then select_active at a target no 2-sample pixel reaches: rho, stats."""
    ctx.reset_accumulation(p)
    ctx.set_active_mask(p, _dev((pattern == 0).astype(np.uint8)))
    ctx.accumulate_active(p, 2)
    return _select(ctx, p, HAND_TARGET, d)


# ---- 1. column tiles: list_rows_kernel ---------------------------------------------------------
@pytest.mark.parametrize("W,H,nsub", ec.COLUMN_FRAMES)
def test_column_tiles_of_hand_made_over_bytes(W, H, nsub):
    """list_rows_kernel past x = 255: the second tile's `base`, wave_cnt rewritten after the barrier, a
    dilate window read across x = 255 / 256.  Through select_active at dilate 0, 1, 2, 8 (over bytes made
    by counts) and through set_active_mask; the counts are 2 (~pattern) + dilate_clipped(pattern, d)."""
    _require_gpu()
    ppw = ec.pixels_per_wave(nsub)
    p = _params(W, H, nsub)
    runs = 0
    patterns = ec.column_patterns(W, H)
    with ptgpu.Context(*_scene("box", W, H)) as ctx:
        for name, pattern in patterns.items():
            on = pattern != 0
            for d in (0, 1, 2, 8):
                key = (name, d)
                rho, st = _hand_made_select(ctx, p, pattern, d)
                ctx.accumulate_active(p, 1)
                counts = _counts(ctx, p)
                active = dilate_clipped(pattern, d)
                assert np.array_equal(np.isinf(rho), on), key  # the over bytes are exactly the pattern
                assert np.array_equal(counts, 2 * (~on).astype(np.int32) + active.astype(np.int32)), key
                assert np.array_equal(st[:4], _stats_of(rho, HAND_TARGET)), key
                assert st[0] == on.sum() and st[3] == W * H, key
                if on.any():
                    assert st[2] == INF_BITS, key
                assert st[4] == active.sum() and st[5] == units_of(active, ppw), key
                _check_sums(ctx, p, counts, "box", key)
                runs += 1
            # d = 0 through the mask entry point
            info = _info()
            ctx.reset_accumulation(p)
            ctx.set_active_mask(p, _dev(pattern), info)
            ctx.accumulate_active(p, 1)
            counts = _counts(ctx, p)
            assert np.array_equal(counts, on.astype(np.int32)), name
            assert info.cpu().tolist() == [int(on.sum()), units_of(on, ppw)], name
            _check_sums(ctx, p, counts, "box", name)
    assert runs == 4 * len(patterns) >= 4 * 7


# ---- 2. row tiles and waves: list_units_kernel ----------------------------------------------
def _two_adds(ctx, p, mask, max_units=None):
    """accumulate_active(2) then (1) under `mask`: info and the counts (max_units None: info[1] read back)."""
    info = _info()
    ctx.reset_accumulation(p)
    ctx.set_active_mask(p, _dev(mask), info)
    got = info.cpu().tolist()
    bound = got[1] if max_units is None else max_units
    ctx.accumulate_active(p, 2, bound)
    ctx.accumulate_active(p, 1, bound)
    return got, _counts(ctx, p)


@pytest.mark.parametrize("W,H,nsub", ec.ROW_FRAMES)
def test_row_tiles_and_waves_through_the_mask(W, H, nsub):
    """list_units_kernel past 64 and 256 rows: wave_sum / before for the rows of waves 1..3, the carry
    across tiles of 256 rows, the cross-wave sum of the pixels.  A wrong row_unit0 moves a row's units
    onto another row's: the counts and the sums show it."""
    _require_gpu()
    ppw = ec.pixels_per_wave(nsub)
    p = _params(W, H, nsub)
    with ptgpu.Context(*_scene("box", W, H)) as ctx:
        for name, mask in ec.row_patterns(W, H).items():
            info, counts = _two_adds(ctx, p, mask, 0)
            assert info == [int(mask.sum()), units_of(mask, ppw)], name
            assert np.array_equal(counts, 3 * mask.astype(np.int32)), name
            _check_sums(ctx, p, counts, "box", name)


def test_row_tiles_of_two_shards():
    """(20, 600) as 2 shards of 1-row bands, 300 slab rows each: dilate 0 through set_active_mask, dilate
    1 through set_active_gathered on hand-made over bytes.  The joined counts are the clipped dilation,
    the shards' pixels and units add up to numpy's."""
    _require_gpu()
    W, H, nsub = ec.ROW_SHARDED
    n, br, ppw = 2, 1, ec.pixels_per_wave(nsub)
    ps = [_params(W, H, nsub, EXACT, br, k, n) for k in range(n)]
    rows = ptgpu.shard_rows(H, br, n)
    assert rows == 300
    with ptgpu.Context(*_scene("box", W, H)) as ctx:  # one context plays both shards in turn
        for name, pattern in ec.row_patterns(W, H).items():
            slabs = split_rank_major(pattern, br, n)
            gathered = _dev(slabs)
            for d in (0, 1):
                want = dilate_clipped(pattern, d)
                got = np.zeros((n, rows, W), np.int32)
                pixels = units = 0
                for k, p in enumerate(ps):
                    if d == 0:
                        info, got[k] = _two_adds(ctx, p, slabs[k])
                        _check_sums(ctx, p, got[k], "box", (name, k))
                    else:
                        stats = torch.zeros(6, dtype=torch.int64, device="cuda")
                        ctx.reset_accumulation(p)
                        ctx.set_active_gathered(p, gathered, d, stats)
                        ctx.accumulate_active(p, 3)
                        got[k] = _counts(ctx, p)
                        st = stats.cpu().tolist()
                        assert st[:4] == [0, 0, 0, 0], (name, k)
                        info = st[4:]
                    mine = split_rank_major(want, br, n)[k]
                    assert info == [int(mine.sum()), units_of(mine, ppw)], (name, d, k)
                    pixels, units = pixels + info[0], units + info[1]
                assert np.array_equal(join_rank_major(got, H, br, n), 3 * want.astype(np.int32)), (name, d)
                assert got.sum() == 3 * want.sum(), (name, d)
                assert (pixels, units) == (int(want.sum()), units_of(want, ppw)), (name, d)


# ---- 3. long rows and many units: list_fill_kernel, bump_counts_kernel ------------------------
@pytest.mark.parametrize("exact_units", [False, True], ids=["max_units_0", "max_units_read_back"])
def test_long_rows_and_many_units(exact_units):
    """(300, 30) at nsub 6, one pixel a wave: a row of 300 units (list_fill_kernel's k += 256) and 9,000
    units in the frame (bump_counts_kernel's grid stride; gather_kernel's unit table of thousands of
    entries, with the launch bound at and above the true count)."""
    _require_gpu()
    W, H, nsub = ec.LONG_ROWS
    ppw = ec.pixels_per_wave(nsub)
    p = _params(W, H, nsub)
    with ptgpu.Context(*_scene("box", W, H)) as ctx:
        for name, mask in ec.long_row_masks(W, H).items():
            info, counts = _two_adds(ctx, p, mask, None if exact_units else 0)
            assert info == [int(mask.sum()), units_of(mask, ppw)], name
            if name == "all":
                assert info[1] == 9000 > ec.STEP["bump_counts_kernel"]
            assert np.array_equal(counts, 3 * mask.astype(np.int32)), name
            _check_sums(ctx, p, counts, "box", name)


# ---- 4. gathered lists at three tiles and at W = 256 k ----------------------------------------
@pytest.mark.parametrize("W,H,nsub", ec.GATHERED_FRAMES)
def test_gathered_list_past_two_tiles(W, H, nsub):
    """tests/test_gpu_multi_adaptive.py's test_gathered_list_of_hand_made_over_bytes on frames of 3 and 4
    column tiles (`left = w[4]` carried twice), of W = 256 k (a seam word whose columns are all >= W) and
    of a one-column last tile, with set bytes at these frames' own seams."""
    _require_gpu()
    ppw = ec.pixels_per_wave(nsub)
    runs = 0
    patterns = ec.column_patterns(W, H)
    wants = {(name, d): dilate_clipped(over, d) for name, over in patterns.items() for d in (0, 1, 8)}
    with ptgpu.Context(*_scene("box", W, H)) as ctx:  # one context plays every shard in turn
        for n in (1, 3):
            for br in (1, 2):
                rows = ptgpu.shard_rows(H, br, n)
                ps = [_params(W, H, nsub, EXACT, br, k, n) for k in range(n)]
                for name, over in patterns.items():
                    gathered = _dev(split_rank_major(over, br, n))
                    assert gathered.numel() == n * rows * W
                    for d in (0, 1, 8):
                        want = wants[name, d]
                        stats = torch.zeros(6, dtype=torch.int64, device="cuda")
                        slabs = torch.full((n, rows * W), -1, dtype=torch.int32, device="cuda")
                        for k, p in enumerate(ps):
                            ctx.reset_accumulation(p)
                            ctx.set_active_gathered(p, gathered, d, stats)
                            ctx.accumulate_active(p, 1)
                            ctx.read_sample_counts(p, slabs[k])
                        torch.cuda.synchronize()
                        g = slabs.cpu().numpy().reshape(n, rows, W)
                        key = (n, br, name, d)
                        assert np.array_equal(join_rank_major(g, H, br, n), want.astype(np.int32)), key
                        assert g.sum() == want.sum(), key  # nothing in the slab rows past the image
                        st = stats.cpu().tolist()
                        assert st[:4] == [0, 0, 0, 0] and st[4:] == [int(want.sum()), units_of(want, ppw)], key
                        runs += 1
    assert runs == 2 * 2 * 3 * len(patterns) >= 2 * 2 * 3 * 7


# ---- 5. the grid-stride trio -----------------------------------------------------------------
GRID = {"U": (ec.GRID_U, 1, 0, 1), "S0": (ec.GRID_S, ec.GRID_S_BAND, 0, ec.GRID_S_SHARDS),
        "S1": (ec.GRID_S, ec.GRID_S_BAND, 1, ec.GRID_S_SHARDS)}


def _median_rel(rho):
    fin = rho[np.isfinite(rho)]
    return float(np.median(fin))


@functools.lru_cache(maxsize=None)
def _grid_frame(case):
    """What the three grid-stride kernels wrote on one slab of more than 2048 x 256 pixels (read-only)."""
    (W, H, nsub), br, rank, shards = GRID[case]
    p = _params(W, H, nsub, EXACT | MOM, br, rank, shards)
    rows = ptgpu.shard_rows(H, br, shards)
    m = ptgpu.slab_to_image_rows(H, br, rank, shards)
    ok = m >= 0
    out = {"ok": ok, "rows": rows, "p": p}
    with ptgpu.Context(*_scene("box", W, H)) as ctx:
        # noise_kernel after a uniform pass of 4 samples
        ctx.reset_accumulation(p)
        ctx.accumulate(p, 0, 4)
        out["S"] = _read(ctx, p)
        _, rho, _ = _noise(ctx, p, 4, 0.0)
        out["noise_rel"] = rel = float(np.median(rho[ok]))
        out["noise"] = _noise(ctx, p, 4, rel)
        # counts of 0, 2 and 4
        first, second = (np.zeros((rows, W), np.uint8) for _ in range(2))
        first[ok], second[ok] = ec.grid_count_masks(W, m[ok])
        ctx.reset_accumulation(p)
        for mask in (first, second):
            ctx.set_active_mask(p, _dev(mask))
            ctx.accumulate_active(p, 2)
        out["want_counts"] = 2 * first.astype(np.int32) + 2 * second.astype(np.int32)
        out["counts"] = _counts(ctx, p)
        out["SA"] = _read(ctx, p)
        # select_over_kernel
        n = rows * W
        rho_t = torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
        over_t = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
        ctx.select_over(p, 0.0, FLOOR, over_t, rho_t)
        torch.cuda.synchronize()
        out["over_rel"] = rel = _median_rel(rho_t.cpu().numpy().reshape(rows, W)[ok])
        rho_t.fill_(-7.0)
        over_t.fill_(9)
        stats = torch.zeros(6, dtype=torch.int64, device="cuda")
        ctx.select_over(p, rel, FLOOR, over_t, rho_t, stats)
        torch.cuda.synchronize()
        out["over"] = (over_t.cpu().numpy().reshape(rows, W), rho_t.cpu().numpy().reshape(rows, W),
                       stats.cpu().numpy().view(np.uint64))
        # noise_active_kernel
        var_t = torch.full((n * 3,), -7.0, dtype=torch.float32, device="cuda")
        rho_t = torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
        ctx.noise_active(p, FLOOR, var_t, rho_t)
        torch.cuda.synchronize()
        out["active"] = (var_t.cpu().numpy().reshape(rows, W, 3), rho_t.cpu().numpy().reshape(rows, W))
    return out


def _within_rho(rho, ref):
    r64 = ref.astype(np.float64)
    return (np.abs(rho.astype(np.float64) - r64) <= 2.0 ** -20 * r64 + 2.0 ** -19).all()


@pytest.mark.parametrize("case", list(GRID))
def test_noise_past_one_grid(case):
    """noise_kernel's grid stride: the pixels of the second pass (U: the last row; S0: image rows
    1024..1026 and 5 rows past the image; S1: rows past the image only) get their own var and rho, count
    once in the stats, and the rows past the image stay untouched."""
    _require_gpu()
    f = _grid_frame(case)
    ok, p = f["ok"], f["p"]
    (W, H, nsub) = GRID[case][0]
    assert f["rows"] * W > ec.STEP["noise_kernel"] and (case == "U") == bool(ok.all())
    S1, S2 = f["S"]
    assert not S1[~ok].any() and not S2[~ok].any()
    V, tol, rho_ref = _noise_ref(S1[ok], S2[ok], 4, nsub)
    var, rho, stats = f["noise"]
    assert (np.abs(var[ok].astype(np.float64) - V) <= tol).all()
    assert _within_rho(rho[ok], rho_ref)
    assert np.array_equal(stats, _stats_of(rho[ok], f["noise_rel"]))
    assert 0 < stats[0] < stats[3] == ok.sum() * W
    assert (var[~ok] == -7.0).all() and (rho[~ok] == -7.0).all()


@pytest.mark.parametrize("case", list(GRID))
def test_select_over_past_one_grid(case):
    _require_gpu()
    f = _grid_frame(case)
    ok = f["ok"]
    (W, H, nsub) = GRID[case][0]
    counts = f["counts"]
    assert np.array_equal(counts, f["want_counts"])
    assert {0, 2, 4} == set(np.unique(counts[ok]).tolist()) and not counts[~ok].any()
    over, rho, stats = f["over"]
    rel = f["over_rel"]
    S1, S2 = f["SA"]
    ref = _rho_at(S1[ok], S2[ok], counts[ok], nsub)
    few = counts[ok] < 2
    assert np.array_equal(np.isinf(rho[ok]), few) and np.isinf(ref[few]).all()
    assert _within_rho(rho[ok][~few], ref[~few])
    assert np.array_equal(over[ok], (rho[ok].astype(np.float64) > rel).astype(np.uint8))  # byte for byte
    assert not over[~ok].any() and (rho[~ok] == -7.0).all()  # 0 in the rows past the image (pre-filled with 9)
    assert np.array_equal(stats[:4], _stats_of(rho[ok], rel)) and not stats[4:].any()
    assert few.sum() < stats[0] < stats[3] == ok.sum() * W and stats[2] == INF_BITS


@pytest.mark.parametrize("case", list(GRID))
def test_noise_active_past_one_grid(case):
    _require_gpu()
    f = _grid_frame(case)
    ok = f["ok"]
    (W, H, nsub) = GRID[case][0]
    counts = f["counts"]
    var, rho = f["active"]
    assert np.array_equal(rho[ok].view(np.uint32), f["over"][1][ok].view(np.uint32))  # select_over's rho, bit for bit
    S1, S2 = f["SA"]
    n = np.maximum(counts[ok], 2)[:, :, None, None].astype(np.float64)
    V, tol, _ = _noise_ref(S1[ok], S2[ok], n, nsub)
    few = counts[ok] < 2
    assert (np.abs(var[ok].astype(np.float64) - V) <= tol)[~few].all()
    inv32 = np.float32(1.0) / np.float32(nsub * nsub)
    cap = np.float32(float(inv32) ** 2 * (nsub * nsub * 0.25))
    assert few.any() and (var[ok][few] == cap).all()
    assert (var[~ok] == -7.0).all() and (rho[~ok] == -7.0).all()


# ---- 6. the adaptive guarantee at four row waves and two column tiles ---------------------------
@functools.lru_cache(maxsize=None)
def _pieces(case, mode):
    """The schedule of ptg_render_adaptive through the device entry points, with what every pass read
    back: per pass (rho, stats, counts before, S1, S2, counts after), then the image (read-only)."""
    scene, W, H, nsub, ends, target, dilate = ec.SCHEDULES[case]
    p = _params(W, H, nsub, mode)
    passes = []
    with ptgpu.Context(*_scene(scene, W, H)) as ctx:
        ctx.reset_accumulation(p)
        ctx.set_active_mask(p)
        ctx.accumulate_active(p, ends[0])
        for k, e in enumerate(ends):
            rho, st = _select(ctx, p, target, dilate)
            before = _counts(ctx, p)
            S1, S2 = _read(ctx, p)
            add = ends[k + 1] - e if k + 1 < len(ends) and st[0] else 0
            ctx.accumulate_active(p, add, int(st[5]))
            passes.append((rho, st, before, S1, S2, _counts(ctx, p), add))
            if not add:
                break
        image = _image(ctx, p)
        sums = _read(ctx, p)
    return passes, image, sums


RUNS = [("X", EXACT), ("X", 0), ("Y", EXACT)]
RUN_IDS = ["X-exact", "X-fast", "Y-exact"]


@pytest.mark.parametrize("case,mode", RUNS, ids=RUN_IDS)
def test_schedule_passes_follow_the_gpus_own_rho(case, mode):
    """Per pass: over = rho > target, active = its clipped dilation, the four counts of the stats from
    those, and the pass adds its samples to exactly the active pixels."""
    _require_gpu()
    scene, W, H, nsub, ends, target, dilate = ec.SCHEDULES[case]
    ppw = ec.pixels_per_wave(nsub)
    passes, _, _ = _pieces(case, mode)
    assert len(passes) == len(ends)
    for k, (rho, st, before, S1, S2, after, add) in enumerate(passes):
        over = rho.astype(np.float64) > target
        active = dilate_clipped(over, dilate)
        near = int(over[:, 248:264].sum()), int(over[248:264].sum())
        print(f"{case} pass {k}: over {int(over.sum())}, active {int(active.sum())}, "
              f"over within 8 of x = 256 / y = 256: {near}")
        assert st[0] == over.sum() and st[3] == W * H and st[4] == active.sum() and st[5] == units_of(active, ppw), k
        assert np.array_equal(st[:4], _stats_of(rho, target)), k
        assert near[0] > 0 and near[1] > 0, k  # over pixels at the column seam and at the row seam
        assert np.array_equal(after, before + add * active.astype(np.int32)), k
        ref = _rho_at(S1, S2, before, nsub)
        assert np.isfinite(ref).all() and _within_rho(rho, ref), k


@pytest.mark.parametrize("case,mode", RUNS, ids=RUN_IDS)
def test_schedule_ends_with_the_plain_kernels_values(case, mode):
    """S1, S2 are the plain moments sums at each pixel's own count, and resolve_active's image is
    render_device's at samples = n_p, pixel for pixel."""
    _require_gpu()
    scene, W, H, nsub, ends, target, dilate = ec.SCHEDULES[case]
    passes, image, (g1, g2) = _pieces(case, mode)
    counts = passes[-1][5]
    share = {n: float((counts == n).mean()) for n in (2, 4, 6, 8)}
    print(f"{case} mode {mode}: final counts " + ", ".join(f"{n}: {100 * s:.2f} %" for n, s in share.items()))
    assert set(np.unique(counts).tolist()) == {2, 4, 6, 8}
    assert min(share.values()) >= 0.003, share
    with ptgpu.Context(*_scene(scene, W, H)) as ctx:
        for n in (2, 4, 6, 8):
            at = counts == n
            S1, S2 = _plain_sums(scene, W, H, nsub, n, mode)
            assert np.array_equal(g1[at], S1[at]) and np.array_equal(g2[at], S2[at]), n
            out = torch.full((H * W * 3,), -7.0, dtype=torch.float32, device="cuda")
            ctx.render_device(out, ptgpu.make_params(W, H, n, nsub, SEED, flags=mode))
            torch.cuda.synchronize()
            assert np.array_equal(image[at], out.cpu().numpy().reshape(H, W, 3)[at]), n
    assert np.array_equal(image, _resolve_at(g1, counts, nsub))


def _totals(passes):
    return ([int(st[0]) for _, st, *_ in passes], [int(st[4]) for _, st, *_ in passes])


def test_driver_and_three_shards_equal_the_pieces():
    """X in the exact mode: ptg_render_adaptive gives the pieces' counts, image and report totals;
    three local shards of 2-row bands give the same counts and image bit for bit."""
    _require_gpu()
    scene, W, H, nsub, ends, target, dilate = ec.SCHEDULES["X"]
    passes, image, _ = _pieces("X", EXACT)
    counts = passes[-1][5]
    img = np.zeros((H * W, 3))
    rep, got = ptgpu.render_adaptive(*_scene(scene, W, H), img, W, H, ends[-1], rel_error=target, floor=FLOOR,
                                     max_fraction=0.0, min_samples=ends[0], dilate=dilate, num_subpixels=nsub,
                                     seed=SEED, flags=EXACT, sample_counts=True)
    assert np.array_equal(got, counts)
    assert np.array_equal(img.reshape(H, W, 3), image.astype(np.float64))
    over, active = _totals(passes)
    assert rep["passes"] == len(passes) and rep["pixels"] == W * H
    assert rep["pass_over"] == over and rep["pass_active"] == active
    assert rep["pass_added"] == [ends[0]] + [ends[k] - ends[k - 1] for k in range(1, len(ends))]
    assert rep["total_samples"] == int(counts.sum(dtype=np.int64)) and rep["max_samples"] == int(counts.max())
    assert rep["pixels_over"] == over[-1] and rep["converged"] == 0
    p = ptgpu.make_params(W, H, ends[-1], nsub, SEED, 2, flags=EXACT)
    with ptgpu.MultiContext(*_scene(scene, W, H), [0], local_shards=3) as m:
        mimg = np.zeros((H * W, 3))
        mrep, mcounts = m.render_adaptive(mimg, p, target, FLOOR, 0.0, ends[0], dilate, sample_counts=True)
    assert np.array_equal(mcounts, counts) and np.array_equal(mimg, img) and mrep == rep
