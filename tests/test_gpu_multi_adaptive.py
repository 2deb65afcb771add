"""Noise-target and adaptive frames on several GPUs (ptg_select_over_device,
ptg_set_active_gathered_device, ptg_multi_noise ... ptg_multi_render_adaptive)
against their guarantee:

    for any shard count, band_rows and dilate in 0..8, in both arithmetic
    modes, the image, the per-pixel sample counts, every report field and the
    kernel counters equal the one-device entry point's bit for bit.

Everything compared is an integer or a float that both sides compute with the
same instructions on the same inputs, so every comparison is for equality.
The gathered active list is checked on hand-made over bytes against the numpy
restatement of tests/test_multi_adaptive_host.py; the drivers against the
one-device drivers, and once against the simulation on the oracle's per-path
values (tests/test_gpu_adaptive.py), so that an error common to both drivers
cannot pass.  One GPU runs the n-shard layout as n local shards
(MultiContext(local_shards=n): the same code, the all-gather done by device
copies) and the RCCL path as a one-rank communicator.
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
from test_gpu_adaptive import CASES, _resolve_at, _simulate, _sums_at  # noqa: E402
from test_gpu_noise import EXACT, FLOOR, SEED, _require_gpu, _scene  # noqa: E402
from test_multi_adaptive_host import dilate_clipped, join_rank_major, split_rank_major, units_of  # noqa: E402

MOM = ptgpu.FLAG_MOMENTS


def _rows(p):
    return ptgpu.shard_rows(p.height, p.band_rows, p.shard_count)


# ---- 1. masks through the gathered list, against numpy ---------------------------------
def _patterns(W, H, br):
    """name -> over bytes [H, W]; identical patterns are run once."""
    z = np.zeros((H, W), np.uint8)
    out = {"none": z, "all": np.ones((H, W), np.uint8)}

    def one(name, y, x):
        if 0 <= y < H and 0 <= x < W:
            m = z.copy()
            m[y, x] = 1
            out[name] = m
    for name, y, x in (("corner00", 0, 0), ("corner0W", 0, W - 1), ("cornerH0", H - 1, 0), ("cornerHW", H - 1, W - 1)):
        one(name, y, x)
    for x in (63, 64, 255, 256, W - 1):
        one(f"x{x}", H // 2, x)
    first = br if br < H else 0  # the second band where there is one
    one("band_first", first, W // 2)
    one("band_last", min(first + br - 1, H - 1), W // 3)
    row = z.copy()
    row[min(1, H - 1)] = 1
    out["full_row"] = row
    col = z.copy()
    col[:, 64 if W > 64 else W // 2] = 7  # any non-zero byte
    out["full_column"] = col
    seen, uniq = set(), {}
    for k, m in out.items():
        if m.tobytes() not in seen:
            seen.add(m.tobytes())
            uniq[k] = m
    return uniq


@pytest.mark.parametrize("W,H,nsub", [(300, 9, 2), (70, 5, 1), (1, 1, 2)])
def test_gathered_list_of_hand_made_over_bytes(W, H, nsub):
    """reset, set_active_gathered, accumulate_active(1), read_sample_counts, un-shard: the counts are the
    clipped dilation of the over bytes; stats[4], [5] summed over the shards are numpy's pixels and units."""
    _require_gpu()
    ppw = 64 // (nsub * nsub)
    runs = 0
    with ptgpu.Context(*_scene("box", W, H)) as ctx:  # one context plays every shard in turn
        for n in (1, 2, 3):
            for br in (1, 2, 7):
                rows = ptgpu.shard_rows(H, br, n)
                ps = [ptgpu.make_params(W, H, 4, nsub, SEED, br, k, n, flags=EXACT) for k in range(n)]
                for name, over in _patterns(W, H, br).items():
                    gathered = torch.from_numpy(split_rank_major(over, br, n).reshape(-1).copy()).cuda()
                    assert gathered.numel() == n * rows * W
                    for d in (0, 1, 2, 8):
                        want = dilate_clipped(over, d)
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
    assert runs >= 3 * 3 * 4 * (2 if W == 1 else 10)  # (1 x 1: only "none" and "all" differ)
    if (W, H) == (300, 9):  # the frame's premises: five bands on three shards, slab rows past the image
        assert ptgpu.shard_rows(9, 2, 3) * 3 > 9 and -(-9 // 2) == 5


# ---- 2. gathered select equals the one-device select ------------------------------------
def _select_one_device(case, dilate):
    name, W, H, nsub, ends, target = CASES[case]
    p = ptgpu.make_params(W, H, ends[-1], nsub, SEED, flags=EXACT)
    with ptgpu.Context(*_scene(name, W, H)) as ctx:
        ctx.reset_accumulation(p)
        ctx.set_active_mask(p)
        ctx.accumulate_active(p, 4)
        stats = torch.zeros(6, dtype=torch.int64, device="cuda")
        ctx.select_active(p, target, FLOOR, dilate, None, stats)
        torch.cuda.synchronize()
        st = stats.cpu().numpy().view(np.uint64)
        ctx.accumulate_active(p, 1, int(st[5]))
        counts = torch.full((H * W,), -1, dtype=torch.int32, device="cuda")
        ctx.read_sample_counts(p, counts)
        torch.cuda.synchronize()
    return counts.cpu().numpy().reshape(H, W), st


@pytest.mark.parametrize("case", ["A", "C"])
def test_gathered_select_equals_the_one_device_select(case):
    _require_gpu()
    name, W, H, nsub, ends, target = CASES[case]
    n = 3
    for dilate in (0, 1, 8):
        want, want_st = _select_one_device(case, dilate)
        assert 0 < want_st[0] < W * H and want_st[0] <= want_st[4]  # some pixels over, not all
        if dilate == 0:
            assert 4 in want and 5 in want
        for br in (1, 4):
            ps = [ptgpu.make_params(W, H, ends[-1], nsub, SEED, br, k, n, flags=EXACT) for k in range(n)]
            rows = _rows(ps[0])
            ctxs = [ptgpu.Context(*_scene(name, W, H)) for _ in range(n)]
            try:
                over = torch.full((n, rows * W), 9, dtype=torch.uint8, device="cuda")
                stats = torch.zeros((n, 6), dtype=torch.int64, device="cuda")
                for k, (c, p) in enumerate(zip(ctxs, ps)):
                    c.reset_accumulation(p)
                    c.set_active_mask(p)
                    c.accumulate_active(p, 4)
                    c.select_over(p, target, FLOOR, over[k], None, stats[k])
                gathered = over.reshape(-1)  # the concatenation: what an all-gather lays out
                slabs = torch.full((n, rows * W), -1, dtype=torch.int32, device="cuda")
                for k, (c, p) in enumerate(zip(ctxs, ps)):
                    c.set_active_gathered(p, gathered, dilate, stats[k])
                    c.accumulate_active(p, 1)
                    c.read_sample_counts(p, slabs[k])
                torch.cuda.synchronize()
            finally:
                for c in ctxs:
                    c.close()
            assert int(over.max()) <= 1
            got = join_rank_major(slabs.cpu().numpy().reshape(n, rows, W), H, br, n)
            assert np.array_equal(got, want), (dilate, br)
            st = stats.cpu().numpy().view(np.uint64)
            total = st.sum(axis=0, dtype=np.uint64)
            total[2] = st[:, 2].max()
            assert np.array_equal(total, want_st), (dilate, br)


# ---- 3. the drivers ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _one_device_adaptive(case, dilate, flags, size=None):
    name, W0, H0, nsub, ends, target = CASES[case]
    W, H = size or (W0, H0)
    img = np.zeros((H * W, 3))
    rep, counts = ptgpu.render_adaptive(*_scene(name, W0, H0), img, W, H, ends[-1], rel_error=target, floor=FLOOR,
                                        max_fraction=0.0, min_samples=ends[0], dilate=dilate, num_subpixels=nsub,
                                        seed=SEED, flags=flags, sample_counts=True)
    img.setflags(write=False)
    counts.setflags(write=False)
    return img, counts, rep


def _multi_adaptive(m, case, dilate, flags, br, size=None, img=None):
    name, W0, H0, nsub, ends, target = CASES[case]
    W, H = size or (W0, H0)
    p = ptgpu.make_params(W, H, ends[-1], nsub, SEED, br, flags=flags)
    img = np.zeros((H * W, 3)) if img is None else img
    rep, counts = m.render_adaptive(img, p, target, FLOOR, 0.0, ends[0], dilate, sample_counts=True)
    return img, counts, rep


COUNT = ptgpu.FLAG_COUNT_TESTS
# case, local shards, band_rows, dilate, flags: every case, every L and every dilate appear
DRIVER_RUNS = [
    ("A", 3, 1, 2, EXACT), ("A", 2, 4, 1, EXACT | COUNT), ("A", 8, 7, 0, EXACT), ("A", 3, 1, 1, 0),
    ("B", 2, 1, 1, EXACT), ("B", 8, 4, 2, EXACT), ("C", 3, 7, 1, EXACT | COUNT), ("C", 8, 1, 0, EXACT),
    ("C", 2, 4, 2, EXACT), ("E", 3, 4, 1, EXACT), ("E", 2, 7, 0, EXACT | COUNT), ("E", 8, 1, 1, EXACT),
]  # (E at dilate 2: the simulation on the oracle makes every pixel of its 14 x 6 frame active in every pass)


@pytest.mark.parametrize("case,L,br,dilate,flags", DRIVER_RUNS)
def test_render_adaptive_equals_the_one_device_driver(case, L, br, dilate, flags):
    _require_gpu()
    name, W, H, nsub, ends, target = CASES[case]
    img, counts, rep = _one_device_adaptive(case, dilate, flags)
    assert rep["passes"] >= 3 and counts.min() < counts.max()  # the comparison proves something
    with ptgpu.MultiContext(*_scene(name, W, H), [0], local_shards=L) as m:
        got_img, got_counts, got_rep = _multi_adaptive(m, case, dilate, flags, br)
    print(f"{case} L {L} band_rows {br} dilate {dilate}: {rep}")
    assert np.array_equal(got_counts, counts)
    assert got_rep == rep
    assert np.array_equal(got_img, img)
    if flags & COUNT:
        assert rep["counters"][0] > 0 and rep["counters"][1] > 0
    else:
        assert rep["counters"] == [0, 0, 0, 0]


def test_second_frame_and_a_frame_of_another_size_reuse_the_context():
    _require_gpu()
    name, W, H, nsub, ends, target = CASES["A"]
    img, counts, rep = _one_device_adaptive("A", 1, EXACT)
    small = (W // 2 + 1, H // 2 + 1)
    simg, scounts, srep = _one_device_adaptive("A", 1, EXACT, small)
    big = (W + 9, H + 5)
    bimg, bcounts, brep = _one_device_adaptive("A", 1, EXACT, big)
    with ptgpu.MultiContext(*_scene(name, W, H), [0], local_shards=3) as m:
        acc = np.zeros((H * W, 3))
        for k in (1, 2):  # the frame ADDS into the image
            _, c, r = _multi_adaptive(m, "A", 1, EXACT, 2, img=acc)
            assert np.array_equal(c, counts) and r == rep and np.array_equal(acc, k * np.asarray(img))
        for size, (wi, wc, wr) in ((small, (simg, scounts, srep)), (big, (bimg, bcounts, brep)),
                                   ((W, H), (img, counts, rep))):
            gi, gc, gr = _multi_adaptive(m, "A", 1, EXACT, 4, size)
            assert np.array_equal(gc, wc) and gr == wr and np.array_equal(gi, wi), size


# The stop fraction, from the oracle, so that at least three passes run as in the adaptive comparison.
# tests/test_gpu_adaptive.py's simulation at dilate 0 leaves over the target after its first three
# checks: A 304, 283, 271 of 768; B 309, 263, 261 of 768; C 74, 66, 65 of 576.  A pixel still over there
# holds the very samples the uniform frame gives it, so the uniform frame has at least as many over:
# more than 0.3 x 768 = 230 (A, B) and more than 0.05 x 576 = 28 (C) after each of the three.
@pytest.mark.parametrize("case,L,br,flags,frac", [("A", 3, 1, EXACT, 0.3), ("C", 2, 4, EXACT, 0.05),
                                                   ("B", 8, 7, 0, 0.3)])
def test_render_to_noise_and_noise_equal_one_device(case, L, br, flags, frac):
    _require_gpu()
    name, W, H, nsub, ends, target = CASES[case]
    scn, cam = _scene(name, W, H)
    img = np.zeros((H * W, 3))
    rep = ptgpu.render_to_noise(scn, cam, img, W, H, ends[-1], target, FLOOR, frac, ends[0], nsub, SEED, flags=flags)
    assert rep["passes"] >= 3 and 0 < rep["pixels_over"] < W * H  # the comparison proves something
    p = ptgpu.make_params(W, H, ends[-1], nsub, SEED, br, flags=flags)
    pm = ptgpu.make_params(W, H, ends[-1], nsub, SEED, br, flags=flags | MOM)
    p1 = ptgpu.make_params(W, H, ends[-1], nsub, SEED, flags=flags | MOM)
    with ptgpu.MultiContext(scn, cam, [0], local_shards=L) as m:
        got = np.zeros((H * W, 3))
        for k in (1, 2):  # the second frame reuses the context and ADDS
            assert m.render_to_noise(got, p, target, FLOOR, frac, ends[0]) == rep
            assert np.array_equal(got, k * img)
        # noise(): the four statistics of the frame against Context.noise after the same passes
        m.reset_accumulation(pm)
        m.accumulate(pm, 0, 3)
        m.accumulate(pm, 3, ends[1])
        st = m.noise(pm, ends[1], target, FLOOR)
    with ptgpu.Context(scn, cam) as ctx:
        ctx.reset_accumulation(p1)
        ctx.accumulate(p1, 0, ends[1])
        want = torch.zeros(4, dtype=torch.int64, device="cuda")
        ctx.noise(p1, ends[1], target, FLOOR, stats=want)
        torch.cuda.synchronize()
    assert np.array_equal(st, want.cpu().numpy().view(np.uint64)) and st[3] == W * H and 0 < st[0] < W * H


# ---- 4. one direct tie to the oracle --------------------------------------------------------
def test_multi_driver_matches_the_simulation_on_the_oracles_paths():
    _require_gpu()
    name, W, H, nsub, ends, target = CASES["A"]
    counts, passes, _ = _simulate("A", 1)
    assert len(np.unique(counts)) > 1
    with ptgpu.MultiContext(*_scene(name, W, H), [0], local_shards=3) as m:
        img, got, rep = _multi_adaptive(m, "A", 1, EXACT, 2)
    assert np.array_equal(got, counts)
    assert list(zip(rep["pass_over"], rep["pass_active"])) == list(passes)
    assert rep["total_samples"] == int(counts.sum(dtype=np.int64)) and rep["max_samples"] == int(counts.max())
    S1, _ = _sums_at("A", counts)
    assert np.array_equal(img.reshape(H, W, 3), _resolve_at(S1, counts, nsub).astype(np.float64))


# ---- 5. the RCCL path ---------------------------------------------------------------------------
def test_one_rank_communicator_runs_the_all_gather():
    _require_gpu()
    name, W, H, nsub, ends, target = CASES["A"]
    img, counts, rep = _one_device_adaptive("A", 1, EXACT)
    with ptgpu.MultiContext(*_scene(name, W, H), [0]) as m:
        assert m.comm_info() == [(1, 0, 0)]  # real communicators: ncclAllGather, not device copies
        got_img, got_counts, got_rep = _multi_adaptive(m, "A", 1, EXACT, 1)
        assert m.comm_info() == [(1, 0, 0)]
    assert np.array_equal(got_counts, counts) and got_rep == rep and np.array_equal(got_img, img)


def test_two_devices():
    _require_gpu()
    if torch.cuda.device_count() < 2:
        pytest.skip(f"needs 2 GPUs, {torch.cuda.device_count()} visible")
    name, W, H, nsub, ends, target = CASES["A"]
    img, counts, rep = _one_device_adaptive("A", 2, EXACT)
    p = ptgpu.make_params(W, H, ends[-1], nsub, SEED, 1, flags=EXACT)
    try:
        # the caller's device is restored: tried with each device current, since a call that left the
        # root's device (0) or its last shard's (1) current would go unnoticed from that device itself
        for cur in (1, 0):
            torch.cuda.set_device(cur)
            with ptgpu.MultiContext(*_scene(name, W, H), [0, 1]) as m:
                assert [r for r, _, _ in m.comm_info()] == [2, 2]
                got_img, got_counts, got_rep = _multi_adaptive(m, "A", 2, EXACT, 1)
                assert torch.cuda.current_device() == cur
                for call in (lambda: m.select_active(p, target, FLOOR, 1), lambda: m.read_sample_counts(p),
                             lambda: m.accumulate_active(p, 1), lambda: m.set_active_mask(p),
                             lambda: m.resolve_active(np.zeros((H, W, 3), np.float32), p)):
                    call()
                    assert torch.cuda.current_device() == cur
            assert torch.cuda.current_device() == cur
    finally:
        torch.cuda.set_device(0)
    assert np.array_equal(got_counts, counts) and got_rep == rep and np.array_equal(got_img, img)


def _cli(tmp_path, tag, *extra):
    cli = os.path.join(os.path.dirname(ptgpu.LIB_PATH), "pt_render_gpu")
    out, spm = tmp_path / f"{tag}.ppm", tmp_path / f"{tag}.pgm"
    r = subprocess.run([cli, "--scene", "box", "--width", "32", "--height", "24", "--format", "p6", "--out", str(out),
                        "--spp", "128", "--noise-target", "0.3", "--noise-fraction", "0", "--min-spp", "16",
                        "--exact-math", "--adaptive", "--dilate", "1", "--spp-map", str(spm), *extra],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    line = re.search(r"^noise: .*$", r.stderr, re.M).group(0)
    return out.read_bytes(), spm.read_bytes(), line


def test_cli_with_one_listed_device_equals_the_plain_run(tmp_path):
    _require_gpu()
    plain = _cli(tmp_path, "plain")
    assert _cli(tmp_path, "listed", "--devices", "0") == plain
    _, counts, rep = _one_device_adaptive("A", 1, EXACT)  # (case A's frame)
    assert plain[1] == b"P5\n32 24\n255\n" + np.asarray(counts).astype(np.uint8).tobytes()


def test_cli_refuses_a_listed_device_that_is_not_there():
    """A usage error (exit status 2) before anything is rendered; the message names the machine's count."""
    _require_gpu()
    cli = os.path.join(os.path.dirname(ptgpu.LIB_PATH), "pt_render_gpu")
    n = torch.cuda.device_count()
    for extra in ([], ["--adaptive"]):
        r = subprocess.run([cli, "--noise-target", "0.1", "--spp", "256", "--devices", f"0,{n}", "--width", "8",
                            "--height", "8", *extra], capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and f"device {n} is not there" in r.stderr, r.stderr
        assert ("one device" if n == 1 else f"{n} devices") in r.stderr


def test_cli_on_two_devices_equals_the_driver(tmp_path):
    _require_gpu()
    if torch.cuda.device_count() < 2:
        pytest.skip(f"needs 2 GPUs, {torch.cuda.device_count()} visible")
    assert _cli(tmp_path, "two", "--devices", "0,1") == _cli(tmp_path, "plain")


# ---- 6. errors and state ---------------------------------------------------------------------------
def test_multi_adaptive_errors_and_state():
    _require_gpu()
    name, W, H, nsub, ends, target = CASES["D"]
    scn, cam = _scene(name, W, H)
    p = ptgpu.make_params(W, H, ends[-1], nsub, SEED, 2, flags=EXACT)
    pm = ptgpu.make_params(W, H, ends[-1], nsub, SEED, 2, flags=EXACT | MOM)
    f32 = np.zeros((H, W, 3), dtype=np.float32)
    torch.cuda.set_device(0)
    with ptgpu.MultiContext(scn, cam, [0], local_shards=3) as m:
        m.reset_accumulation(p)
        with pytest.raises(ptgpu.PtgError, match=r"\(-1\).*no active list"):
            # before any list.  (select_active itself needs no list before it -- it builds one, and on a
            # frame without samples every pixel is over, as tests/test_gpu_adaptive.py shows for a context;
            # what a missing list refuses is the pass that would use it.)
            m.accumulate_active(p, 2)
        for d in (-1, 9):
            with pytest.raises(ptgpu.PtgError, match=r"\(-1\).*dilate"):
                m.select_active(p, target, FLOOR, d)
            with pytest.raises(ptgpu.PtgError, match=r"\(-1\).*dilate"):
                m.render_adaptive(np.zeros((H * W, 3)), p, target, dilate=d)
        with pytest.raises(ptgpu.PtgError, match=r"\(-1\).*floor"):
            m.select_active(p, target, 0.0, 1)
        with pytest.raises(ptgpu.PtgError, match=r"\(-1\).*max_fraction"):
            m.render_to_noise(np.zeros((H * W, 3)), p, target, max_fraction=1.0)
        with pytest.raises(ptgpu.PtgError, match=r"\(-1\).*shard_count must be 1"):
            m.select_active(ptgpu.make_params(W, H, 8, nsub, SEED, 2, 1, 3, flags=EXACT), target, FLOOR, 1)
        with pytest.raises(ptgpu.PtgError, match=r"\(-4\).*fp32"):
            m.set_active_mask(ptgpu.make_params(W, H, 8, nsub, SEED, 2, flags=ptgpu.FLAG_REFERENCE_F64))
        # a region of interest, then the selection: after adaptive passes the uniform entry points refuse ...
        roi = np.zeros((H, W), np.uint8)
        roi[3:9, 5:30] = 1
        m.set_active_mask(p, roi)
        m.accumulate_active(p, 3)
        assert np.array_equal(m.read_sample_counts(p), 3 * roi.astype(np.int32))
        st = m.select_active(p, target, FLOOR, 1)
        # a pixel without samples is over (rho = +inf); the region is 6 x 25, so with dilate 1 only its
        # inner 4 x 23 pixels can stay inactive
        assert st[3] == W * H and W * H - int(roi.sum()) <= st[0] <= W * H
        assert W * H - 4 * 23 <= st[4] <= W * H
        active_before = int(st[4])
        m.accumulate_active(p, 1)
        added = m.read_sample_counts(p) - 3 * roi.astype(np.int32)
        assert set(np.unique(added).tolist()) <= {0, 1} and int(added.sum()) == active_before
        assert (added[roi == 0] == 1).all()
        m.resolve_active(f32, p)
        assert f32.max() > 0
        for call in (lambda: m.accumulate(p, 4, 6), lambda: m.resolve(f32, p, 4), lambda: m.noise(pm, 4, 0.1, FLOOR)):
            with pytest.raises(ptgpu.PtgError, match=r"\(-1\).*adaptive passes since the last reset"):
                call()
        # ... and the adaptive ones after a uniform pass, until a reset
        m.reset_accumulation(pm)
        m.accumulate(pm, 0, 2)
        for call in (lambda: m.set_active_mask(p), lambda: m.select_active(p, target, FLOOR, 1),
                     lambda: m.accumulate_active(p, 1), lambda: m.resolve_active(f32, p),
                     lambda: m.read_sample_counts(p)):
            with pytest.raises(ptgpu.PtgError, match=r"\(-1\).*ptg_accumulate_device pass since the last reset"):
                call()
        m.reset_accumulation(p)
        m.set_active_mask(p)
        m.accumulate_active(p, 2)
        assert (m.read_sample_counts(p) == 2).all()
    assert torch.cuda.current_device() == 0
    # the existing entry point keeps refusing a dilated list on a shard
    with ptgpu.Context(scn, cam) as ctx:
        ps = ptgpu.make_params(W, H, 8, nsub, SEED, 2, 0, 2, flags=EXACT)
        ctx.reset_accumulation(ps)
        with pytest.raises(ptgpu.PtgError, match=r"\(-4\).*dilate"):
            ctx.select_active(ps, target, FLOOR, 1)
