"""The premises of tests/tie_scenes.py, on the oracle alone.  No GPU.

include/ptgpu.h gives an exact tie of two roots to the sphere visited first
(linear scenes) or to the lowest scene index (BVH scenes).  The GPU tests
(tests/test_gpu_ties.py) hold every kernel to the oracle on scenes with such
ties; here the scenes are shown to be worth it:

1. Power: exchanging the scene indices inside every group of equal geometry
   changes Mode B's frame (48x32, 4 samples, nsub 2) on at least 25 % of the
   pixels -- a kernel with the rule wrong fails loudly.  Measured: twins_lin
   and _low 57.7 %, twins_room and _low 86.0 %, twin_wall 98.6 %, twins_bvh
   and _low 59.4 %, twins_bvh250 36.3 %, stack9_a/b/c 39.2 / 38.7 / 39.1 %,
   twin_floor 78.2 %, the lamp cases (32x24) 41.0 %.
2. The lamp cases: Mode A/xs with the light list differs between the two
   orders by a per-pixel RMSE of at least 1e-2 (ten times the bar of the GPU's
   fp32 test against it); and the light-sampled frame is unbiased against the
   plain one by tests/test_oracle_light_sampling.py's check.
3. Exact ties are exact in double and in fp32: RMSE(Mode B, Mode A/xs) of a
   case is at most 1.2 times that of its twin-free scene + 1e-5
   (tests/test_wall_rules.py's form).  The twin-free scene is
   tie_scenes.winners_only: the case without the spheres the rule never shows.
   (Against the scene before twinning the `_low` cases would compare two
   different pictures, whose RMSE a handful of chaotic fp32 paths decides:
   room(16) 2.0e-4 with 3 such pixels, twins_room_low 5.1e-4 with 4.)  A twin
   whose radius had passed through float32 is another sphere to Mode A/xs:
   RMSE 0.082 on twins_lin.  Measured: the two sides are equal to every
   printed digit.
4. Order independence (BVH cases): a seeded permutation of the sphere list
   that keeps the order inside every group leaves Mode B's frame bit-identical;
   the same permutation with every group reversed does not.
5. Scan layout: the library's host preparation equals the oracle's, the cases
   are linear or BVH as named, walls pair as expected, and in a linear case the
   members of a group are of one kind, so "visited first" is "lowest index".
6. The first-hit restatement (tests/denoise_ref.py) in float32 against float64
   on the cases tests/test_gpu_denoise.py takes, by that test's bars.
7. The yardstick y of tests/test_gpu_fast_paths.py for the cases added there.
"""
import functools

import numpy as np
import pytest

import denoise_ref
import light_zoo as zoo
import ptgpu
import pyoracle as po
import test_oracle_light_sampling as oracle_ls
import tie_scenes as ts
from test_gpu_statistical import two_sample_check

SEED = 0x5EED0001
W, H, SAMPS, NSUB = 48, 32, 4, 2


def _frame(name):
    return (zoo.W, zoo.H) if name in ts.LAMPS else (W, H)


def _mode_b(scn, cam, w, h):
    return po.render_xs_f32(*ts.oracle_arrays(scn, cam), w, h, SAMPS, NSUB, SEED)[0]


def _mode_a(scn, cam, w, h):
    return po.render_xs_f64(*ts.oracle_arrays(scn, cam), w, h, SAMPS, NSUB, SEED)[0]


@functools.lru_cache(maxsize=None)
def _case_b(name):
    img = _mode_b(*ts.make(name, *_frame(name)), *_frame(name))
    img.setflags(write=False)
    return img


def _changed(a, b):
    return float((np.abs(a.astype(np.float64) - b).max(axis=2) > 0).mean())


def _rmse(a, b):
    return float(np.sqrt(((a.astype(np.float64) - b) ** 2).mean()))


# ---- the cases are what their names say ------------------------------------------
@pytest.mark.parametrize("name", list(ts.CASES))
def test_counts_and_groups(name):
    scn, cam = ts.make(name, *_frame(name))
    assert len(scn.spheres) == ts.COUNTS[name]
    assert (len(scn.spheres) > 64) == (name in ts.BVH)
    gs = ts.groups(scn)
    if name in ts.NEAR:
        assert gs == []  # no ties (test_near_twins_are_ulps_apart_in_float32)
    else:
        assert (len(gs), {len(g) for g in gs}) == (ts.GROUPS[name][0], {ts.GROUPS[name][1]})
        for g in gs:  # equal in double, hence in float32, and different to look at
            looks = {(s.emission, s.color, s.reflection) for s in (scn.spheres[i] for i in g)}
            assert len(looks) == len(g)


@pytest.mark.parametrize("name,ulps", [("near_up1", 1), ("near_down1", -1), ("near_up8", 8), ("near_down8", -8),
                                       ("near_lin_up1", 1)])
def test_near_twins_are_ulps_apart_in_float32(name, ulps):
    scn, _ = ts.make(name, W, H)
    n = len(scn.spheres)
    base = {"near_lin_up1": 40}.get(name, 60)
    twins = scn.spheres[base:]
    assert len(twins) == n - base == base // 2
    for k, t in enumerate(twins):
        o = scn.spheres[1 + 2 * k]
        assert t.position == o.position
        assert int(np.float32(t.radius).view(np.int32)) - int(np.float32(o.radius).view(np.int32)) == ulps


# ---- 1 ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ts.EXACT_TIES)
def test_swapping_the_indices_changes_the_frame(name):
    w, h = _frame(name)
    share = _changed(_case_b(name), _mode_b(*ts.swapped(name, w, h), w, h))
    print(f"{name}: swapping the indices inside the groups changes {100 * share:.1f} % of the pixels")
    assert share >= 0.25


# ---- 2 ----------------------------------------------------------------------------
def _lamp_arrays(name):
    scn, cam = ts.make(name, zoo.W, zoo.H)
    return ts.oracle_arrays(scn, cam) + (tuple(zoo.lights(scn)),)


def test_lamp_order_decides_the_light_sampled_frame():
    frames = {}
    for name in ts.LAMPS:
        sp, ca, ls = _lamp_arrays(name)
        assert list(ls) == {"lamp_dark_first": [5, 6, 7], "lamp_first": [2, 3, 4]}[name]
        frames[name], _ = po.render_xs_f64_ls(sp, ca, zoo.W, zoo.H, 64, ls, zoo.NSUB, SEED, nthreads=oracle_ls.NT)
    rmse = _rmse(frames["lamp_dark_first"], frames["lamp_first"])
    print(f"lamp cases: Mode A/xs with the light list, RMSE between the two orders {rmse:.3f}")
    assert rmse >= 1e-2


@pytest.mark.parametrize("name", ts.LAMPS)
def test_lamp_light_list_is_unbiased_against_the_plain_oracle(name):
    """tests/test_oracle_light_sampling.py's test 3 at `three`'s sample count:
    a listed light behind a dark twin of lower index is occluded by it in both
    estimators (lamp_dark_first: the plain frame never sees the lights, the
    shadow rays never reach them)."""
    sp, ca, ls = _lamp_arrays(name)
    n = zoo.SAMPLES["three"]

    def stats(lights, runs):
        g = np.stack([po.render_xs_f64_ls(sp, ca, zoo.W, zoo.H, n, lights, zoo.NSUB, oracle_ls.run_seed(r),
                                          nthreads=oracle_ls.NT, raw=True)[0] for r in runs])
        return g.mean(0), g.var(0, ddof=1)

    (ml, vl), (mp, vp) = stats(ls, oracle_ls.LISTED), stats((), oracle_ls.PLAIN_A)
    res = two_sample_check(ml, vl, mp, vp, oracle_ls.RUNS)
    print(f"{name}: image mean with the light list {ml.mean():.4f}, plain {mp.mean():.4f}; {res}")


# ---- 3 ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ts.EXACT_TIES)
def test_exact_ties_are_exact_in_both_arithmetics(name):
    w, h = _frame(name)
    scn, cam = ts.make(name, w, h)
    base, bcam = ts.winners_only(name, w, h)
    assert ts.groups(base) == [] and len(base.spheres) == ts.COUNTS[name] - ts.GROUPS[name][0] * (ts.GROUPS[name][1] - 1)
    r = _rmse(_case_b(name), _mode_a(scn, cam, w, h))
    rb = _rmse(_mode_b(base, bcam, w, h), _mode_a(base, bcam, w, h))
    print(f"{name}: RMSE(Mode B, Mode A/xs) {r:.3e}, twin-free {rb:.3e}")
    assert r <= 1.2 * rb + 1e-5


def test_a_twin_through_float32_is_no_twin():
    """The slip the module's docstring warns of, as a check that test 3 can fail."""
    scn, cam = ts.make("twins_lin", W, H)
    for i in range(40, 60):
        s = scn.spheres[i]
        scn.spheres[i] = ptgpu.sphere(float(np.float32(s.radius)), s.position, s.emission, s.color, s.reflection)
    r = _rmse(_mode_b(scn, cam, W, H), _mode_a(scn, cam, W, H))
    base, bcam = ts.winners_only("twins_lin", W, H)
    rb = _rmse(_mode_b(base, bcam, W, H), _mode_a(base, bcam, W, H))
    print(f"twins_lin with float32 radii on the twins: RMSE(Mode B, Mode A/xs) {r:.3e} (exact twins {rb:.3e})")
    assert r > 10 * (1.2 * rb + 1e-5)


# ---- 4 ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ts.BVH_TIES)
def test_mode_b_does_not_depend_on_the_order_outside_the_groups(name):
    kept = _mode_b(*ts.permuted(name, W, H, True), W, H)
    rev = _mode_b(*ts.permuted(name, W, H, False), W, H)
    a, b = int(_changed(_case_b(name), kept) * W * H + 0.5), int(_changed(_case_b(name), rev) * W * H + 0.5)
    print(f"{name}: pixels that change under the order-keeping permutation {a}, with the groups reversed {b} of {W * H}")
    assert np.array_equal(kept, _case_b(name))
    assert b >= 0.25 * W * H
    scn, _ = ts.permuted(name, W, H, True)
    first = ts.make(name, W, H)[0].spheres
    assert [id(s) for s in scn.spheres] != [id(s) for s in first] and len(ts.groups(scn)) == ts.GROUPS[name][0]


# ---- 5 ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ts.CASES))
def test_scan_layout(name):
    w, h = _frame(name)
    scn, cam = ts.make(name, w, h)
    sp, ca = ts.oracle_arrays(scn, cam)
    axis, order = po.scan_layout(sp, ca)
    assert ptgpu.scene_layout(scn, cam) == (axis, order)
    n = len(scn.spheres)
    if name.startswith("twins_room"):  # the room's walls keep their pairs (box mode: every wall paired or alone)
        assert axis == [3, 3, 2, 4, 4] + [-1] * 24
    elif name == "twin_wall":
        # two walls on one side of z: neither a pair nor the only wall of the axis, so no box mode; x and y pair
        assert axis == [3, 3, 2, 4, 4, -1, -1, -1, -1, 2]
        assert order == [1, 0, 3, 4, 2, 9, 5, 6, 7, 8]  # (a pair: its + wall first)
    elif name == "twin_floor":
        assert axis == [1] + [-1] * 69 + [1]  # both floors anchored on y: the huge spheres' loop holds the tie
    elif name in ts.LAMPS:
        assert axis == [1] + [-1] * 7
    elif name.startswith("stack9"):
        assert axis == [1] + [-1] * 78
        assert [i for i, s in enumerate(scn.spheres) if s.radius == ts.STACK[0]] == [2 + 7 * j for j in range(9)]
    else:
        assert axis == [1] + [-1] * (n - 1)
    if name in ts.LINEAR:
        assert sorted(order) == list(range(n))
        for g in ts.groups(scn):
            assert len({axis[i] for i in g}) == 1  # one kind ...
            at = [order.index(i) for i in g]
            assert at == sorted(at)  # ... so index order is visiting order


# ---- 6 ----------------------------------------------------------------------------
FEATURE_CASES = ["twins_lin_low", "twins_bvh_low", "stack9_b"]


@pytest.mark.parametrize("nsub", [1, 2])
@pytest.mark.parametrize("name", FEATURE_CASES)
def test_first_hit_reference_stays_inside_its_cap(name, nsub):
    """tests/test_denoise_host.py's check on the tie cases: the restatement's
    strict < in index order gives the tie to the lowest index in both dtypes.
    (room(16) with twins does not meet it: its small spheres overlap, the hit
    agrees on 99.25 % of the pixels at nsub 2; it is no features case.)"""
    fw, fh = 64, 48
    scn, cam = ts.make(name, fw, fh)
    f64, i64 = denoise_ref.first_hit(scn, cam, fw, fh, nsub, np.float64)
    f32, i32 = denoise_ref.first_hit(scn, cam, fw, fh, nsub, np.float32)
    d = denoise_ref.feature_differences(f32, f64)
    same_hit = f32[..., 7] == f64[..., 7]
    alb = float(np.abs(f32[..., 8:11] - f64[..., 8:11])[same_hit].max())
    share = float(d["agree"].sum() / (f64[..., 7] > 0).sum())
    print(f"{name} nsub {nsub}: hit differs {d['hit_differs']:.4f}, albedo {alb:.1e}, agree {share:.4f}, rays "
          f"differing {int((i64 != i32).sum())}")
    assert d["hit_differs"] <= 0.005
    assert alb <= 1e-6
    assert share >= 0.995
    # the tie is in view: some ray's winner is a group's first member, none another member
    first = {g[0] for g in ts.groups(scn)}
    later = {i for g in ts.groups(scn) for i in g[1:]}
    assert first & set(i64.reshape(-1).tolist()) and not later & set(i64.reshape(-1).tolist())


# ---- 7 ----------------------------------------------------------------------------
FAST_PATH_CASES = ["twins_lin_low", "twins_room_low", "twins_bvh_low", "stack9_a"]


@pytest.mark.parametrize("name", FAST_PATH_CASES)
def test_fast_paths_yardstick(name):
    fp = pytest.importorskip("test_gpu_fast_paths")
    assert name in fp.SCENES_B
    y, ref, _ = fp._oracle_yardstick(name)
    print(f"{name}: fast-paths yardstick y = {y} of {fp.N_PATHS} paths (bound 3 y + {fp.S_SLACK})")
    assert np.isfinite(ref).all() and ref.max() > 0
