"""PTG_FLAG_STRATIFIED's definition on the CPU: tests/strat_ref.py, the numpy
restatement of the path tracer with the four replaced pairs of draws, in
float64.  No GPU.

1. With the flag off the restatement is tests/light_ref.py's, bit for bit.
2. The null check: the plain restatement against itself, two disjoint sets of
   16 seeds, through test_gpu_statistical.two_sample_check with the project's
   thresholds (frac <= 0.005, |mean z| < 0.08, image mean within 4 se).  It
   fixes SAMPLES: per scene the power of two at which this check passes, found
   as tests/test_oracle_light_sampling.py found its counts.
3. The stratified restatement is unbiased: 16 further seeds with the flag
   against the plain side, through the same check, thresholds unchanged.
4. The variance ratio plain / stratified (per pixel-channel variance of the
   raw mean over the 16 seeds) is printed; `simple` without light sampling
   reproduces the prototype's median of about 2.5, and
   tests/test_gpu_stratified.py holds the GPU to 0.6 of the figure found here.

Frames 32 x 24, nsub 2.  Scenes: `simple` (its emitters met by chance: no
light list), and the zoo's `beside` and `sixteen` with their light lists.

Measured (frac |z| > 4.5, mean z, image mean difference in se; median and
sum variance ratio; `pytest -s` prints each line):

| scene | samples | null | stratified against plain | variance ratio median, sum |
|---|---|---|---|---|
| simple | 64 | 0, -0.042, -1.6 | 0, +0.011, -0.0 | 2.37, 2.54 |
| beside | 64 | 0, +0.025, +2.8 | 0, -0.007, +0.5 | 4.29, 7.56 |
| sixteen | 64 | 0, +0.035, +1.1 | 0, +0.010, +0.6 | 1.79, 1.19 |

64 is the prototype's count.  The null check also passes at 16 and 32 on simple
and sixteen and at 32 on beside (beside at 16: image means 4.3 se apart); the
variance ratio grows with the count, as a (0,2)-sequence's does (simple: 1.66
at 16, 1.95 at 32, 2.37 at 64, 3.17 at 128), so the figure the GPU is held to
is taken at the prototype's 64.
"""
import functools

import numpy as np
import pytest

import light_ref
import light_zoo as zoo
import ptgpu
import strat_ref
from test_gpu_statistical import two_sample_check

SEED = 0x5EED0001
RUNS = 16
W, H, NSUB = zoo.W, zoo.H, zoo.NSUB
SCENES = ("simple", "beside", "sixteen")
# samples per sub-pixel: the prototype's power of two, at which the null check (test 2) passes on all three
SAMPLES = {"simple": 64, "beside": 64, "sixteen": 64}
PLAIN_A, PLAIN_B, FLAGGED = range(0, RUNS), range(RUNS, 2 * RUNS), range(2 * RUNS, 3 * RUNS)


def run_seed(r):
    """The seed of run r, as the GPU tests derive it."""
    return (SEED + 0x9E3779B97F4A7C15 * (r + 1)) & (2 ** 64 - 1)


@functools.lru_cache(maxsize=None)
def scene(name):
    """(scene, camera, light list used with it) -- `simple` runs without light sampling."""
    if name == "simple":
        scn = ptgpu.make_scene("simple", W, H)
        return scn, ptgpu.camera.with_config(scn.camera_parameters), ()
    scn, cam, ls = zoo.make(name)
    return scn, cam, tuple(ls)


@functools.lru_cache(maxsize=None)
def arrays(name):
    scn, cam, ls = scene(name)
    return zoo.oracle_arrays(scn, cam) + (ls,)


def frame_coords(n):
    """Every path of the frame at n samples per sub-pixel, in the order (row, x, sy, sx, sample)."""
    row, x, sy, sx, k = np.meshgrid(np.arange(H), np.arange(W), np.arange(NSUB), np.arange(NSUB), np.arange(n),
                                    indexing="ij")
    return np.stack([x, H - 1 - row, sx, sy, k], axis=-1).reshape(-1, 5).astype(np.int32)


def raw_mean(name, n, seed, stratified):
    """The raw per-pixel-channel mean [H, W, 3] of the frame's n * nsub^2 paths per pixel, float64."""
    sp, ca, ls = arrays(name)
    E, _ = strat_ref.trace(sp, ca, W, H, NSUB, seed, frame_coords(n), ls, np.float64, stratified=stratified)
    return E.reshape(H, W, NSUB * NSUB * n, 3).mean(axis=2)


@functools.lru_cache(maxsize=None)
def seed_stats(name, stratified, runs):
    """Mean and variance over the seeds `runs` of the raw means.  Read-only, shared with tests/test_gpu_stratified.py."""
    g = np.stack([raw_mean(name, SAMPLES[name], run_seed(r), stratified) for r in runs])
    m, v = g.mean(0), g.var(0, ddof=1)
    m.setflags(write=False)
    v.setflags(write=False)
    return m, v


def variance_ratio(vp, vs):
    keep = vs > 0
    return float(np.median(vp[keep] / vs[keep])), float(vp.sum() / vs.sum())


def cpu_variance_ratio(name):
    """(median, sum) of the variance plain / stratified of the float64 restatement."""
    return variance_ratio(seed_stats(name, False, PLAIN_A)[1], seed_stats(name, True, FLAGGED)[1])


def _report(name, what, res):
    print(f"{name} at {SAMPLES[name]} samples, {what}: frac {res['frac_abs_z_gt_4.5']:.4f}, mean z "
          f"{res['mean_z']:+.3f}, image mean diff / se {res['image_mean_diff'] / res['image_mean_se']:+.2f}")


# ---- 1 -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_flag_off_is_light_ref(name, dtype):
    sp, ca, ls = arrays(name)
    coords = frame_coords(2)
    for lights in ((), zoo.lights(scene(name)[0])):
        E, segs = strat_ref.trace(sp, ca, W, H, NSUB, SEED, coords, lights, dtype, stratified=False)
        E0, segs0 = light_ref.trace(sp, ca, W, H, NSUB, SEED, coords, lights, dtype)
        assert np.array_equal(E, E0) and np.array_equal(segs, segs0)
        Es, _ = strat_ref.trace(sp, ca, W, H, NSUB, SEED, coords, lights, dtype)
        assert not np.array_equal(Es, E0)


# ---- 2 -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_plain_restatement_against_itself(name):
    (ma, va), (mb, vb) = seed_stats(name, False, PLAIN_B), seed_stats(name, False, PLAIN_A)
    _report(name, "null", two_sample_check(ma, va, mb, vb, RUNS))


# ---- 3, 4 --------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_stratified_is_unbiased_against_the_plain_restatement(name):
    (ms, vs), (mp, vp) = seed_stats(name, True, FLAGGED), seed_stats(name, False, PLAIN_A)
    assert not np.array_equal(ms, mp)
    med, tot = cpu_variance_ratio(name)
    print(f"{name}: variance plain / stratified, median {med:.3f}, sum {tot:.3f}")
    _report(name, "stratified", two_sample_check(ms, vs, mp, vp, RUNS))


def test_simple_reproduces_the_prototype_variance_ratio():
    """The design prototype measured a median of 2.5 on `simple` (64 samples, 12 seeds per side); the same
    estimator at this module's seeds must land near it -- a sampler that fell back to plain draws gives 1."""
    med, tot = cpu_variance_ratio("simple")
    print(f"simple: variance plain / stratified, median {med:.3f}, sum {tot:.3f} (prototype: 2.5, 2.7)")
    assert 2.0 <= med <= 3.2, (med, tot)
