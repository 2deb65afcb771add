"""Scenes whose paths leave the range the exact accumulation sums unclipped
(include/ptgpu.h "Sample accumulation": NaN and negative components count as
0, components above 2^30 as 2^30, PTG_FLAG_COUNT_NONFINITE counts such paths).
Used by tests/test_radiance_range_host.py and tests/test_gpu_radiance_range.py.

Every scene is a variant of the box scene (spheres 0-4 the walls, 5 the lamp,
6 the mirror, 7 the glass sphere) or of synthetic:300, pure Python, the same
at every call; every value is finite, so ptg_create_context accepts it.  A
colour above 1 is what makes NaN and inf from finite input: the throughput T
overflows to +inf after a few bounces and the next black surface adds inf * 0.

CLASSES gives, per scene, the paths of each class the oracle's Mode B finds in
the base frame (16x12, 3 samples per sub-pixel, nsub 2, seed 0x5EED0001: 2,304
paths; bvh_mix: 16x9, 2 samples, 1,152 paths).  A path is `nan` when a
component is NaN, `neg` when one is negative, `high` when one is above 2^30
(+inf included), `edge` when one equals 2^30 exactly, `mid` when one lies in
(2^15, 2^30] (its square is clipped again in S2), `sq` when a clipped
component's fp32 square exceeds 2^30.  A class that is not listed is absent.
"""
import numpy as np

import ptgpu

TOP = 2.0 ** 30  # the clip value
NEG_EMISSION = (-0.5, 0.25, -3.0)

# the base frame of every scene: W, H, samples per sub-pixel, nsub
BASE = (16, 12, 3, 2)
BVH_BASE = (16, 9, 2, 2)


def _with(s, **kw):
    f = dict(radius=s.radius, position=s.position, emission=s.emission, color=s.color, reflection=s.reflection)
    f.update(kw)
    return ptgpu.sphere(f["radius"], f["position"], f["emission"], f["color"], f["reflection"])


def _box(W, H, lamp=None, walls=None, others=None):
    """The box scene with keyword changes to the lamp, to every wall (a function of the wall) or to spheres 6 and 7."""
    scn = ptgpu.make_scene("box", W, H)
    if walls:
        for i in range(5):
            scn.spheres[i] = _with(scn.spheres[i], **walls(scn.spheres[i]))
    if lamp:
        scn.spheres[5] = _with(scn.spheres[5], **lamp)
    if others:
        for i in (6, 7):
            scn.spheres[i] = _with(scn.spheres[i], **others)
    return scn


def _over(W, H):
    return _box(W, H, lamp=dict(emission=(2.0 ** 31,) * 3))


def _edge(W, H):
    """A camera ray that meets the lamp carries (2^30, the next float above, the next float below)."""
    return _box(W, H, lamp=dict(emission=(TOP, TOP * (1 + 2.0 ** -23), TOP * (1 - 2.0 ** -24)), color=(0.0, 0.0, 0.0)))


def _bvh_mix(W, H):
    """synthetic:300 with the emitter at (2^31, -2^31, 2^31), colour 1e30 on the
    spheres of even index mod 7 (the ground among them: a path that leaves it
    for the sky is above 2^30, two such bounces overflow T and the next hit
    adds inf * 0) and the emission (-0.5, 0, -3) on those of index 1, 3, 5 mod
    7, which has no positive component: the emitter stays the only listed
    light of PTG_FLAG_LIGHT_SAMPLING.  One sphere in 7 of each kind gave 8
    NaN and 5 negative paths at BVH_BASE; this gives 40 and 27."""
    scn = ptgpu.make_scene("synthetic:300", W, H)
    for i, s in enumerate(scn.spheres):
        if max(s.emission) > 0.0:
            scn.spheres[i] = _with(s, emission=(2.0 ** 31, -(2.0 ** 31), 2.0 ** 31))
        elif i % 7 in (0, 2, 4, 6):
            scn.spheres[i] = _with(s, color=(1e30,) * 3)
        elif i % 7 in (1, 3, 5):
            scn.spheres[i] = _with(s, emission=(-0.5, 0.0, -3.0))
    return scn


def _edge_in(W, H):
    """edge without the component above 2^30: exactly 2^30 is in range, so nothing is clipped or counted."""
    return _box(W, H, lamp=dict(emission=(TOP, TOP * (1 - 2.0 ** -24), 0.5), color=(0.0, 0.0, 0.0)))


CASES = {
    "over": _over,
    "edge": _edge,
    "edge_in": _edge_in,
    "s2sat": lambda W, H: _box(W, H, lamp=dict(emission=(40000.0, 2.0 ** 15, 181.02))),
    "neg": lambda W, H: _box(W, H, others=dict(emission=NEG_EMISSION)),
    "negcolor": lambda W, H: _box(W, H, walls=lambda s: dict(color=(-s.color[0], s.color[1], -0.0))),
    "nanwalls": lambda W, H: _box(W, H, walls=lambda s: dict(color=(1e12,) * 3, emission=(1e-3, 0.0, 1e-3))),
    "cap": lambda W, H: _box(W, H, walls=lambda s: dict(color=(1.0, 1.0, 1.0))),
    "tiny": lambda W, H: _box(W, H, lamp=dict(emission=(2.0 ** -33, 2.0 ** -32, 3 * 2.0 ** -32))),
    "bvh_mix": _bvh_mix,
    # for PTG_FLAG_LIGHT_SAMPLING: `over`, whose lamp (radius 0.2, emission 2^31) is the one listed light
    "over_ls": _over,
}

# measured on the oracle (tests/test_radiance_range_host.py prints them)
CLASSES = {
    "over": dict(high=51),
    "edge": dict(edge=32, high=32, mid=131),
    "edge_in": dict(edge=32, mid=131),
    "s2sat": dict(sq=38),
    "neg": dict(neg=1132),
    "negcolor": dict(neg=34),
    "nanwalls": dict(nan=1837, high=865),
    "cap": dict(),
    "tiny": dict(),
    "bvh_mix": dict(nan=20, neg=20, high=20),  # a floor, not a measurement: at least 20 of each
    "over_ls": dict(high=51),
}
CLIPPED = ("nan", "neg", "high")  # the classes q() clips and PTG_FLAG_COUNT_NONFINITE counts


def base_shape(name):
    return BVH_BASE if name == "bvh_mix" else BASE


def make(name, W, H):
    """(scene, camera) of a named case."""
    scn = CASES[name](W, H)
    return scn, ptgpu.camera.with_config(scn.camera_parameters)


def classes(E):
    """Per class the boolean mask over the paths of E [..., 3] (float32 radiance)."""
    E = np.asarray(E, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        cl = np.minimum(np.where(E >= 0, E, np.float32(0)), np.float32(TOP))
        return {
            "nan": np.isnan(E).any(axis=-1),
            "neg": (E < 0).any(axis=-1),
            "high": (E > np.float32(TOP)).any(axis=-1),
            "edge": (E == np.float32(TOP)).any(axis=-1),
            "mid": ((E > np.float32(2.0 ** 15)) & (E <= np.float32(TOP))).any(axis=-1),
            "sq": ((cl * cl > np.float32(TOP)) & (E <= np.float32(TOP))).any(axis=-1),
        }


def clipped(E):
    """The paths PTG_FLAG_COUNT_NONFINITE counts: a component that is not in [0, 2^30]."""
    c = classes(E)
    return c["nan"] | c["neg"] | c["high"]
