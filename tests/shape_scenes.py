"""Scenes that put the linear scan and the BVH switch at shapes the shipped
scenes never reach (tests/test_scene_shapes.py, test_gpu_scene_shapes.py,
test_gpu_fast_paths.py): rooms of the box scene's walls around 0 .. 59 random
small spheres, rooms with walls missing, one with curved walls and a sphere
beyond a wall's tangent plane, the empty and the one-sphere scene, and
clusters of 12 .. 70 spheres on both sides of the 64-sphere limit, two of them
through a thin lens.  Pure Python and seeded: every call builds the same
scene.  Small spheres may overlap each other and the walls; the oracle
defines the result.
"""
import numpy as np

import ptgpu
import pyoracle as po
from wide_scenes import cluster_scene


def room(n_small, W, H, walls=(0, 1, 2, 3, 4), lit_wall=False, seed=3):
    """The box scene's camera and the walls picked by index (left, right, back,
    top, bottom), in the order given, then n_small random spheres: radius
    U(0.03, 0.12), centre x, y in [-0.4 + r, 0.4 - r], z in [-1 + r, 0.6],
    colour U(0.3, 0.95) per channel, materials cycling diffuse, specular,
    dielectric, every fifth (from index 0) with emission 9.  lit_wall: the
    last listed wall has emission 1.5."""
    scn = ptgpu.make_scene("box", W, H)
    box = scn.spheres[:5]
    picked = [box[i] for i in walls]
    if lit_wall:
        w = picked[-1]
        picked[-1] = ptgpu.sphere(w.radius, w.position, (1.5, 1.5, 1.5), w.color, w.reflection)
    rng = np.random.default_rng(seed)
    mats = (ptgpu.reflection_type.diffuse, ptgpu.reflection_type.specular, ptgpu.reflection_type.dielectric)
    small = []
    for i in range(n_small):
        r = float(rng.uniform(0.03, 0.12))
        pos = (float(rng.uniform(-0.4 + r, 0.4 - r)), float(rng.uniform(-0.4 + r, 0.4 - r)),
               float(rng.uniform(-1.0 + r, 0.6)))
        col = tuple(float(c) for c in rng.uniform(0.3, 0.95, 3))
        emit = (9.0, 9.0, 9.0) if i % 5 == 0 else (0.0, 0.0, 0.0)
        small.append(ptgpu.sphere(r, pos, emit, col, mats[i % 3]))
    scn.spheres = picked + small
    return scn


def _inside0(W, H):
    scn = room(0, W, H, walls=(0, 1, 2, 4, 3), lit_wall=True)
    c = scn.camera_parameters
    c.position = (0.0, 0.0, -0.3)
    c.direction = (0.0, 0.0, -1.0)
    c.focus_distance = 0.7
    return scn


def _single(W, H):
    scn = room(0, W, H, walls=())
    scn.spheres = [ptgpu.sphere(0.5, (0.0, 0.0, -1.0), (2.0, 2.0, 2.0), (0.5, 0.5, 0.5),
                                ptgpu.reflection_type.diffuse)]
    return scn


def _sliver(W, H):
    """open_01 with its two walls curved (radius 50 in place of 1e6: huge by
    the 16x rule, still anchored on x and paired) and a diffuse sphere of
    radius 0.2 in the sliver between the + wall and its tangent plane x = 0.4,
    8 units along z from the anchor, where the sliver is 0.64 wide; wall_clear
    asks nothing of small spheres, so box mode stays on.  The camera (no lens)
    looks back at that sphere's +z face from inside the room.  Bounces off it
    start beyond the plane and outside the wall by far more than eps; those
    that leave along +z with 0 <= d_x / d_z below the wall's slope there
    (0.16; some 8 % of a cosine lobe about +z) move toward the wall in x and
    away from its centre: hb >= 0, c > 0, and the line meets the wall sphere
    behind the origin (disc > 0).  Only the sign of hb keeps the fast mode's
    outside-only wall test (kAxAnyOut) from a hit at c / qq."""
    scn = room(4, W, H, walls=(0, 1))
    for i, sgn in ((0, -1.0), (1, 1.0)):
        w = scn.spheres[i]
        scn.spheres[i] = ptgpu.sphere(50.0, (sgn * 50.4, 0.0, -1.0), w.emission, w.color, w.reflection)
    scn.spheres.append(ptgpu.sphere(0.2, (0.72, 0.0, 7.0), (0.0, 0.0, 0.0), (0.9, 0.9, 0.9),
                                    ptgpu.reflection_type.diffuse))
    c = scn.camera_parameters
    c.position = (0.35, 0.0, 7.9)
    c.direction = (0.72, 0.0, 7.0)
    c.aperture = 0.0
    c.focus_distance = ptgpu.length((0.37, 0.0, -0.9))
    return scn


def _lens(n):
    def build(W, H):
        scn = cluster_scene(n, W, H)
        scn.camera_parameters.aperture = 0.3
        return scn
    return build


# name -> builder(W, H).  (No case needed another seed than room()'s default:
# each passes tests/test_scene_shapes.py's full-scan guard.)
CASES = {
    **{f"room{k}": (lambda W, H, k=k: room(k, W, H)) for k in (1, 2, 3, 4, 5, 16, 59)},
    "inside0": _inside0,
    "outside0": lambda W, H: room(0, W, H, walls=(0, 1, 2, 4, 3), lit_wall=True),
    "open_014": lambda W, H: room(4, W, H, walls=(0, 1, 4)),
    "open_01": lambda W, H: room(4, W, H, walls=(0, 1)),
    "open_342": lambda W, H: room(4, W, H, walls=(3, 4, 2)),
    "open_0134": lambda W, H: room(4, W, H, walls=(0, 1, 3, 4)),
    "open_0234": lambda W, H: room(4, W, H, walls=(0, 2, 3, 4)),
    "sliver": _sliver,
    "empty": lambda W, H: room(0, W, H, walls=()),
    "single": _single,
    **{f"cluster{n}": (lambda W, H, n=n: cluster_scene(n, W, H)) for n in (12, 64, 65, 66, 70)},
    "cluster64_lens": _lens(64),
    "cluster65_lens": _lens(65),
}

ROOMS = [f"room{k}" for k in (1, 2, 3, 4, 5, 16, 59)]
OPEN = ["open_014", "open_01", "open_342", "open_0134", "open_0234"]

# the oracle's anchor axes of each case's leading spheres (its walls):
# 3 + k a wall of axis k's pair, k a single wall of axis k, -1 the general anchor
LAYOUTS = {
    **{name: [3, 3, 2, 4, 4] for name in ROOMS},
    "inside0": [3, 3, 2, 4, 4],
    "outside0": [-1] * 5,
    "open_014": [3, 3, 1],
    "open_01": [3, 3],
    "open_342": [4, 4, 2],
    "open_0134": [3, 3, 4, 4],
    "open_0234": [0, 2, 4, 4],
    "sliver": [3, 3],
}

# cases that run box mode (exact arithmetic), and their small-sphere counts
BOX_MODE = {**{f"room{k}": k for k in (1, 2, 3, 4, 5, 16, 59)}, "inside0": 0, **{name: 4 for name in OPEN},
            "sliver": 5}


def make(name, W, H):
    """(scene, camera) of a named case."""
    scn = CASES[name](W, H)
    return scn, ptgpu.camera.with_config(scn.camera_parameters)


def oracle_arrays(scn, cam):
    return (np.ascontiguousarray(scn.to_array().view(po.SPHERE_DT)),
            np.ascontiguousarray(cam.to_array().view(po.CAMERA_DT)))
