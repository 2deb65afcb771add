"""Scenes in which two or more spheres give exactly the same root
(tests/test_tie_scenes_host.py, test_gpu_ties.py and the parametrised lists of
test_gpu_fast_paths.py, test_gpu_denoise.py): include/ptgpu.h's rule at
ptg_scene_layout -- linear scenes give a tie to the sphere visited first, BVH
scenes to the lowest scene index -- is what these scenes see and no other
scene of the suite does.  Pure Python and seeded: every call builds the same
scene.

A twin is built from its original's own Python values of radius and position,
so it is the same sphere in double and in fp32.  It differs in colour, in
material (cycling diffuse, specular, dielectric by twin) and, every fifth
twin, in emission.  The `near_*` cases are no ties: the twin's float32 radius
is moved by +-1 or +-8 ulps, which probes the cull margins of the BVH leaf
test and the box cap; they are compared with Mode B only, never with double.

Twins are given to every `stride`-th sphere that is not huge, starting at
scene index 1 (a cluster's lamp): cluster_scene(40) has 20 twins (60 spheres,
linear), cluster_scene(60) 30 twins (90 spheres: one more than the 89 the
cases were first drafted with, which counted from index 2), cluster_scene(200)
with stride 4 has 50, room(16) has 8.
"""
import numpy as np

import light_zoo as zoo
import ptgpu
import pyoracle as po
from shape_scenes import room
from wide_scenes import cluster_scene

D, S, G = ptgpu.reflection_type.diffuse, ptgpu.reflection_type.specular, ptgpu.reflection_type.dielectric
MATS = (D, S, G)
BLACK = (0.0, 0.0, 0.0)
STACK = (1.2, (0.0, 3.0, 8.0))  # stack9's sphere: in front of the cluster, in the middle of the frame


def _twin(s, k, rng, ulps=0):
    """Twin number k of sphere s: its geometry (the float32 radius moved by
    `ulps`), another colour, material k mod 3, every fifth an emitter."""
    r = s.radius
    if ulps:
        r32 = np.float32(r)
        for _ in range(abs(ulps)):
            r32 = np.nextafter(r32, np.float32(np.inf if ulps > 0 else 0.0))
        r = float(r32)
    col = tuple(float(c) for c in rng.uniform(0.2, 0.95, 3))
    emit = (2.0, 1.5, 1.0) if k % 5 == 0 else BLACK
    return ptgpu.sphere(r, s.position, emit, col, MATS[k % 3])


def _is_huge(s, cam):
    """kernel_args.hpp is_huge."""
    d = ptgpu.length(tuple(cam.position[c] - s.position[c] for c in range(3)))
    return s.radius >= 1000.0 or s.radius > 16.0 * (abs(d - s.radius) + 1.0)


def with_twins(scn, stride=2, low=False, ulps=0, seed=11):
    """Every stride-th non-huge sphere of scn twinned: the twin appended, or
    (low) at the original's index with the original appended."""
    rng = np.random.default_rng(seed)
    cam = ptgpu.camera.with_config(scn.camera_parameters)
    small = [i for i, s in enumerate(scn.spheres) if not _is_huge(s, cam)]
    for k, i in enumerate(small[::stride]):
        s = scn.spheres[i]
        t = _twin(s, k, rng, ulps)
        if low:
            scn.spheres[i] = t
            scn.spheres.append(s)
        else:
            scn.spheres.append(t)
    return scn


def _twin_wall(W, H):
    """room(4) with its back wall once more after the small spheres, lit."""
    scn = room(4, W, H)
    w = scn.spheres[2]
    scn.spheres.append(ptgpu.sphere(w.radius, w.position, (1.5, 1.5, 1.5), (0.9, 0.5, 0.2), w.reflection))
    return scn


def _stack9(first):
    """cluster_scene(70) with nine copies of one sphere at the scene indices
    2 + 7 j; copy j has material and colour number (j + first) mod 9.  Nine
    copies are more than a leaf holds (6): the tie crosses leaves."""
    def build(W, H):
        scn = cluster_scene(70, W, H)
        rng = np.random.default_rng(23)
        cols = [tuple(float(c) for c in rng.uniform(0.2, 0.95, 3)) for _ in range(9)]
        for j in range(9):
            m = (j + first) % 9
            emit = (1.5, 2.0, 1.0) if m % 4 == 3 else BLACK
            scn.spheres.insert(2 + 7 * j, ptgpu.sphere(STACK[0], STACK[1], emit, cols[m], MATS[m % 3]))
        return scn
    return build


def _twin_floor(W, H):
    """cluster_scene(70) with its R = 1000 floor once more at the end: a tie among the huge spheres."""
    scn = cluster_scene(70, W, H)
    f = scn.spheres[0]
    scn.spheres.append(ptgpu.sphere(f.radius, f.position, BLACK, (0.9, 0.3, 0.1), S))
    return scn


def _lamps(dark_first):
    """light_zoo's `three` with a black diffuse twin of each of its lights
    (scene indices 2, 3, 4), inserted before the lights or appended."""
    def build(W, H):
        assert W * zoo.H == H * zoo.W  # (the zoo's cameras are built for 32 x 24)
        scn = zoo.CASES["three"]()
        lamps = scn.spheres[2:5]
        dark = [ptgpu.sphere(s.radius, s.position, BLACK, BLACK, D) for s in lamps]
        scn.spheres = scn.spheres[:2] + (dark + lamps if dark_first else lamps + dark)
        assert zoo.lights(scn) == ([5, 6, 7] if dark_first else [2, 3, 4])
        return scn
    return build


CASES = {
    "twins_lin": lambda W, H: with_twins(cluster_scene(40, W, H)),
    "twins_lin_low": lambda W, H: with_twins(cluster_scene(40, W, H), low=True),
    "twins_room": lambda W, H: with_twins(room(16, W, H)),
    "twins_room_low": lambda W, H: with_twins(room(16, W, H), low=True),
    "twin_wall": _twin_wall,
    "twins_bvh": lambda W, H: with_twins(cluster_scene(60, W, H)),
    "twins_bvh_low": lambda W, H: with_twins(cluster_scene(60, W, H), low=True),
    "twins_bvh250": lambda W, H: with_twins(cluster_scene(200, W, H), stride=4),
    "stack9_a": _stack9(0),
    "stack9_b": _stack9(1),
    "stack9_c": _stack9(2),
    "twin_floor": _twin_floor,
    "near_up1": lambda W, H: with_twins(cluster_scene(60, W, H), ulps=1),
    "near_down1": lambda W, H: with_twins(cluster_scene(60, W, H), ulps=-1),
    "near_up8": lambda W, H: with_twins(cluster_scene(60, W, H), ulps=8),
    "near_down8": lambda W, H: with_twins(cluster_scene(60, W, H), ulps=-8),
    "near_lin_up1": lambda W, H: with_twins(cluster_scene(40, W, H), ulps=1),
    "lamp_dark_first": _lamps(True),
    "lamp_first": _lamps(False),
}

NEAR = [n for n in CASES if n.startswith("near_")]
LAMPS = ["lamp_dark_first", "lamp_first"]
EXACT_TIES = [n for n in CASES if n not in NEAR]
LINEAR = ["twins_lin", "twins_lin_low", "twins_room", "twins_room_low", "twin_wall", "near_lin_up1"] + LAMPS
BVH = [n for n in CASES if n not in LINEAR]
BVH_TIES = [n for n in BVH if n not in NEAR]

# sphere counts, and the number of groups of equal geometry with their size
COUNTS = {"twins_lin": 60, "twins_lin_low": 60, "twins_room": 29, "twins_room_low": 29, "twin_wall": 10,
          "twins_bvh": 90, "twins_bvh_low": 90, "twins_bvh250": 250, "stack9_a": 79, "stack9_b": 79, "stack9_c": 79,
          "twin_floor": 71, "near_up1": 90, "near_down1": 90, "near_up8": 90, "near_down8": 90, "near_lin_up1": 60,
          "lamp_dark_first": 8, "lamp_first": 8}
GROUPS = {"twins_lin": (20, 2), "twins_lin_low": (20, 2), "twins_room": (8, 2), "twins_room_low": (8, 2),
          "twin_wall": (1, 2), "twins_bvh": (30, 2), "twins_bvh_low": (30, 2), "twins_bvh250": (50, 2),
          "stack9_a": (1, 9), "stack9_b": (1, 9), "stack9_c": (1, 9), "twin_floor": (1, 2),
          "lamp_dark_first": (3, 2), "lamp_first": (3, 2)}

# what the launch of each linear case looks like: (box_mode, wall_pairs) in exact mode
LINEAR_LAUNCH = {"twins_lin": (0, 0), "twins_lin_low": (0, 0), "near_lin_up1": (0, 0), "twins_room": (1, 3),
                 "twins_room_low": (1, 3), "twin_wall": (0, 3), "lamp_dark_first": (0, 0), "lamp_first": (0, 0)}


def groups(scn):
    """The groups of two or more spheres of equal geometry: lists of scene indices, ascending."""
    by = {}
    for i, s in enumerate(scn.spheres):
        by.setdefault((s.radius, tuple(s.position)), []).append(i)
    return [g for g in by.values() if len(g) > 1]


def swapped(name, W, H):
    """The case with the scene indices inside every group of equal geometry reversed."""
    scn = CASES[name](W, H)
    old = list(scn.spheres)
    for g in groups(scn):
        for i, j in zip(g, reversed(g)):
            scn.spheres[i] = old[j]
    return scn, ptgpu.camera.with_config(scn.camera_parameters)


def winners_only(name, W, H):
    """The twin-free scene that the rule makes of an exact-tie case: of every
    group of equal geometry only the member with the lowest scene index (in a
    linear case that is the one visited first: the members of a group are of
    one kind).  The others are never seen."""
    scn = CASES[name](W, H)
    drop = {i for g in groups(scn) for i in g[1:]}
    scn.spheres = [s for i, s in enumerate(scn.spheres) if i not in drop]
    return scn, ptgpu.camera.with_config(scn.camera_parameters)


def permuted(name, W, H, keep_groups, seed=5):
    """The case with its sphere list permuted (seeded).  keep_groups: the
    members of every group of equal geometry keep their relative order; else
    every group's order is reversed."""
    scn = CASES[name](W, H)
    old = list(scn.spheres)
    was = {id(s): i for i, s in enumerate(old)}
    perm = np.random.default_rng(seed).permutation(len(old)).tolist()
    scn.spheres = [old[i] for i in perm]
    for g in groups(scn):
        members = sorted((scn.spheres[i] for i in g), key=lambda s: was[id(s)], reverse=not keep_groups)
        for i, s in zip(g, members):
            scn.spheres[i] = s
    return scn, ptgpu.camera.with_config(scn.camera_parameters)


def frame(name):
    """The frame of the image tests: the lamp cases at the zoo's size, one case ragged."""
    if name in LAMPS:
        return zoo.W, zoo.H
    return (37, 23) if name == "twins_room_low" else (48, 32)


def make(name, W, H):
    """(scene, camera) of a named case."""
    scn = CASES[name](W, H)
    return scn, ptgpu.camera.with_config(scn.camera_parameters)


def oracle_arrays(scn, cam):
    return (np.ascontiguousarray(scn.to_array().view(po.SPHERE_DT)),
            np.ascontiguousarray(cam.to_array().view(po.CAMERA_DT)))
