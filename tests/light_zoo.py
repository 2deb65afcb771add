"""Scenes for PTG_FLAG_LIGHT_SAMPLING that the shipped scenes never reach
(tests/test_oracle_light_sampling.py, test_gpu_light_sampling.py,
test_gpu_ref64.py): more than two lights, emitters that are mirrors or glass,
lights that overlap, a light cut by a wall in box mode, lights whose scan
position differs from their scene index, several lights on the BVH kernels,
and hit points INSIDE a light's sphere (a dome light around the scene, a lamp
of emissive glass around a diffuse ball).  Pure Python and without random
numbers: every call builds the same scene.  Every scene is rendered 32 x 24
with 2 x 2 sub-pixels; the oracle's Mode A/xs with the light list defines the
result.

SAMPLES[name] is the sample count per sub-pixel of the statistical tests, fixed
by the null check of tests/test_oracle_light_sampling.py (the plain oracle
against itself passes two_sample_check at that count).
"""
import math

import numpy as np

import ptgpu
import pyoracle as po

W, H, NSUB = 32, 24, 2
D, S, G = ptgpu.reflection_type.diffuse, ptgpu.reflection_type.specular, ptgpu.reflection_type.dielectric
BLACK = (0.0, 0.0, 0.0)
GREY = (0.7, 0.7, 0.7)


def _look(scn, position, at, fov, aperture=0.0):
    c = scn.camera_parameters
    c.position, c.direction = position, at
    c.vertical_fov_radians = fov
    c.aperture = aperture
    c.focus_distance = ptgpu.length(tuple(p - a for p, a in zip(position, at)))
    return scn


def _open(spheres, position, at, fov):
    """A scene under the sky: the box scene's camera type with every field set."""
    scn = ptgpu.make_scene("box", W, H)
    scn.spheres = list(spheres)
    return _look(scn, position, at, fov)


def _floor(y=-0.5):
    """simple_scene's ground: R = 100, plane-like for these cameras (huge: never a light, anchored)."""
    return ptgpu.sphere(100.0, (0.0, y - 100.0, -1.0), BLACK, (0.8, 0.8, 0.8), D)


def _beside():
    return _open([_floor(), ptgpu.sphere(0.5, (0.0, 0.0, -1.0), BLACK, GREY, D),
                  ptgpu.sphere(0.3, (1.0, 0.4, -0.7), (4.0, 4.0, 4.0), BLACK, D)],
                 (0.0, 1.0, 2.5), (0.0, 0.0, -1.0), 0.6)


def _dome():
    """Ball and floor inside one emissive sphere of R = 20, the camera inside
    too: every hit point lies inside the only light."""
    scn = _open([ptgpu.sphere(20.0, (0.0, 0.0, 0.0), (0.8, 0.8, 0.8), (0.3, 0.3, 0.3), D),
                 ptgpu.sphere(5.0, (0.0, -5.5, 0.0), BLACK, (0.8, 0.8, 0.8), D),
                 ptgpu.sphere(0.5, (0.0, 0.0, 0.0), BLACK, GREY, D)],
                (0.0, 1.0, 4.0), (0.0, 0.0, 0.0), 0.6)
    assert lights(scn) == [0]  # R = 20 is neither >= 1000 nor plane-like from inside: a listed light
    return scn


def _glass_lamp():
    """A diffuse ball of R 0.2 inside an emissive dielectric of R 0.5, and one
    small diffuse light outside: the ball's hit points lie inside light 0."""
    scn = _open([_floor(), ptgpu.sphere(0.5, (0.0, 0.0, -1.0), (2.0, 2.0, 2.0), (0.999, 0.999, 0.999), G),
                 ptgpu.sphere(0.2, (0.0, 0.0, -1.0), BLACK, GREY, D),
                 ptgpu.sphere(0.25, (1.0, 0.8, -0.5), (5.0, 5.0, 5.0), BLACK, D)],
                (0.0, 0.8, 2.2), (0.0, 0.0, -1.0), 0.6)
    assert lights(scn) == [1, 3]
    return scn


def _three():
    """L = 3 (the pick (m L) >> 24 with L no power of two): two overlapping
    diffuse lights of different emission and an emissive mirror."""
    scn = _open([_floor(), ptgpu.sphere(0.5, (0.0, 0.0, -1.0), BLACK, GREY, D),
                 ptgpu.sphere(0.3, (-0.9, 0.6, -1.0), (6.0, 3.0, 1.0), BLACK, D),
                 ptgpu.sphere(0.25, (-0.6, 0.7, -1.0), (1.0, 3.0, 6.0), BLACK, D),
                 ptgpu.sphere(0.3, (0.95, 0.1, -0.8), (1.5, 1.5, 1.5), (0.9, 0.9, 0.9), S)],
                (0.0, 1.0, 2.5), (0.0, 0.1, -1.0), 0.7)
    assert lights(scn) == [2, 3, 4]
    return scn


FLOOR16 = 100.0  # `sixteen`'s floor: a sphere of this radius under the origin, its top at y = 0


def _rest(r, rho):
    """Centre height of a sphere of radius r resting on that floor at horizontal distance rho from its top."""
    return math.sqrt((FLOOR16 + r) ** 2 - rho * rho) - FLOOR16


def sixteen_lights():
    """The 16 lights of `sixteen` as (radius, position, emission, colour,
    material) tuples: radii 0.02 .. 2 in equal ratios, on an outward spiral
    over the floor, materials cycling diffuse, mirror, glass; every fourth
    rests tangent on the floor, the others float 0.3, 0.6, 0.9 above that; the
    smallest is moved far away (|centre| > 50) and stays dim, so that the rare
    path that meets it carries no weight."""
    out = []
    for i in range(16):
        r = 0.02 * 100.0 ** (i / 15.0)
        ang, dist = 2.4 * i, 1.5 + 0.35 * i
        pos = (dist * math.cos(ang), _rest(r, dist) + 0.3 * (i % 4), dist * math.sin(ang))
        e = 0.25 / r if r < 0.25 else 1.0
        emit = (e * (1.0 + (i % 3)), e * (1.0 + 0.5 * (i % 5)), e * (3.0 - 0.6 * (i % 4)))
        if i == 0:
            pos, emit = (30.0, 25.0, -40.0), (5.0, 5.0, 5.0)
        col = BLACK if i % 3 == 0 else (0.9, 0.9, 0.9)
        out.append((r, pos, emit, col, (D, S, G)[i % 3]))
    return out


def _sixteen():
    """L = 16 over a floor of R = 100 (plane-like for the camera: anchored, never a light)."""
    scn = _open([ptgpu.sphere(FLOOR16, (0.0, -FLOOR16, 0.0), BLACK, (0.6, 0.6, 0.6), D),
                 ptgpu.sphere(0.6, (0.0, 0.6, 0.0), BLACK, GREY, D)]
                + [ptgpu.sphere(*t) for t in sixteen_lights()],
                (0.0, 3.0, 9.0), (0.0, 0.5, 0.0), 0.8)
    assert lights(scn) == list(range(2, 18))
    t = scn.spheres[6]  # (i = 4: tangent on the floor)
    gap = ptgpu.length((t.position[0], t.position[1] + FLOOR16, t.position[2])) - (FLOOR16 + t.radius)
    assert abs(gap) < 1e-12, gap
    return scn


def _through_ceiling():
    """The box room with its lamp replaced by a sphere of R = 1 whose cap
    (0.03 deep, 0.24 across) pokes through the ceiling wall y = 0.4, as
    smallpt hangs its lamp.  R < 1000 and not plane-like for the camera, so it
    stays on the light list, while the five walls keep their pairs and box
    mode (test_gpu_light_sampling.py asserts launch_info's box mode)."""
    scn = ptgpu.make_scene("box", W, H)
    scn.spheres[5] = ptgpu.sphere(1.0, (0.0, 1.37, -0.5), (9.0, 9.0, 9.0), BLACK, D)
    cam = ptgpu.camera.with_config(scn.camera_parameters)
    lamp = scn.spheres[5]
    gap = abs(ptgpu.length(tuple(c - p for c, p in zip(cam.position, lamp.position))) - lamp.radius)
    assert lamp.radius < 1000.0 and not lamp.radius > 16.0 * (gap + 1.0)  # the two rules of "huge"
    assert lights(scn) == [5]
    assert ptgpu.scene_layout(scn, cam)[0][:5] == [3, 3, 2, 4, 4]  # x and y walls paired, the back wall alone
    return scn


def _permuted():
    """A linear scene whose scan (huge spheres first, then the small ones in
    index order) tests the lights at indices 0 and 2 at positions 2 and 3."""
    scn = _open([ptgpu.sphere(0.2, (-0.9, 0.5, -0.8), (8.0, 6.0, 4.0), BLACK, D),
                 ptgpu.sphere(1000.0, (0.0, -1000.5, -1.0), BLACK, (0.8, 0.8, 0.8), D),
                 ptgpu.sphere(0.25, (0.9, 0.0, -0.6), (2.0, 2.0, 2.0), (0.9, 0.9, 0.9), S),
                 ptgpu.sphere(1e5, (0.0, 0.0, -1e5 - 3.0), BLACK, (0.4, 0.5, 0.8), D),
                 ptgpu.sphere(0.5, (0.0, 0.0, -1.0), BLACK, GREY, D),
                 ptgpu.sphere(0.15, (0.3, 0.9, -0.2), (4.0, 8.0, 4.0), BLACK, D)],
                (0.0, 1.0, 2.5), (0.0, 0.0, -1.0), 0.7)
    ls = lights(scn)
    assert ls == [0, 2, 5]
    order = po.scan_layout(*oracle_arrays(scn, ptgpu.camera.with_config(scn.camera_parameters)))[1]
    assert sum(order.index(i) != i for i in ls) >= 2, order
    return scn


def _bvh_lights():
    """synthetic:300 with one emitter inserted at index 0 and three appended:
    every scene index shifts, L = 5 on the BVH kernels."""
    scn = ptgpu.make_scene("synthetic:300", W, H)
    scn.spheres = ([ptgpu.sphere(0.3, (-3.0, 0.3, 2.0), (6.0, 4.0, 2.0), BLACK, D)] + scn.spheres +
                   [ptgpu.sphere(0.4, (3.0, 1.0, 1.0), (2.0, 4.0, 6.0), BLACK, D),
                    ptgpu.sphere(0.5, (0.0, 0.5, 4.0), (1.0, 1.0, 1.0), (0.9, 0.9, 0.9), S),
                    ptgpu.sphere(0.4, (-1.5, 0.4, 5.0), (2.0, 2.0, 2.0), (0.999, 0.999, 0.999), G)])
    assert len(scn.spheres) == 304 and lights(scn) == [0, 2, 301, 302, 303]
    return scn


CASES = {"beside": _beside, "dome": _dome, "glass_lamp": _glass_lamp, "three": _three, "sixteen": _sixteen,
         "through_ceiling": _through_ceiling, "permuted": _permuted, "bvh_lights": _bvh_lights}

# samples per sub-pixel of the statistical tests (see the module docstring)
SAMPLES = {"beside": 128, "dome": 64, "glass_lamp": 256, "three": 128, "sixteen": 128, "through_ceiling": 128,
           "permuted": 128, "bvh_lights": 128}


def lights(scn):
    return ptgpu.light_list(scn, ptgpu.camera.with_config(scn.camera_parameters))


def make(name):
    """(scene, camera, light list) of a named case."""
    scn = CASES[name]()
    return scn, ptgpu.camera.with_config(scn.camera_parameters), lights(scn)


def oracle_arrays(scn, cam):
    return (np.ascontiguousarray(scn.to_array().view(po.SPHERE_DT)),
            np.ascontiguousarray(cam.to_array().view(po.CAMERA_DT)))
