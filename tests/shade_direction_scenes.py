"""Two scenes without a dielectric, and the seeded paths traced through them
(tests/test_gpu_shade_directions.py, tools/gen_fast_path_pins.py).

    mirror_in_diffuse_room   tests/shape_scenes.py's room of diffuse walls, its
                             top wall lit, around box's mirror sphere: diffuse
                             bounces and mirror reflections, no refraction
    mirror_room_diffuse_ball box_mirror's room of mirror walls with its glass
                             sphere made diffuse: waves that hold mirror lanes
                             only (they skip the diffuse/dielectric block) next
                             to waves that mix both materials

No lane of either scene ever refracts, so a change to the refraction's
arithmetic may not move one bit of their paths, in either arithmetic mode.
"""
import os

import numpy as np

import ptgpu
import shape_scenes as ss

W, H, NSUB = 64, 48, 2
N_PATHS = 4096
SEED = 0x5EED0001
D, S, G = ptgpu.reflection_type.diffuse, ptgpu.reflection_type.specular, ptgpu.reflection_type.dielectric
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fast_paths_no_glass.npz")
MODES = {"fast": 0, "exact": ptgpu.FLAG_EXACT_MATH}


def _mirror_in_diffuse_room(w, h):
    scn = ss.room(0, w, h, walls=(0, 1, 2, 4, 3), lit_wall=True)
    r = 0.2  # box_scene's mirror sphere: on the floor, touching the right wall
    scn.spheres.append(ptgpu.sphere(r, (r, -r, -0.4), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), S))
    return scn


def _mirror_room_diffuse_ball(w, h):
    scn = ptgpu.make_scene("box_mirror", w, h)
    glass = [i for i, s in enumerate(scn.spheres) if s.reflection == G]
    assert len(glass) == 1
    s = scn.spheres[glass[0]]
    scn.spheres[glass[0]] = ptgpu.sphere(s.radius, s.position, s.emission, s.color, D)
    return scn


SCENES = {"mirror_in_diffuse_room": _mirror_in_diffuse_room, "mirror_room_diffuse_ball": _mirror_room_diffuse_ball}


def scene(name, w=W, h=H):
    scn = SCENES[name](w, h)
    assert all(s.reflection != G for s in scn.spheres)
    return scn, ptgpu.camera.with_config(scn.camera_parameters)


def coords():
    """N_PATHS seeded paths of the W x H frame: x, y, sx, sy, sample."""
    rng = np.random.default_rng(23)
    n = N_PATHS
    return np.stack([rng.integers(0, W, n), rng.integers(0, H, n), rng.integers(0, NSUB, n),
                     rng.integers(0, NSUB, n), rng.integers(0, 1 << 20, n)], axis=1).astype(np.int32)


def trace(name):
    """{mode: (radiance float32 [N_PATHS, 3], segments int32 [N_PATHS])} from the trace kernel (needs a GPU)."""
    import torch
    c = torch.from_numpy(coords()).cuda()
    out = {}
    with ptgpu.Context(*scene(name)) as ctx:
        for mode, flags in MODES.items():
            r, s = ctx.trace_samples(c, ptgpu.make_params(W, H, 1, NSUB, SEED, flags=flags))
            torch.cuda.synchronize()
            out[mode] = (r.cpu().numpy(), s.cpu().numpy())
    return out
