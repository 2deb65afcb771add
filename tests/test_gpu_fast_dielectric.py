"""The fast mode's dielectric sampler on scenes that are mostly glass.

The fast instantiation of shade() takes cos theta from the facing normal's dot
with the ray (kn r1 in place of -v1.nn) and |r_out_perp|^2 from
(ratio sin theta)^2 in place of perp.perp.  Both are
identities for unit nn and v1, so they move a path only where a rounding
decides: at grazing incidence, at the total-reflection threshold and on the
way out of the sphere.  Three 64x48 scenes put most paths there:

    glass_single       tests/shape_scenes.py's `single`, its sphere a clear
                       dielectric that fills 84 % of the view's height, the sky
                       the only light: every path that enters bounces inside
                       until a Fresnel draw lets it out (limb = grazing)
    glass_inside       the camera inside a dielectric sphere of radius 1, 0.7
                       off its centre, looking 45 degrees off the radius: the
                       first hit's sin theta runs from 0.31 to 0.63 over the
                       view, across the total-reflection threshold 0.5 (a ray
                       that enters a sphere from outside always meets it
                       again below that threshold, so only a path born inside
                       is totally reflected); colour 0.9, so the roulette
                       ends the trapped paths
    glass_mirror_room  the box scene's room (top wall lit) around box's own
                       touching pair, one dielectric and one mirror sphere

(a) render kernel == trace kernel, bit for bit, on the whole 64x48 frame
    (test_gpu_fast_paths.py (a)'s identity; 12,288 paths).
(b) fast against exact on 4,096 seeded paths, test_gpu_fast_paths.py (b)'s
    rule: moved <= 3 y + 2, y the oracle's own count for the scene.

Measured on an MI355X (parent = the sampler before this change):

    scene               y   parent   this tree   bound (3 y + 2)
    glass_single        0      0         0           2
    glass_inside        0      0         0           2
    glass_mirror_room   7      6         6          23
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import ptgpu  # noqa: E402
import pyoracle as po  # noqa: E402
import shape_scenes as ss  # noqa: E402
import test_gpu_fast_paths as fp  # noqa: E402

W, H = 64, 48
G, S = ptgpu.reflection_type.dielectric, ptgpu.reflection_type.specular


def _glass_single(w, h):
    scn = ss.CASES["single"](w, h)
    # at the camera's focus point, 2.4 away: angular radius asin(0.5 / 2.4) = 0.21 of the view's 0.25 half-height
    scn.spheres = [ptgpu.sphere(0.5, (0.0, 0.0, -0.4), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), G)]
    return scn


def _glass_inside(w, h):
    scn = ss.CASES["single"](w, h)
    scn.spheres = [ptgpu.sphere(1.0, (0.0, 0.0, -1.0), (0.0, 0.0, 0.0), (0.9, 0.9, 0.9), G)]
    c = scn.camera_parameters
    c.position = (0.0, 0.0, -0.3)
    c.direction = (1.0, 0.0, 0.7)  # (the point looked at)
    c.focus_distance = 1.0  # lens radius 0.1: every origin stays inside
    return scn


def _glass_mirror_room(w, h):
    scn = ss.room(0, w, h, walls=(0, 1, 2, 4, 3), lit_wall=True)
    r = 0.2  # box_scene's pair: on the floor, touching each other and the side walls
    scn.spheres += [ptgpu.sphere(r, (r, -r, -0.4), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), S),
                    ptgpu.sphere(r, (-r, -r, -0.4), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), G)]
    return scn


SCENES = {"glass_single": _glass_single, "glass_inside": _glass_inside, "glass_mirror_room": _glass_mirror_room}


def _scene(name, w, h):
    scn = SCENES[name](w, h)
    return scn, ptgpu.camera.with_config(scn.camera_parameters)


# ---- (a) render kernel == trace kernel ---------------------------------------
@pytest.mark.parametrize("name", list(SCENES))
def test_fast_render_kernel_equals_fast_trace_kernel(name, monkeypatch):
    fp._require_gpu()
    monkeypatch.setattr(fp, "_scene", _scene)
    fp.check_render_equals_trace(name, W, H, 1, 2, [(0, 1)])


# ---- (b) fast against exact, path by path -------------------------------------
def _coords():
    rng = np.random.default_rng(11)
    n = fp.N_PATHS
    return np.stack([rng.integers(0, W, n), rng.integers(0, H, n), rng.integers(0, 2, n),
                     rng.integers(0, 2, n), rng.integers(0, 1 << 20, n)], axis=1).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _oracle_yardstick(name):
    """y of test_gpu_fast_paths.py (b) for one of this module's scenes, and the Mode B paths."""
    sp, ca = ss.oracle_arrays(*_scene(name, W, H))
    coords = _coords()

    def run():
        out = np.zeros((fp.N_PATHS, 3), dtype=np.float32)
        segs = np.zeros(fp.N_PATHS, dtype=np.int64)
        for i, (x, y, sx, sy, s) in enumerate(coords.tolist()):
            out[i], segs[i] = po.sample_f32(sp, ca, W, H, 2, fp.SEED, x, y, sx, sy, s)
        return out, segs

    b, bs = run()
    with po.mode_b_variant(po.BV_IEEE_SQRT | po.BV_IEEE_DIV | po.BV_LIBM_TRIG):
        v, vs = run()
    return int(fp._mismatches(b, bs, v, vs).sum()), b, bs


@pytest.mark.parametrize("name", list(SCENES))
def test_fast_dielectric_paths_stay_with_the_exact_paths(name):
    fp._require_gpu()
    y, ref, rsegs = _oracle_yardstick(name)
    coords = torch.from_numpy(_coords()).cuda()
    with ptgpu.Context(*_scene(name, W, H)) as ctx:
        e, es = ctx.trace_samples(coords, ptgpu.make_params(W, H, 1, 2, fp.SEED, flags=fp.EXACT))
        f, fs = ctx.trace_samples(coords, ptgpu.make_params(W, H, 1, 2, fp.SEED))
        torch.cuda.synchronize()
    e, es, f, fs = e.cpu().numpy(), es.cpu().numpy(), f.cpu().numpy(), fs.cpu().numpy()
    assert e.tobytes() == ref.tobytes() and np.array_equal(es, rsegs)  # the exact side is the oracle's Mode B
    bad = fp._mismatches(e, es, f, fs)
    measured, bound = int(bad.sum()), 3 * y + fp.S_SLACK
    glass = int((es > 2).sum())  # paths of more than two segments: these met the glass
    print(f"{name}: y {y}, measured {measured}, bound {bound}; mean segments {es.mean():.2f}, "
          f"{glass} paths of more than 2 segments; first {_coords()[bad][:4].tolist()}")
    assert glass >= fp.N_PATHS // 4  # the scene is what the docstring says
    assert np.isfinite(f).all() and (f >= 0.0).all()
    assert measured <= bound
