"""Scenes of the followed-feature tests (tests/test_follow_host.py on the CPU,
tests/test_gpu_follow_features.py on the GPU); no test of its own."""
import ptgpu
from denoise_camera import OFF_AXIS
from ptgpu.scene import _sub, length, reflection_type, scene, sphere

D, S, G = reflection_type.diffuse, reflection_type.specular, reflection_type.dielectric

# (scene, width, height): the GPU cases, each at nsub 1 and 2 and at B = 1, 2 and 8
GPU_CASES = [("box", 64, 48), ("simple", 64, 48), ("box_mirror", 64, 48), ("synthetic:300", 32, 18),
             ("mirror_back", 64, 48)]
BOUNCES = (1, 2, 8)
MARGIN = 1e-4      # rays whose float64 margin is below this are excluded
MAX_EXCLUDED = 0.02  # of a case's pixels


def mirror_back(W, H):
    """The box scene with its back wall a mirror of colour 0.999: the wall the
    camera looks at shows the room's other surfaces and the balls from behind."""
    scn = ptgpu.make_scene("box", W, H)
    back = scn.spheres[2]
    assert back.position[2] < -1e5  # the back wall (ptgpu/scene.py _box)
    scn.spheres[2] = sphere(back.radius, back.position, back.emission, (0.999, 0.999, 0.999), S)
    return scn


def box_all_diffuse(W, H):
    """The box scene with its mirror and glass balls made diffuse: nothing to follow."""
    scn = ptgpu.make_scene("box", W, H)
    scn.spheres = [sphere(s.radius, s.position, s.emission, s.color, D) for s in scn.spheres]
    return scn


def _off_axis(scn):
    c = scn.camera_parameters
    c.position = tuple(p + o for p, o in zip(c.position, OFF_AXIS))
    c.focus_distance = length(_sub(c.position, c.direction))
    return scn


# synthetic:300 is 300 spheres of radius 0.05..0.15 on the ground of a 20 x 20 field, seen by its own camera
# from 12 away: every small sphere then has |disc| / hb^2 <= (r / D)^2 < 1.6e-4, and nearly all rays that hit
# one are under the margin.  The camera is moved instead (never the cap): 1.3 above one glass ball, looking
# down at it, the ground behind it -- 0.7 % of the pixels are excluded (float64 restatement, nsub 2, B = 8)
# and 25 of the 576 pixels follow a chain.
SYNTH_TARGET, SYNTH_OFFSET = 292, (0.3, 1.2, 0.4)


def scene_and_camera(name, W, H, off_axis=True):
    """The box scenes from a little off the room's axis (tests/denoise_camera.py),
    synthetic:300 from close by (above)."""
    if name == "mirror_back":
        scn = mirror_back(W, H)
    elif name == "box_all_diffuse":
        scn = box_all_diffuse(W, H)
    else:
        scn = ptgpu.make_scene(name, W, H)
    if off_axis and (name.startswith("box") or name == "mirror_back"):
        _off_axis(scn)
    if name == "synthetic:300":
        c = scn.camera_parameters
        c.direction = tuple(scn.spheres[SYNTH_TARGET].position)
        c.position = tuple(p + o for p, o in zip(c.direction, SYNTH_OFFSET))
        c.focus_distance = length(_sub(c.position, c.direction))
    return scn, ptgpu.camera.with_config(scn.camera_parameters)


def _look(scn, position, at, W, H, fov):
    c = scn.camera_parameters
    c.position, c.direction = position, at
    c.aspect_ratio = W / H
    c.vertical_fov_radians = fov
    c.aperture = 0.0
    c.focus_distance = length(_sub(position, at))
    return scn, ptgpu.camera.with_config(c)


MIRROR_R, BALL_R = 1e5, 0.15


def mirror_plane(W, H, mirrored_camera=False):
    """A diffuse ball and a diffuse floor in front of a plane-like mirror: one
    specular sphere of radius 1e5 whose surface touches z = 0 at the origin.
    The camera at (0.3, 0.4, 3) looks at the mirror; mirrored_camera: the same
    scene without the mirror seen from the camera's image in the plane z = 0,
    (0.3, 0.4, -3), looking the mirrored way."""
    spheres = [sphere(BALL_R, (0.6, 0.1, 1.0), (0, 0, 0), (0.2, 0.6, 0.9), D),
               sphere(1000.0, (0.0, -1001.0, 1.0), (0, 0, 0), (0.7, 0.7, 0.3), D)]
    if not mirrored_camera:
        spheres.append(sphere(MIRROR_R, (0.0, 0.0, -MIRROR_R), (0, 0, 0), (1.0, 1.0, 1.0), S))
        return _look(scene(spheres), (0.3, 0.4, 3.0), (0.3, 0.4, 0.0), W, H, 0.5)
    return _look(scene(spheres), (0.3, 0.4, -3.0), (0.3, 0.4, 0.0), W, H, 0.5)


def glass_ball(W, H):
    """A glass ball of radius 0.5 at the origin in front of a diffuse wall
    (a sphere of radius 1000 whose surface is the plane z = -2 near the axis)."""
    spheres = [sphere(0.5, (0.0, 0.0, 0.0), (0, 0, 0), (0.9, 0.95, 1.0), G),
               sphere(1000.0, (0.0, 0.0, -1002.0), (0, 0, 0), (0.5, 0.4, 0.3), D)]
    return _look(scene(spheres), (0.05, 0.03, 3.0), (0.0, 0.0, 0.0), W, H, 0.5)


def facing_mirrors(W, H):
    """Two mirror spheres of radius 1e5 facing each other across the gap
    |x| < 1, the camera between them looking at one: every ray bounces between
    the two for ever."""
    spheres = [sphere(MIRROR_R, (-MIRROR_R - 1.0, 0.0, 0.0), (0, 0, 0), (0.9, 0.9, 0.9), S),
               sphere(MIRROR_R, (MIRROR_R + 1.0, 0.0, 0.0), (0, 0, 0), (0.9, 0.9, 0.9), S)]
    return _look(scene(spheres), (0.0, 0.0, 0.0), (1.0, 0.02, 0.03), W, H, 0.4)
