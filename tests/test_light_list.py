"""The light list of PTG_FLAG_LIGHT_SAMPLING (ptg_light_list, host only): the
emissive spheres that scene preparation does not treat as huge, in scene index
order, at most PTG_MAX_LIGHTS of them.
"""
import pytest

import ptgpu

W, H = 64, 48


def _lights(scn):
    return ptgpu.light_list(scn, ptgpu.camera.with_config(scn.camera_parameters))


@pytest.mark.parametrize("name,want", [("box", [5]), ("box_mirror", [5]), ("simple", [3, 4]), ("synthetic:300", [1])])
def test_shipped_scenes(name, want):
    scn = ptgpu.make_scene(name, W, H)
    assert _lights(scn) == want
    for i, s in enumerate(scn.spheres):  # the definition: emissive and neither walls nor ground
        if i in want:
            assert max(s.emission) > 0 and s.radius < 1000
        else:
            assert max(s.emission) == 0 or s.radius >= 100


def _emitter(i, radius=0.05, emission=(0.0, 0.5, 0.0)):
    return ptgpu.sphere(radius, (-0.4 + 0.05 * i, 0.0, -0.5), emission, (0.5, 0.5, 0.5),
                        ptgpu.reflection_type.diffuse)


def test_sixteen_small_emitters_are_accepted_and_one_channel_is_enough():
    scn = ptgpu.make_scene("box", W, H)
    scn.spheres = scn.spheres[:5] + [_emitter(i) for i in range(16)]
    assert _lights(scn) == list(range(5, 21))


def test_seventeen_small_emitters_are_refused():
    scn = ptgpu.make_scene("box", W, H)
    scn.spheres = scn.spheres[:5] + [_emitter(i) for i in range(17)]
    with pytest.raises(ptgpu.PtgError, match=r"\(-4\).*17 small emitters"):  # PTG_ERR_UNSUPPORTED
        _lights(scn)


def test_a_huge_emitter_alone_gives_an_empty_list():
    scn = ptgpu.make_scene("box", W, H)
    lit_wall = scn.spheres[3]
    scn.spheres = [ptgpu.sphere(lit_wall.radius, lit_wall.position, (1.5, 1.5, 1.5), lit_wall.color,
                                lit_wall.reflection),
                   _emitter(0, emission=(0.0, 0.0, 0.0))]
    assert lit_wall.radius >= 1000
    assert _lights(scn) == []


def test_any_material_qualifies():
    scn = ptgpu.make_scene("box", W, H)
    scn.spheres = scn.spheres[:5] + [
        ptgpu.sphere(0.05, (0.1 * k, 0.0, -0.5), (1.0, 1.0, 1.0), (0.5, 0.5, 0.5), m)
        for k, m in enumerate((ptgpu.reflection_type.diffuse, ptgpu.reflection_type.specular,
                               ptgpu.reflection_type.dielectric))]
    assert _lights(scn) == [5, 6, 7]
