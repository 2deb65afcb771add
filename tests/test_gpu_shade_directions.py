"""shade()'s shared second draw and its one next-direction formula.

The fast instantiation of shade() forms the next direction of every material
as one linear combination nn K3 + vv K2 + v1 K1.  For a
diffuse and for a reflecting lane that is the earlier arithmetic operation by
operation; only a refracting lane's direction is rounded differently.  The
second xorshift step is taken once for the whole diffuse/dielectric block, in
both arithmetic modes, and must leave every lane's stream where it was.

(a) Lanes that never refract keep their bits: 4,096 seeded paths through the
    two scenes of tests/shade_direction_scenes.py (no dielectric), from the
    trace kernel in the fast and in the exact mode, against
    tests/golden/fast_paths_no_glass.npz -- recorded with
    tools/gen_fast_path_pins.py on the commit before this change (two runs,
    identical files).
(b) On the same scenes the fast render kernel equals the fast trace kernel on
    the whole 64x48 frame (test_gpu_fast_paths.py (a)'s identity).

Refracting lanes are fenced by test_gpu_fast_paths.py (b) and
test_gpu_fast_dielectric.py (b), unchanged: fast against exact on 4,096
paths, moved <= 3 y + 2, y the oracle's own count.  Measured on an MI355X
(parent = the kernel before this change):

    scene               y   parent   this tree   bound (3 y + 2)
    glass_single        0      0         0            2
    glass_inside        0      0         0            2
    glass_mirror_room   7      6         7           23
    box                 3      5         5           11
    box_mirror          8     11        11           26
    simple              0      0         0            2
    room4               0      0         0            2
    room16              9      9         8           29
    room59             45     44        44          137
    sunk_scene         12     11        11           38
    open_014            0      1         1            2
    sliver              0      0         0            2
    synthetic:300       0      0         0            2
    cluster64           0      0         0            2
    cluster65           0      0         0            2

(the first three rows are test_gpu_fast_dielectric.py's scenes, the others
test_gpu_fast_paths.py's)
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import shade_direction_scenes as sd  # noqa: E402
import test_gpu_fast_paths as fp  # noqa: E402


# ---- (a) the pinned paths ------------------------------------------------------
@pytest.mark.parametrize("name", list(sd.SCENES))
def test_paths_without_glass_keep_their_bits(name):
    fp._require_gpu()
    pins = np.load(sd.FIXTURE)
    assert np.array_equal(pins["coords"], sd.coords())  # the fixture is of these paths
    got = sd.trace(name)
    for mode in sd.MODES:
        rad, segs = got[mode]
        want_r, want_s = pins[f"{name}.{mode}.radiance"], pins[f"{name}.{mode}.segments"]
        bad = (rad.view(np.uint32) != want_r).any(axis=1) | (segs != want_s)
        print(f"{name} {mode}: {int(bad.sum())} of {sd.N_PATHS} paths differ from the pins; mean segments "
              f"{segs.mean():.2f}; first {sd.coords()[bad][:4].tolist()}")
        assert np.isfinite(rad).all()
        assert (want_s > 2).sum() >= sd.N_PATHS // 4  # the paths bounce: they run shade()'s samplers
        assert not bad.any()


# ---- (b) render kernel == trace kernel ------------------------------------------
@pytest.mark.parametrize("name", list(sd.SCENES))
def test_fast_render_kernel_equals_fast_trace_kernel(name, monkeypatch):
    fp._require_gpu()
    monkeypatch.setattr(fp, "_scene", lambda n, w, h: sd.scene(n, w, h))
    fp.check_render_equals_trace(name, sd.W, sd.H, 1, sd.NSUB, [(0, 1)])
