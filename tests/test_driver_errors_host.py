"""Every whole-frame driver's answer to one bad argument, byte for byte (no GPU).

The drivers -- five on one device, their five ptg_multi_* forms, the five
one-shot *_multi forms -- share their target checks, so the status and the
ptg_last_error() text of each single-bad-argument case are pinned against
tests/golden/driver_errors.json, recorded from the library of the commit
before the checks were shared (tools/build_prev.sh, then
`PTGPU_LIB=.../build/libptgpu_prev.so python tests/test_driver_errors_host.py
--record` writes the file from whatever library is loaded).

Every case returns before any device work, so the answers are the same with
and without a GPU.  The ptg_multi_* forms need a live handle for everything but
their NULL-handle case; tests/test_gpu_driver_golden.py runs them on a device.
"""
import ctypes as C
import json
import os
import sys

import numpy as np

if __name__ == "__main__":  # --record: the paths tests/conftest.py sets
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(_root, "cpu-path-tracing_amd"))

import ptgpu  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "driver_errors.json")
W = H = 8

# entry point -> (form, target, filtered).  form "one": scene, params, device; "shot": scene, params, devices, n;
# "ctx": handle, params.  Then target, filter, image, sample counts (adaptive), report (with a target).
DRIVERS = {
    "ptg_render_to_noise": ("one", "noise", False),
    "ptg_render_adaptive": ("one", "adaptive", False),
    "ptg_render_denoised": ("one", None, True),
    "ptg_render_to_noise_denoised": ("one", "noise", True),
    "ptg_render_adaptive_denoised": ("one", "adaptive", True),
    "ptg_multi_render_to_noise": ("ctx", "noise", False),
    "ptg_multi_render_adaptive": ("ctx", "adaptive", False),
    "ptg_multi_render_denoised": ("ctx", None, True),
    "ptg_multi_render_to_noise_denoised": ("ctx", "noise", True),
    "ptg_multi_render_adaptive_denoised": ("ctx", "adaptive", True),
    "ptg_render_to_noise_multi": ("shot", "noise", False),
    "ptg_render_adaptive_multi": ("shot", "adaptive", False),
    "ptg_render_denoised_multi": ("shot", None, True),
    "ptg_render_to_noise_denoised_multi": ("shot", "noise", True),
    "ptg_render_adaptive_denoised_multi": ("shot", "adaptive", True),
}

NAN = float("nan")
# case -> (who it applies to, the one argument it spoils)
ANY, TARGET, ADAPTIVE, FILTERED, SHOT = "any", "target", "adaptive", "filtered", "shot"
CASES = {
    "null_image": (ANY, dict(image=None)),
    "null_params": (ANY, dict(params=None)),
    "null_target": (TARGET, dict(target=None)),
    "null_camera": (FILTERED, dict(camera=None)),  # (an unfiltered driver hands its camera to the context unchecked)
    "floor_zero": (TARGET, dict(floor=0.0)),
    "floor_negative": (TARGET, dict(floor=-1.0)),
    "floor_nan": (TARGET, dict(floor=NAN)),
    "rel_error_negative": (TARGET, dict(rel_error=-1.0)),
    "max_fraction_one": (TARGET, dict(max_fraction=1.0)),
    "max_fraction_negative": (TARGET, dict(max_fraction=-0.5)),
    "max_fraction_nan": (TARGET, dict(max_fraction=NAN)),
    "dilate_minus_one": (ADAPTIVE, dict(dilate=-1)),
    "dilate_nine": (ADAPTIVE, dict(dilate=9)),
    "min_samples_one": (TARGET, dict(min_samples=1)),
    "samples_one": (ANY, dict(samples=1)),
    "shard_count_two": (ANY, dict(shard=(1, 2))),
    "reference_f64": (ANY, dict(flags=ptgpu.FLAG_REFERENCE_F64)),
    "filter_iterations_nine": (FILTERED, dict(iterations=9)),
    "no_device": (SHOT, dict(n_devices=0)),
}


def _applies(who, form, target, filtered):
    return {ANY: True, TARGET: target is not None, ADAPTIVE: target == "adaptive", FILTERED: filtered,
            SHOT: form == "shot"}[who]


def cases_of(entry):
    form, target, filtered = DRIVERS[entry]
    if form == "ctx":
        return {"null_handle": {}}
    return {name: bad for name, (who, bad) in CASES.items() if _applies(who, form, target, filtered)}


def _vp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _ref(x):
    return C.byref(x) if x is not None else None


def call(entry, bad, image):
    """One call of `entry` with every argument good but the one `bad` names; (status, message)."""
    L = ptgpu.lib()
    form, target, filtered = DRIVERS[entry]
    scn = ptgpu.box_scene(W, H)
    sp, ca = scn.to_array(), ptgpu.camera.with_config(scn.camera_parameters).to_array()
    if "camera" in bad:
        ca = None
    rank, count = bad.get("shard", (0, 1))
    p = ptgpu.make_params(W, H, bad.get("samples", 16), flags=bad.get("flags", 0), shard_rank=rank, shard_count=count)
    if "params" in bad:
        p = None
    t = None
    if target and "target" not in bad:
        cls = ptgpu.AdaptiveTarget if target == "adaptive" else ptgpu.NoiseTarget
        t = cls(bad.get("rel_error", 0.1), bad.get("floor", 0.01), bad.get("max_fraction", 0.0),
                bad.get("min_samples", 4), bad.get("dilate", 1) if target == "adaptive" else 0)
    k = None
    if "iterations" in bad:
        k = ptgpu.denoise_defaults()
        k.iterations = bad["iterations"]
    img = None if "image" in bad else image
    if form == "ctx":
        args = [None, _ref(p)]
    else:
        args = [_vp(sp), len(sp), _vp(ca), _ref(p)]
        args += [-1] if form == "one" else [(C.c_int * 2)(0, 1), bad.get("n_devices", 2)]
    if target:
        args.append(_ref(t))
    if filtered:
        args.append(_ref(k))
    args.append(_vp(img))
    if target == "adaptive":
        args.append(None)  # sample counts
    if target:
        args.append(None)  # report
    status = getattr(L, entry)(*args)
    return int(status), L.ptg_last_error().decode()


def replay():
    """[entry, case, status, message] of every case, from the loaded library."""
    image = np.zeros((W * H, 3))
    rows = [[entry, name, *call(entry, bad, image)] for entry in DRIVERS for name, bad in cases_of(entry).items()]
    assert not image.any()  # nothing was added to the image
    return rows


def test_every_driver_answers_one_bad_argument_as_recorded():
    with open(GOLDEN) as f:
        want = json.load(f)
    got = replay()
    # the fixture holds exactly the cases above, each refused
    assert [r[:2] for r in want] == [r[:2] for r in got]
    # 10 drivers x 5 cases of any driver, 8 x 9 of a target, 4 x 2 of dilate, 6 x 2 of a filter, 5 without a
    # device, 5 NULL handles
    assert len({r[0] for r in want}) == 15 and len(want) == 50 + 72 + 8 + 12 + 5 + 5
    assert all(r[2] in (-1, -4) and r[3] for r in want)
    for w, g in zip(want, got):
        assert w == g, (w, g)


def test_messages_name_their_driver_or_its_shared_check():
    """What the recorded text says, so a fixture from a broken library cannot pass silently."""
    with open(GOLDEN) as f:
        rows = {(e, c): (s, m) for e, c, s, m in json.load(f)}
    assert rows[("ptg_render_to_noise", "floor_zero")] == (-1, "render_to_noise: floor must be > 0 and rel_error >= 0")
    # today's prefix under the filtered noise-target driver (pinned, not endorsed)
    assert rows[("ptg_render_to_noise_denoised", "max_fraction_one")] == \
        (-1, "render_to_noise: max_fraction must be in [0, 1)")
    assert rows[("ptg_render_adaptive_denoised_multi", "dilate_nine")] == \
        (-1, "render_adaptive_denoised_multi: dilate must be in [0, 8]")
    assert rows[("ptg_render_adaptive", "reference_f64")][0] == -4
    assert all("NULL" in m for (e, c), (s, m) in rows.items() if c.startswith("null_"))


if __name__ == "__main__":
    if "--record" not in sys.argv:
        sys.exit("usage: python tests/test_driver_errors_host.py --record")
    rows = replay()
    with open(GOLDEN, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
    print(f"wrote {GOLDEN}: {len(rows)} cases from {ptgpu.lib()._name}")
