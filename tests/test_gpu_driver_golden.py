"""The twelve whole-frame drivers keep their images, sample counts and reports, bit for bit.

The drivers share one noise-target loop and one adaptive loop (csrc/frame_passes.hpp); before that each wrote its
own.  tests/golden/driver_frames.npz holds what the library of the commit before the loops were shared gave on an
MI355X (tools/build_prev.sh, then `PTGPU_LIB=.../build/libptgpu_prev.so python tests/test_gpu_driver_golden.py
--record` writes the file from whatever library is loaded).

Frame: box, 24x10, 2x2 sub-pixels, 16 samples, min_samples 4 (pass ends 4, 8, 16), band_rows 4 -- H is no multiple
of the band, so slab rows 10 and 11 lie past the image.  The ptg_multi_* forms run on a MultiContext of 3 local
shards (uneven: 2, 1 and 0 bands of image rows).  Both arithmetic modes.  Targets (floor 0.01, so rho <= 50):

  a  rel_error 100                    the first check converges: 1 pass
  b  rel_error 0, max_fraction 0      never converges: 3 passes
  c  a rel_error and a max_fraction   the recorder picked so that the library it recorded stopped after pass 2
     (kept in the fixture: noise 1.5335, 2.5 / 240 pixels; adaptive 1.0024, 16.5 / 240)

The adaptive drivers run a and b with dilate 1, c with dilate 0; one adaptive frame per form runs with
FLAG_COUNT_TESTS for report.counters.  Compared exactly: the image (added into a non-zero one), the sample counts,
the report's bytes.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

if __name__ == "__main__":  # --record: the paths tests/conftest.py sets
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(_root, "cpu-path-tracing_amd"))

import ptgpu  # noqa: E402
from ptgpu._abi import check  # noqa: E402
from test_driver_errors_host import DRIVERS  # noqa: E402  (entry point -> form, target, filtered)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "driver_frames.npz")
W, H, SAMPLES, MIN_SAMPLES, BAND_ROWS, SHARDS = 24, 10, 16, 4, 4, 3
FLOOR = 0.01
MODES = {"fast": 0, "exact": ptgpu.FLAG_EXACT_MATH}
# five on one device, five on a MultiContext, two of the one-shot forms (devices = [0])
TWELVE = [e for e, (form, _, _) in DRIVERS.items() if form != "shot"] + \
    ["ptg_render_to_noise_multi", "ptg_render_adaptive_denoised_multi"]
COUNTED = ["ptg_render_adaptive", "ptg_multi_render_adaptive_denoised"]  # with FLAG_COUNT_TESTS, target c


def _require_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a visible MI355X")


def _scene():
    scn = ptgpu.box_scene(W, H)
    return scn, ptgpu.camera.with_config(scn.camera_parameters)


def _start():
    """The image the drivers add into: non-zero, different in every value."""
    return 0.25 + np.arange(W * H * 3, dtype=np.float64).reshape(H, W, 3) / 1024.0


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def run(entry, flags, target, multi=None):
    """One frame of `entry`: (image, counts or None, the report's bytes or None).  target: None or (rel_error,
    max_fraction, dilate); multi: the MultiContext of the ptg_multi_* forms."""
    form, kind, filtered = DRIVERS[entry]
    scn, cam = _scene()
    sp, ca = scn.to_array(), cam.to_array()
    p = ptgpu.make_params(W, H, SAMPLES, 2, band_rows=BAND_ROWS, flags=flags)
    image = _start()
    counts = np.full((H, W), -1, dtype=np.int32) if kind == "adaptive" else None
    rep = {"noise": ptgpu.NoiseReport, "adaptive": ptgpu.AdaptiveReport, None: lambda: None}[kind]()
    if form == "ctx":
        args = [multi._h, C.byref(p)]
    else:
        args = [_vp(sp), len(sp), _vp(ca), C.byref(p)] + ([0] if form == "one" else [(C.c_int * 1)(0), 1])
    if kind:
        rel_error, max_fraction, dilate = target
        cls = ptgpu.AdaptiveTarget if kind == "adaptive" else ptgpu.NoiseTarget
        args.append(C.byref(cls(rel_error, FLOOR, max_fraction, MIN_SAMPLES, dilate if kind == "adaptive" else 0)))
    if filtered:
        args.append(None)  # the default filter, the camera's pixel_spread
    args.append(_vp(image))
    if kind == "adaptive":
        args.append(_vp(counts))
    if kind:
        args.append(C.byref(rep))
    check(getattr(ptgpu.lib(), entry)(*args), entry)
    return image, counts, (np.frombuffer(bytes(rep), dtype=np.uint8) if kind else None)


def targets_of(entry, mode, pick_c):
    """name -> target of the frames of `entry`; pick_c(kind, mode): target c's (rel_error, max_fraction)."""
    kind = DRIVERS[entry][1]
    if kind is None:
        return {"plain": None}
    return {"a": (100.0, 0.0, 1), "b": (0.0, 0.0, 1), "c": (*pick_c(kind, mode), 0)}


def frames(entry, mode, pick_c, multi):
    """key -> array of every frame of (entry, mode), from the loaded library."""
    out = {}
    todo = [(name, MODES[mode], t) for name, t in targets_of(entry, mode, pick_c).items()]
    if entry in COUNTED and mode == "fast":
        todo.append(("c_counted", ptgpu.FLAG_COUNT_TESTS, (*pick_c(DRIVERS[entry][1], mode), 0)))
    for name, flags, t in todo:
        image, counts, rep = run(entry, flags, t, multi)
        out[f"{entry}/{mode}/{name}/image"] = image
        if counts is not None:
            out[f"{entry}/{mode}/{name}/counts"] = counts
        if rep is not None:
            out[f"{entry}/{mode}/{name}/report"] = rep
    return out


_golden_cache = {}


def _golden():
    if not _golden_cache:
        with np.load(GOLDEN) as z:
            _golden_cache.update({k: z[k] for k in z.files})
    return _golden_cache


@pytest.fixture(scope="module")
def multi():
    _require_gpu()
    with ptgpu.MultiContext(*_scene(), [0], local_shards=SHARDS) as m:
        yield m


def _report(entry, raw):
    cls = ptgpu.AdaptiveReport if DRIVERS[entry][1] == "adaptive" else ptgpu.NoiseReport
    return cls.from_buffer_copy(raw.tobytes())


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("entry", TWELVE)
def test_driver_keeps_its_frames(entry, mode, multi):
    want = _golden()
    got = frames(entry, mode, lambda kind, m: tuple(float(v) for v in want[f"c/{kind}/{m}"]), multi)
    mine = sorted(k for k in want if k.startswith(f"{entry}/{mode}/"))
    assert mine and mine == sorted(got)
    for key in mine:
        g, w = got[key], want[key]
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), key
    # what the recorded frames are, so a fixture from a broken library cannot pass silently
    for name in targets_of(entry, mode, lambda *a: (0.0, 0.0)):
        assert not np.array_equal(want[f"{entry}/{mode}/{name}/image"], _start())
        if name == "plain":
            continue
        rep = _report(entry, want[f"{entry}/{mode}/{name}/report"])
        assert (rep.passes, rep.converged) == {"a": (1, 1), "b": (3, 0), "c": (2, 1)}[name]
        assert rep.pixels == W * H
        if DRIVERS[entry][1] == "adaptive":
            counts = want[f"{entry}/{mode}/{name}/counts"]
            assert counts.min() >= MIN_SAMPLES and counts.max() == rep.max_samples == (4, 16, 8)["abc".index(name)]
            assert rep.total_samples == counts.sum()
    if entry in COUNTED and mode == "fast":
        assert _report(entry, want[f"{entry}/{mode}/c_counted/report"]).counters[0] > 0
        assert not any(_report(entry, want[f"{entry}/{mode}/c/report"]).counters)


def record():
    """Picks target c per loop and mode and writes every frame.  Target c: the loaded library runs with
    max_fraction 0 over a geometric ladder of rel_error; the rel_error at which the pixels over the target drop
    the most from pass 1 to pass 2 is taken, with the max_fraction that lies between the two counts -- pass 1
    misses it, pass 2 meets it.  (In the box scene most pixels' rho grows with the first samples, so the counts
    drop only where the last few pixels are over: a second, fine ladder covers those values.)"""
    chosen = {}

    def pick_c(kind, mode):
        if (kind, mode) not in chosen:
            entry = "ptg_render_adaptive" if kind == "adaptive" else "ptg_render_to_noise"
            # some, none: the largest rel_error with a pixel over after pass 1, the least without
            best, some, none = None, 0.02, 20.0
            for ladder in ("coarse", "fine"):
                for rel in np.geomspace(0.02, 20.0, 31) if ladder == "coarse" else np.geomspace(some / 2, none, 300):
                    rep = _report(entry, run(entry, MODES[mode], (float(rel), 0.0, 0))[2])
                    over = list(rep.pass_over[:rep.passes])
                    if ladder == "coarse":
                        some, none = (max(some, rel), none) if over[0] else (some, min(none, rel))
                    if rep.passes >= 2 and over[0] - over[1] > (best[0] if best else 0):
                        best = (over[0] - over[1], float(rel), (over[1] + 0.5) / (W * H), over)
                if best:
                    break
            if best is None:
                sys.exit(f"no rel_error at which fewer pixels are over after pass 2 ({kind}, {mode})")
            print(f"{kind} {mode}: rel_error {best[1]!r}, max_fraction {best[2]!r}, over {best[3]}")
            chosen[(kind, mode)] = best[1:3]
        return chosen[(kind, mode)]

    arrays = {}
    with ptgpu.MultiContext(*_scene(), [0], local_shards=SHARDS) as m:
        for entry in TWELVE:
            for mode in MODES:
                arrays.update(frames(entry, mode, pick_c, m))
    for (kind, mode), c in chosen.items():
        arrays[f"c/{kind}/{mode}"] = np.array(c, dtype=np.float64)  # rel_error, max_fraction
    np.savez_compressed(GOLDEN, **arrays)
    print(f"wrote {GOLDEN}: {len(arrays)} arrays, target c {chosen}, from {ptgpu.lib()._name}")


if __name__ == "__main__":
    if "--record" not in sys.argv:
        sys.exit("usage: python tests/test_gpu_driver_golden.py --record")
    record()
