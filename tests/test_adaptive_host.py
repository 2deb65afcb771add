"""Host side of adaptive sampling (no GPU): the structs and declarations of
include/ptgpu.h against the ctypes bindings, the argument checks that run
before any device call, plan_active's invariants (tests/active_plan_check.cpp,
built with AddressSanitizer + UBSan) and the identity the per-pixel sample
offset rests on: sample_state(key + b G, s) == sample_state(key, b + s)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ptgpu
from conftest import ROOT

INVALID, NO_DEVICE, UNSUPPORTED = -1, -3, -4
HIPCC = "/opt/rocm/bin/hipcc"
NEW = ("ptg_set_active_mask_device", "ptg_select_active_device", "ptg_accumulate_active_device",
       "ptg_resolve_active_device", "ptg_read_sample_counts_device", "ptg_render_adaptive")


def _header():
    with open(os.path.join(ROOT, "include", "ptgpu.h")) as f:
        return f.read()


def test_header_declares_the_entry_points_and_the_abi_version_stays():
    text = _header()
    for name in NEW:
        assert re.search(rf"^int {name}\(", text, re.M), name  # (tests/test_host.py parses declarations this way)
        assert name in ptgpu.EXPORTS and hasattr(ptgpu.lib(), name)
    assert int(re.search(r"#define PTG_ABI_VERSION (\d+)", text).group(1)) == 2 == ptgpu.ABI_VERSION  # additive
    # a new struct: the old target's reserved_ keeps no meaning
    assert re.search(r"int32_t reserved_;\s*\} ptg_noise_target;", text)
    assert re.search(r"int32_t dilate;[^}]*\} ptg_adaptive_target;", text)


@pytest.fixture(scope="module")
def check_out(tmp_path_factory):
    if not shutil.which(HIPCC):
        pytest.skip("hipcc not present")
    exe = tmp_path_factory.mktemp("active_plan") / "active_plan_check"
    src = os.path.join(ROOT, "tests", "active_plan_check.cpp")
    subprocess.check_call([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-g",
                           "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "include"), src, "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


def test_plan_active_invariants(check_out):
    m = re.search(r"^plans ok (\d+), refused \(too many work units\) (\d+), failures 0$", check_out, re.M)
    assert m, check_out
    # 2 kernels x 5 unit counts x 4 chunk settings x 65536 adds, less the empty plans (units 0), plus the extras
    assert int(m.group(1)) + int(m.group(2)) == 2 * 4 * 4 * 65536 + 2 * 2
    assert int(m.group(2)) > 0  # 2^28 units in chunks of 1: computed in 64 bits and refused


def test_struct_layouts_match_the_header(check_out):
    def layout(struct, cname):
        m = re.search(rf"^{cname} size (\d+) (.*)$", check_out, re.M)
        words = m.group(2).split()
        want = {"size": int(m.group(1)), **{k: int(v) for k, v in zip(words[::2], words[1::2])}}
        got = {"size": C.sizeof(struct), **{k: getattr(struct, k).offset for k in want if k != "size"}}
        assert got == want, cname
    layout(ptgpu.AdaptiveTarget, "ptg_adaptive_target")
    layout(ptgpu.AdaptiveReport, "ptg_adaptive_report")
    assert len(ptgpu.AdaptiveReport().pass_active) == len(ptgpu.NoiseReport().pass_over)  # PTG_NOISE_MAX_PASSES


def _call(sp, ca, p, target, img, counts=None, rep=None):
    vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
    return ptgpu.lib().ptg_render_adaptive(vp(sp), len(sp) if sp is not None else 0, vp(ca),
                                           C.byref(p) if p else None, -1, C.byref(target) if target else None,
                                           vp(img), vp(counts), C.byref(rep) if rep else None)


def test_render_adaptive_argument_checks():
    L = ptgpu.lib()
    scn = ptgpu.box_scene(8, 8)
    cam = ptgpu.camera.with_config(scn.camera_parameters)
    sp, ca = scn.to_array(), cam.to_array()
    img = np.zeros((64, 3))
    p = ptgpu.make_params(8, 8, 16)
    ok = lambda **kw: ptgpu.AdaptiveTarget(kw.get("rel_error", 0.1), kw.get("floor", 0.01),  # noqa: E731
                                           kw.get("max_fraction", 0.0), kw.get("min_samples", 4), kw.get("dilate", 1))
    cases = [
        ((sp, ca, p, ok(), None), b"NULL"),
        ((sp, ca, p, None, img), b"NULL"),
        ((sp, ca, None, ok(), img), b"params is NULL"),
        ((sp, None, p, ok(), img), b"NULL"),
        ((sp, ca, p, ok(floor=0.0), img), b"floor"),
        ((sp, ca, p, ok(floor=float("nan")), img), b"floor"),
        ((sp, ca, p, ok(rel_error=-0.5), img), b"rel_error"),
        ((sp, ca, p, ok(max_fraction=1.0), img), b"max_fraction"),
        ((sp, ca, p, ok(max_fraction=float("nan")), img), b"max_fraction"),
        ((sp, ca, p, ok(dilate=-1), img), b"dilate"),
        ((sp, ca, p, ok(dilate=9), img), b"dilate"),
        ((sp, ca, ptgpu.make_params(8, 8, 16, shard_rank=1, shard_count=2), ok(), img), b"shard_count"),
        ((sp, ca, p, ok(min_samples=1), img), b">= 2"),
        ((sp, ca, ptgpu.make_params(8, 8, 1), ok(), img), b">= 2"),
    ]
    for args, msg in cases:
        assert _call(*args) == INVALID, msg
        assert msg in L.ptg_last_error(), (msg, L.ptg_last_error())
    p64 = ptgpu.make_params(8, 8, 16, flags=ptgpu.FLAG_REFERENCE_F64)
    assert _call(sp, ca, p64, ok(), img) == UNSUPPORTED and b"fp32 only" in L.ptg_last_error()
    n = C.c_int(0)
    L.ptg_device_count(C.byref(n))
    if n.value == 0:  # the CPU container: valid arguments reach the device and come back cleanly
        counts = np.full((8, 8), -5, dtype=np.int32)
        rep = ptgpu.AdaptiveReport()
        assert _call(sp, ca, p, ok(), img, counts, rep) == NO_DEVICE
        assert (counts == -5).all() and rep.passes == 0
        with pytest.raises(ptgpu.PtgError, match=r"\(-3\)"):
            ptgpu.render_adaptive(scn, cam, img, 8, 8, 16, rel_error=0.1)
    assert not img.any()  # nothing was added to the image
    with pytest.raises(ValueError):
        ptgpu.render_adaptive(scn, cam, np.zeros((10, 3)), 8, 8, 16, rel_error=0.1)


def test_device_entry_points_refuse_null_arguments_without_gpu_work():
    L = ptgpu.lib()
    p = ptgpu.make_params(8, 8, 16)
    P = C.byref(p)
    one = C.c_void_p(8)  # a non-NULL context that is never dereferenced: params NULL is refused first
    assert L.ptg_set_active_mask_device(None, P, None, None, None) == INVALID and b"NULL" in L.ptg_last_error()
    assert L.ptg_select_active_device(None, P, 0.1, 0.01, 0, None, None, None) == INVALID
    assert L.ptg_accumulate_active_device(None, P, 1, 0, None, None) == INVALID
    assert L.ptg_resolve_active_device(None, P, None, None) == INVALID
    assert L.ptg_read_sample_counts_device(None, P, None, None) == INVALID
    for call in (lambda: L.ptg_set_active_mask_device(one, None, None, None, None),
                 lambda: L.ptg_select_active_device(one, None, 0.1, 0.01, 0, None, None, None),
                 lambda: L.ptg_accumulate_active_device(one, None, 1, 0, None, None)):
        assert call() == INVALID and b"params is NULL" in L.ptg_last_error()
    # checked before the context is used: the ranges of select_active and accumulate_active
    assert L.ptg_select_active_device(one, P, 0.1, 0.01, 9, None, None, None) == INVALID
    assert b"dilate" in L.ptg_last_error()
    assert L.ptg_select_active_device(one, P, 0.1, 0.0, 0, None, None, None) == INVALID and b"floor" in L.ptg_last_error()
    sh = ptgpu.make_params(8, 8, 16, shard_rank=1, shard_count=2)
    assert L.ptg_select_active_device(one, C.byref(sh), 0.1, 0.01, 1, None, None, None) == UNSUPPORTED
    assert b"other shards" in L.ptg_last_error()
    assert L.ptg_accumulate_active_device(one, P, -1, 0, None, None) == INVALID and b"add_samples" in L.ptg_last_error()


# ---- the key identity ---------------------------------------------------------------------
G = np.uint64(0x9E3779B97F4A7C15)


def _mix64(z):  # pt_device.hpp mix64, mod 2^64
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def _sample_state(key, s):  # pt_device.hpp sample_state
    st = (_mix64(key + (s.astype(np.uint64) + np.uint64(1)) * G) >> np.uint64(32)).astype(np.uint32)
    return np.where(st != 0, st, np.uint32(0x6D2B79F5))


def test_shifting_the_key_shifts_the_sample_index():
    rng = np.random.default_rng(7)
    n = 200000
    key = rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    total = rng.integers(0, 2 ** 31, n, dtype=np.uint64)  # b + s < 2^31
    b = (rng.random(n) * (total + np.uint64(1))).astype(np.uint64)
    b = np.minimum(b, total)
    s = total - b
    for bb, ss in ((b, s), (total, np.zeros_like(s)), (np.zeros_like(b), total)):
        with np.errstate(over="ignore"):
            shifted = _sample_state(key + bb * G, ss)
            plain = _sample_state(key, bb + ss)
        assert np.array_equal(shifted, plain)
    with np.errstate(over="ignore"):
        assert int(_sample_state(np.uint64(0), np.uint64(0))) == int(_mix64(G) >> np.uint64(32))
