"""Launch-plan invariants and values, and the scene fields the kernels are
given (cpu-path-tracing_amd/csrc/launch_plan.hpp, scene_prep.hpp), checked on
the CPU by tests/launch_plan_check.cpp built with AddressSanitizer + UBSan.

The program asserts, for a table of frames, shards and progressive passes,
what render_kernel relies on when it maps a unit to its level, pixel group and
samples (the kernels index the unit-level table without checks), and prints
every plan.  The plans, and the scan layout / box-mode fields and linear
upload table of the three built-in scenes, must equal
tests/golden/launch_plans.json, recorded before the host code moved out of
ptg_render.hip: a change of the plan's values is a deliberate act that
re-records the fixture (launch_plan_check --dump), never a side effect."""
import json
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("launch_plan") / "launch_plan_check"
    src = os.path.join(ROOT, "tests", "launch_plan_check.cpp")
    subprocess.check_call([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-g",
                           "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "include"), src, "-o", str(exe)])
    return str(exe)


def _run(exe, *args):
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


@pytest.mark.skipif(not shutil.which(HIPCC), reason="hipcc not present")
def test_launch_plan_invariants(check_exe):
    out = _run(check_exe)
    # the frames the kernel's A/B records are about, as the plan prints them
    assert "n9 1920x1080x1024: grid=38610 units=154440 levels=2" in out
    assert "n9 1920x1080x1024 shard 1/8: grid=18540 units=74160 levels=2 resolve_row0=66" in out
    assert "n10000 1920x1080x1024: grid=187560" in out
    assert "n10000 1920x1080x1024 shard 1/8: grid=150600 units=150600" in out
    assert "too many work units" in out
    # level kinds away from nsub 2 (tests/test_gpu_frame_shapes.py runs them on the GPU)
    assert "n9 128x96x8 nsub8: grid=17408 units=69632 levels=2 resolve_row0=32" in out
    assert "n9 128x95x8 nsub8: grid=6080 units=24320 levels=1" in out
    assert "n300 700x246x8 nsub3: grid=82000 units=82000 levels=2 resolve_row0=164" in out
    assert "n300 700x246x9 nsub3: grid=57400 units=57400 levels=2 resolve_row0=-1" in out


@pytest.mark.skipif(not shutil.which(HIPCC), reason="hipcc not present")
def test_launch_plans_match_the_recorded_ones(check_exe):
    got = json.loads(_run(check_exe, "--dump"))
    with open(os.path.join(ROOT, "tests", "golden", "launch_plans.json")) as f:
        want = json.load(f)
    assert [p["name"] for p in got["plans"]] == [p["name"] for p in want["plans"]]
    for g, w in zip(got["plans"], want["plans"]):
        assert g == w, g["name"]
    assert [s["name"] for s in got["scenes"]] == [s["name"] for s in want["scenes"]]
    for g, w in zip(got["scenes"], want["scenes"]):
        assert g == w, g["name"]
