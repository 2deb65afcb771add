"""csrc/sobol_pairs.hpp, PTG_FLAG_STRATIFIED's sampler, on the host
(tests/sobol_check.cpp): P(i) against the second Sobol' dimension formed bit
by bit, the (0,2) property of the scrambled, shuffled pairs for every block
size 2..256 over 64 keys and all four pair numbers, and that different pair
numbers give different points.  The program is also built with
-fsanitize=address,undefined and run on its own.  Its printed vectors are what
the numpy restatement (tests/strat_ref.py) must reproduce to the bit.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import strat_ref
from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "sobol_check.cpp")


def _run(tmp_path, name, extra):
    exe = tmp_path / name
    subprocess.check_call(["g++", "-std=c++17", "-O2", *extra, SRC, "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[:2000] + r.stderr[:2000]
    lines = r.stdout.splitlines()
    print(lines[0])
    w = lines[0].split()
    assert w[0::2] == ["P_mismatches", "cells_off", "out_of_range", "equal_pairs", "blocks"]
    assert [int(v) for v in w[1:8:2]] == [0, 0, 0, 0]
    # 64 keys x 2 sample ranges x 4 pairs x sum over m of (1024 / 2^m) blocks x (m + 1) shapes
    assert int(w[9]) == 64 * 2 * 4 * sum((1024 >> m) * (m + 1) for m in range(1, 9))
    return [[int(v) for v in ln.split()[1:]] for ln in lines[1:] if ln.startswith("vec ")]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_host_check_and_the_numpy_restatement(tmp_path):
    vec = np.array(_run(tmp_path, "sobol_check", []), dtype=np.uint64)
    assert len(vec) == 2 * 3 * 4 * 6
    seed, ps, j, s = vec[:, 0], vec[:, 1], vec[:, 2].astype(int), vec[:, 3]
    key = np.array([strat_ref.key_hash(int(a), int(b)) for a, b in zip(seed, ps)], dtype=np.uint64)
    got = strat_ref.pairs_of_keys(key, s.astype(np.uint32))[np.arange(len(vec)), j]
    assert np.array_equal(got, vec[:, 4:6].astype(np.uint32))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_host_check_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    _run(tmp_path, "sobol_check_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def test_numpy_P_is_the_second_sobol_dimension_reversed():
    i = np.concatenate([np.arange(1 << 12, dtype=np.uint32),
                        (np.arange(1 << 12, dtype=np.uint64) * 2654435761 % (1 << 32)).astype(np.uint32)])
    assert np.array_equal(strat_ref.P(i), strat_ref.brev(strat_ref.sobol_dim2(i)))


def test_numpy_pairs_are_a_02_sequence():
    key = strat_ref.key_hash(7, np.arange(32) * 31)
    s = np.arange(256, dtype=np.uint32)
    q = np.stack([strat_ref.pairs_of_keys(key, np.full(len(key), v)) for v in s], axis=-1)  # [key, pair, 2, sample]
    assert strat_ref.is_02_sequence(q[:, :, 0, :], q[:, :, 1, :])
    # plain xorshift draws are not: the check can fail
    rng = np.random.default_rng(1)
    assert not strat_ref.is_02_sequence(rng.integers(0, 1 << 24, 256), rng.integers(0, 1 << 24, 256))
