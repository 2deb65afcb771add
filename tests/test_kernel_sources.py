"""The kernel-source hash covers every file of csrc/ that holds device code.

ptgpu.render.KERNEL_SOURCES names the files whose text ties a committed profile to a kernel
(kernel_source_hash()).  ptg_render.hip's device code lives in headers by topic; a header split off later and
not added to the list would drop kernel text from the hash unnoticed.  So every file of csrc/ whose text
contains __global__ or __device__ is either in the list or in NOT_HASHED below, with the reason.
"""
import os

import ptgpu
from ptgpu.render import KERNEL_SOURCES

CSRC = os.path.join(os.path.dirname(os.path.abspath(ptgpu.__file__)), os.pardir, "csrc")

# files with device code that the hash leaves out: none of them holds a timed kernel
NOT_HASHED = (
    ("ref64.hpp", "the reference-arithmetic kernel (PTG_FLAG_REFERENCE_F64): a checker, not timed"),
    ("follow_features.hpp", "the followed-feature kernel of the denoiser's guide: one untimed pass per frame"),
    ("sincos_cr.hpp", "the correctly rounded sin/cos of ref64.hpp's kernel"),
    ("ptg_denoise.hip", "the a-trous filter's translation unit: no render kernel"),
    ("denoise_filter.hpp", "the filter's arithmetic, shared with its CPU check"),
)


def _text(name):
    with open(os.path.join(CSRC, name), encoding="utf-8") as f:
        return f.read()


def _has_device_code(name):
    text = _text(name)
    return "__global__" in text or "__device__" in text


def test_every_file_with_device_code_is_hashed_or_excluded():
    excluded = [name for name, _ in NOT_HASHED]
    with_device_code = sorted(n for n in os.listdir(CSRC) if _has_device_code(n))
    assert with_device_code, "no device code found under csrc/"
    unlisted = [n for n in with_device_code if n not in KERNEL_SOURCES and n not in excluded]
    assert not unlisted, f"device code outside the kernel-source hash: {unlisted}"
    assert not set(excluded) & set(KERNEL_SOURCES)
    # an exclusion names a file that exists and still holds device code (else the entry is stale)
    assert [n for n in excluded if n not in with_device_code] == []
    assert all(reason for _, reason in NOT_HASHED)


def test_every_kernel_source_exists():
    assert len(set(KERNEL_SOURCES)) == len(KERNEL_SOURCES)
    missing = [n for n in KERNEL_SOURCES if not os.path.isfile(os.path.join(CSRC, n))]
    assert not missing
    assert ptgpu.kernel_source_hash() != "unavailable"


def test_ptg_render_hip_holds_no_device_code():
    """It stays in the hash for its launchers (block size, LDS bytes); the kernels are in the headers."""
    assert "ptg_render.hip" in KERNEL_SOURCES
    assert not _has_device_code("ptg_render.hip")
