#!/usr/bin/env python3
"""Record tests/golden/fast_paths_no_glass.npz: radiance and segment counts of
4,096 seeded paths through the two scenes of tests/shade_direction_scenes.py
(no dielectric in either), from the trace kernel in the fast and in the exact
arithmetic mode.  tests/test_gpu_shade_directions.py compares later kernels
with it bit for bit, so it is recorded on the commit BEFORE a change to
shade() that may move refracting lanes only.

    python3 tools/gen_fast_path_pins.py [out.npz]      (on an MI355X)
    python3 tools/gen_fast_path_pins.py --check a.npz b.npz

Run it twice and --check the two files before committing one: the pins are
only worth having if the kernel reproduces itself.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "cpu-path-tracing_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def record(dst):
    import ptgpu
    import shade_direction_scenes as sd
    arrays = {"coords": sd.coords(), "kernel_hash": np.array(ptgpu.kernel_source_hash())}
    for name in sd.SCENES:
        for mode, (rad, segs) in sd.trace(name).items():
            arrays[f"{name}.{mode}.radiance"] = rad.view(np.uint32)  # bits, so that a NaN would compare too
            arrays[f"{name}.{mode}.segments"] = segs.astype(np.int32)
            print(f"{name} {mode}: mean segments {segs.mean():.2f}, mean radiance {rad.mean():.4f}, "
                  f"{int((rad.max(axis=1) > 0).sum())} lit paths")
    np.savez_compressed(dst, **arrays)
    print(f"wrote {dst}: {os.path.getsize(dst)} bytes, kernel {arrays['kernel_hash']}")


def check(a, b):
    A, B = np.load(a), np.load(b)
    bad = [k for k in sorted(set(A.files) | set(B.files))
           if k not in A.files or k not in B.files or A[k].tobytes() != B[k].tobytes()]
    print(f"{len(A.files)} arrays, {len(bad)} differ {bad}")
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1:2] == ["--check"]:
        sys.exit(check(sys.argv[2], sys.argv[3]))
    import shade_direction_scenes as sd
    record(sys.argv[1] if len(sys.argv) > 1 else sd.FIXTURE)
