#!/usr/bin/env python3
"""Compare two device assembly listings kernel by kernel.

    hipcc <the Makefile's HIPFLAGS> --offload-device-only -S -o old.s csrc/ptg_render.hip   (old tree)
    hipcc <the Makefile's HIPFLAGS> --offload-device-only -S -o new.s csrc/ptg_render.hip   (new tree)
    tools/isa_diff.py old.s new.s

For every function symbol of either listing: its instruction count in both
and whether the bodies (label to .Lfunc_end; comments, the compilation unit
id, the function ordinal in block labels and the kernarg size stripped) are
identical.  Exit status 1 when a kernel of the old
listing is missing from or differs in the new one.
"""
import re
import sys


def bodies(path):
    out, name, buf = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+|\w+):\s*(;.*)?$", line)
        if name is None and m and not line.startswith(".L"):
            name, buf = m.group(1), []
            continue
        if name is not None:
            if line.startswith(".Lfunc_end"):
                out[name] = buf
                name = None
                continue
            text = line.split(";")[0].rstrip()
            text = re.sub(r"__hip_cuid_\w+", "__hip_cuid", text)
            # block labels carry the function's ordinal in the file; the kernarg size is metadata
            text = re.sub(r"\.LBB\d+_", ".LBB_", text)
            text = re.sub(r"(\.amdhsa_kernarg_size) \d+", r"\1 N", text)
            if text.strip():
                buf.append(text)
    return out


def main():
    old, new = bodies(sys.argv[1]), bodies(sys.argv[2])
    bad = 0
    for name in sorted(set(old) | set(new)):
        a, b = old.get(name), new.get(name)
        n = lambda t: sum(1 for x in t if x.startswith("\t") and not x.lstrip().startswith(".")) if t else 0
        if a is None:
            state = "new"
        elif b is None:
            state, bad = "MISSING", bad + 1
        elif a == b:
            state = "identical"
        else:
            state, bad = "DIFFERS", bad + 1
        print(f"{state:10s} old {n(a):6d} new {n(b):6d}  {name}")
    print(f"{len(old)} old symbols, {len(new)} new symbols, {bad} missing or different")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
