#!/usr/bin/env bash
# Build the committed (HEAD or $1) library as build/libptgpu_${2:-prev}.so for same-box A/B runs and for
# recording fixtures from a parent commit (PTGPU_LIB=build/libptgpu_prev.so): every source that revision's
# Makefile links, with the Makefile's flags.
set -e
rev=${1:-HEAD}
root=$(git rev-parse --show-toplevel)
tmp=$(mktemp -d)
git -C "$root" archive "$rev" cpu-path-tracing_amd/csrc include | tar -x -C "$tmp"
mkdir -p "$root/cpu-path-tracing_amd/build"
name=${2:-prev}
# every .hip and .cpp under csrc/ is a translation unit of the library (the Makefile's link lines)
srcs=$(ls "$tmp"/cpu-path-tracing_amd/csrc/*.hip "$tmp"/cpu-path-tracing_amd/csrc/*.cpp 2>/dev/null)
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-slp-vectorize -shared \
    -o "$root/cpu-path-tracing_amd/build/libptgpu_$name.so" $srcs -L/opt/rocm/lib -lrccl -Wl,-rpath,/opt/rocm/lib
rm -rf "$tmp"
echo "built build/libptgpu_$name.so from $rev"
