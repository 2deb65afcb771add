#!/usr/bin/env bash
# Final check of HEAD on a machine with one MI355X: the -m gpu suite and
# profiles (tools/gpu_suite_profile.sh), then __graft_entry__.smoke() and the
# full bench line (N = 1, CPU baseline included: bench.py --full).  The smoke
# log and the line go to $OUT_DIR (default: out/).
# Usage: bash tools/gpu_final.sh <tag>
tag=${1:-final}
out=${OUT_DIR:-out}
bash tools/gpu_suite_profile.sh $tag || exit 1
mkdir -p "$out"
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > "$out/${tag}_smoke.log" 2>&1 \
  || { echo SMOKE FAILED; tail -20 "$out/${tag}_smoke.log"; exit 1; }
tail -1 "$out/${tag}_smoke.log"
timeout -k 10 300 python bench.py --full > "$out/${tag}_bench.json" 2> "$out/${tag}_bench.err" \
  || { echo BENCH FAILED; tail "$out/${tag}_bench.err"; exit 1; }
cut -c1-600 "$out/${tag}_bench.json"
