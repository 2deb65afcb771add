#!/usr/bin/env bash
# End-to-end check of HEAD on a machine with one MI355X: the -m gpu suite,
# __graft_entry__.smoke(), the full bench line (N = 1, CPU baseline included:
# bench.py --full) and the 1-GPU rehearsal of the one-process N > 1 path.
# Logs and lines go to $OUT_DIR (default: out/).
# Usage: bash tools/gpu_check.sh <tag>
tag=${1:-final}
out=${OUT_DIR:-out}
mkdir -p "$out"
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread \
    > "$out/${tag}_pytest.log" 2>&1
rc=$?; echo "pytest rc=$rc"; tail -3 "$out/${tag}_pytest.log"; [ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > "$out/${tag}_smoke.log" 2>&1 \
  || { echo SMOKE FAILED; tail -20 "$out/${tag}_smoke.log"; exit 1; }
tail -1 "$out/${tag}_smoke.log"
timeout -k 10 300 python bench.py --full > "$out/${tag}_bench.json" 2> "$out/${tag}_bench.err" \
  || { echo BENCH FAILED; tail "$out/${tag}_bench.err"; exit 1; }
cut -c1-400 "$out/${tag}_bench.json"
PTG_REHEARSAL=1 timeout -k 10 300 python bench.py --full --gpus 8 --steps 2 --warmup 1 --t1-steps 1 \
  > "$out/${tag}_rehearse8_inprocess.json" 2> "$out/${tag}_rehearse8_inprocess.err" \
  || { echo REHEARSAL8 FAILED; tail "$out/${tag}_rehearse8_inprocess.err"; exit 1; }
cut -c1-300 "$out/${tag}_rehearse8_inprocess.json"
echo done
