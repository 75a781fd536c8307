#!/bin/bash
# Checkpoint: GPU tests, the full bench line, kernel-trace stats of the bench ($1: directory under ${OUT_DIR:-bench_out})
set -o pipefail
export TMPDIR=/tmp
O=${OUT_DIR:-bench_out}/${1:-ck}
mkdir -p $O
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > $O/gpu_tests.txt 2>&1 || { echo TESTS_FAILED; tail -30 $O/gpu_tests.txt; exit 1; }
tail -3 $O/gpu_tests.txt
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > $O/smoke.txt 2>&1 || { echo SMOKE_FAILED; tail -20 $O/smoke.txt; exit 4; }
tail -1 $O/smoke.txt
timeout -k 10 600 python -u bench.py --full --steps 200 --warmup 20 > $O/bench.log 2>&1 || { echo BENCH_FAILED; tail -30 $O/bench.log; exit 2; }
tail -1 $O/bench.log
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $O/prof -o run --output-format csv -- python3 bench.py --full --steps 200 --warmup 20 --no-cpu-baseline > $O/prof.log 2>&1 || { echo PROF_FAILED; tail -20 $O/prof.log; exit 3; }
# the per-dispatch trace is tens of MB: keep the stats
find $O/prof \( -name '*kernel_trace.csv' -o -name '*agent_info.csv' \) -delete
echo ALL_OK
