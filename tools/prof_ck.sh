set -o pipefail
export TMPDIR=/tmp
O=${OUT_DIR:-bench_out}/profck
mkdir -p $O
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d $O/prof -o run --output-format csv -- python3 bench.py --full --steps 200 --warmup 20 --no-cpu-baseline > $O/prof.log 2>&1 || { echo PROF_FAILED; tail -20 $O/prof.log; exit 3; }
find $O/prof \( -name '*kernel_trace.csv' -o -name '*agent_info.csv' \) -delete
find $O -type f | head
