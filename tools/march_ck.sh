# C3 kernel parity (march / nmarch tests) and a bench line
set -o pipefail
O=${OUT_DIR:-bench_out}/marchck
mkdir -p $O
timeout -k 10 600 python3 -u -m pytest -x -q --timeout 200 --timeout-method thread tests/test_gpu_march.py tests/test_gpu_pds.py > $O/tests.txt 2>&1 || { tail -30 $O/tests.txt; exit 1; }
tail -2 $O/tests.txt
timeout -k 10 600 python3 -u bench.py --full --steps 200 --warmup 20 --no-cpu-baseline > $O/bench.log 2>&1 || { tail -20 $O/bench.log; exit 2; }
python3 -c "
import json
d=json.loads(open('$O/bench.log').read().strip().splitlines()[-1])
print(d['value'], d['roofline']['kernel_ms'], d['roofline']['frac'])
"
