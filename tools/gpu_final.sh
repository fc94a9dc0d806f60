#!/bin/bash
# round-end evidence: full -m gpu suite, the full bench line (bench.py --full: median of 3 runs,
# roofline, CPU baseline), the rocprofv3 kernel-stats profile of a plain bench run, side benches:
# tools/gpu_final.sh <tag>   (output under $OUT, default out/)
set -o pipefail
TAG=${1:-final}
cd "$(dirname "$0")/.." || exit 1
OUT=${OUT:-out}
mkdir -p "$OUT"
export TMPDIR=${TMPDIR:-/tmp}
timeout -k 10 900 python -u -m pytest tests -m gpu -q --timeout 300 --timeout-method thread > "$OUT"/${TAG}_pytest.log 2>&1
rc=$?
tail -2 "$OUT"/${TAG}_pytest.log
if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then exit $rc; fi
timeout -k 10 600 python -u bench.py --full > "$OUT"/${TAG}_bench.json 2> "$OUT"/${TAG}_bench.err || { tail -20 "$OUT"/${TAG}_bench.err; exit 1; }
cat "$OUT"/${TAG}_bench.json
timeout -k 10 300 rocprofv3 --kernel-trace --stats -f csv -d "$OUT"/${TAG}_prof -o prof -- python3 bench.py --steps 20 --warmup 5 > "$OUT"/${TAG}_prof_bench.json 2> "$OUT"/${TAG}_prof.err || { tail -20 "$OUT"/${TAG}_prof.err; exit 1; }
timeout -k 10 300 python3 bench.py --full --model centernet --steps 20 --warmup 5 > "$OUT"/${TAG}_cn.json 2>/dev/null || exit 1
timeout -k 10 300 python3 bench.py --full --model retinanet --steps 20 --warmup 5 > "$OUT"/${TAG}_rn.json 2>/dev/null || exit 1
timeout -k 10 300 python3 -c "import __graft_entry__ as g; g.smoke()" > "$OUT"/${TAG}_smoke.log 2>&1 || { tail -20 "$OUT"/${TAG}_smoke.log; exit 1; }
tail -1 "$OUT"/${TAG}_smoke.log
exit $rc
