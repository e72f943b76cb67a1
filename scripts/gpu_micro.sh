#!/bin/bash
# GPU tests, the microbenchmarks and (PMC="<counters>") one counter pass over
# the full bench.  Output goes to $OUT (default bench_out/ in the repository root).
set -u
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
R="$(pwd)"
O="$R/${OUT:-bench_out}"; mkdir -p "$O"
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q -p no:cacheprovider --timeout 120 --timeout-method thread > "$O/pytest_gpu.log" 2>&1
rc=$?; echo "pytest_gpu rc=$rc"; tail -3 "$O/pytest_gpu.log"
if [ $rc -ne 0 ]; then exit $rc; fi
timeout -k 10 600 python scripts/microbench.py > "$O/micro.jsonl" 2> "$O/micro.err"
rc=$?; echo "micro rc=$rc"; cat "$O/micro.jsonl"; tail -3 "$O/micro.err"
if [ $rc -ne 0 ]; then exit $rc; fi
if [ -n "${PMC:-}" ]; then
  cd /tmp && export TMPDIR=/tmp
  timeout -k 10 600 rocprofv3 --pmc $PMC -d "$O/pmc" -o pmc --output-format csv -- python "$R/bench.py" --full --steps 10 --warmup 2 --no-cpu-baseline > "$O/pmc_bench.json" 2> "$O/pmc.err"
  rc=$?; echo "pmc rc=$rc"; tail -2 "$O/pmc.err"
fi
exit $rc
