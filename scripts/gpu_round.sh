#!/bin/bash
# One GPU-box session: tests, smoke, short full bench, rocprof kernel stats.
# Stops at the first crash/timeout (exit codes other than 0/1 from pytest).
# Output goes to $OUT (default bench_out/ in the repository root).
set -u
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
R="$(pwd)"
O="$R/${OUT:-bench_out}"; mkdir -p "$O"
STEPS=${STEPS:-50}
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q -p no:cacheprovider --timeout 120 --timeout-method thread > "$O/pytest_gpu.log" 2>&1
rc=$?
echo "pytest_gpu rc=$rc"; tail -5 "$O/pytest_gpu.log"
if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then echo "stopping after pytest rc=$rc"; exit $rc; fi
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > "$O/smoke.log" 2>&1
rc=$?; echo "smoke rc=$rc"; tail -3 "$O/smoke.log"
if [ $rc -ne 0 ]; then exit $rc; fi
timeout -k 10 600 python bench.py --full --steps "$STEPS" --warmup 10 > "$O/bench.json" 2> "$O/bench.err"
rc=$?; echo "bench rc=$rc"; cat "$O/bench.json"; tail -3 "$O/bench.err"
if [ $rc -ne 0 ]; then exit $rc; fi
if [ "${PROFILE:-1}" = "1" ]; then
  cd /tmp && export TMPDIR=/tmp
  timeout -k 10 600 rocprofv3 --kernel-trace --stats -d "$O/prof" -o run --output-format csv -- python "$R/bench.py" --full --steps "$STEPS" --warmup 10 --no-cpu-baseline --extra "" > "$O/bench_prof.json" 2> "$O/bench_prof.err"
  rc=$?; echo "rocprof rc=$rc"
  find "$O/prof" -name "*stats*" | head
  if [ $rc -ne 0 ]; then exit $rc; fi
fi
if [ "${TORCHRUN:-0}" = "1" ]; then
  cd "$R"
  timeout -k 10 300 python -m torch.distributed.run --nnodes=1 --nproc-per-node 1 --master-addr 127.0.0.1 --master-port 29511 bench.py --gpus 1 --steps 20 --warmup 5 > "$O/bench_torchrun.json" 2> "$O/bench_torchrun.err"
  rc=$?; echo "torchrun bench rc=$rc"; cat "$O/bench_torchrun.json"
  if [ $rc -ne 0 ]; then tail -5 "$O/bench_torchrun.err"; exit $rc; fi
fi
if [ "${REHEARSAL:-0}" = "1" ]; then
  # the N>1 code path with 2 ranks on this one GPU (gloo group; not a scaling number)
  cd "$R"
  ZHIP_BENCH_REHEARSAL=1 timeout -k 10 400 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29513 bench.py --gpus 2 --full --steps 20 --warmup 5 --extra "${REHEARSAL_EXTRA:-c4,c5}" > "$O/bench_rehearsal2.json" 2> "$O/bench_rehearsal2.err"
  rc=$?; echo "rehearsal bench rc=$rc"; cat "$O/bench_rehearsal2.json"
  if [ $rc -ne 0 ]; then tail -15 "$O/bench_rehearsal2.err"; exit $rc; fi
fi
if [ "${PMC:-0}" = "1" ]; then
  bash "$R/scripts/gpu_pmc.sh"
  rc=$?
fi
exit $rc
