#!/bin/bash
# Round evidence on one GPU box: the GPU suite, smoke(), bench.py --full (default args) and a rocprofv3
# kernel trace of the same bench command.   bash tools/gpu_round_end.sh TAG
# Results go to $BEAST_OUT (default bench_out/).
set -u
TAG="${1:-r03}"
OUT="${BEAST_OUT:-bench_out}"
mkdir -p "$OUT"
timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --timeout 150 --timeout-method thread > "$OUT/pytest_gpu_$TAG.log" 2>&1
rc=$?; echo "pytest rc=$rc"; tail -n 2 "$OUT/pytest_gpu_$TAG.log"; [ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > "$OUT/smoke_$TAG.log" 2>&1
rc=$?; echo "smoke rc=$rc"; tail -n 2 "$OUT/smoke_$TAG.log"; [ $rc -eq 0 ] || exit $rc
timeout -k 10 900 python bench.py --full > "$OUT/bench_$TAG.json" 2> "$OUT/bench_$TAG.err"
rc=$?; echo "bench rc=$rc"; [ $rc -eq 0 ] || { tail -n 5 "$OUT/bench_$TAG.err"; exit $rc; }
cd /tmp && export TMPDIR=/tmp && cd - > /dev/null
mkdir -p "$OUT/prof_$TAG"
timeout -k 10 900 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof_$TAG" -o run -- python bench.py --full \
  > "$OUT/prof_$TAG/bench_under_rocprof.json" 2> "$OUT/prof_$TAG/stderr.log"
rc=$?; echo "rocprof rc=$rc"; find "$OUT/prof_$TAG" -name "*kernel_stats.csv"
exit $rc
