#!/bin/bash
# encode / reconstruct A/B on one box: parity of the variant library (encode / reconstruct tests),
# then the codec-only bench of product and variant, interleaved:   bash tools/ab/codec_ab.sh VARIANT.so TAG
# Results go to $BEAST_OUT (default bench_out/).
set -u
VAR="$1"; TAG="${2:-ab}"
OUT="${BEAST_OUT:-bench_out}"
mkdir -p "$OUT"
BEAST_LIB=$VAR timeout -k 10 600 python -u -m pytest tests/test_gpu_parity.py -m gpu -x -q --timeout 120 \
  --timeout-method thread -k "reconstruct or encode or decode" > "$OUT/ab_${TAG}_tests.log" 2>&1
rc=$?; echo "variant tests rc=$rc"; tail -n 2 "$OUT/ab_${TAG}_tests.log"; [ $rc -eq 0 ] || exit $rc
for i in 1 2 3; do
  for L in product variant; do
    if [ $L = variant ]; then export BEAST_LIB=$VAR; else unset BEAST_LIB; fi
    timeout -k 10 300 python bench.py --full --no-bpe --no-fit --no-cpu --no-large --steps 20 \
      > "$OUT/ab_${TAG}_${L}_$i.json" 2> "$OUT/ab_${TAG}_${L}_$i.err" || exit 3
    python - "$L" "$OUT/ab_${TAG}_${L}_$i.json" <<'PY'
import json, sys
l = json.loads(open(sys.argv[2]).read().strip().splitlines()[-1])
e = l["roofline"]["events"]
print("%-8s value %.1fM  gpu/step %.2f us  enc %.2f us  rec %.2f us" % (sys.argv[1], l["value"] / 1e6,
      l["timing"]["median_gpu_event_us_per_step"], e["k_encode_pipe_us"], e["k_reconstruct_us"]))
PY
  done
done
