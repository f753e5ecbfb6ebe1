set -o pipefail
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
export TMPDIR=/tmp
timeout -k 10 300 python -u -m pytest tests/test_kernels_gpu.py -k "flash or attention or attn" -x -q --timeout 120 --timeout-method thread > "$OUT/fl.log" 2>&1 || { tail -30 "$OUT/fl.log"; exit 1; }
tail -2 "$OUT/fl.log"
timeout -k 10 200 python -u tools/attn_bench.py --iters 20 > "$OUT/attn.log" 2>&1 || exit 1
cat "$OUT/attn.log"
[ -n "$NOBENCH" ] || timeout -k 10 300 python -u bench.py --full > "$OUT/bench.log" 2> "$OUT/bench.err" || exit 1
[ -n "$NOBENCH" ] || cat "$OUT/bench.log"
