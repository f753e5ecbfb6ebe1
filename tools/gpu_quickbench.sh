# kernel tests of the GEMM paths + parity, then the full bench (from the repo root)
set -o pipefail
export TMPDIR=/tmp
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
timeout -k 10 400 python -u -m pytest tests/test_kernels_gpu.py tests/test_mx8_gpu.py tests/test_parity_gpu.py tests/test_frametape_gpu.py -x -q -rf --timeout 150 --timeout-method thread > "$OUT/qb_tests.log" 2>&1
rc=$?
tail -3 "$OUT/qb_tests.log"
[ $rc -eq 0 ] || { tail -40 "$OUT/qb_tests.log"; exit $rc; }
timeout -k 10 400 python -u bench.py --full --cpu-baseline 0 ${BENCH_ARGS} > "$OUT/qb_bench.log" 2> "$OUT/qb_bench.err" || { echo BENCH_FAILED; tail -30 "$OUT/qb_bench.err"; exit 1; }
cat "$OUT/qb_bench.log"
