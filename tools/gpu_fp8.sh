# MX-fp8 model-level tests + config-5 bench (run via gpurun from the repo root)
set -o pipefail
export TMPDIR=/tmp
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
timeout -k 10 500 python -u -m pytest tests/test_mx8_gpu.py tests/test_fp8_gpu.py -x -q -s -rf --timeout 240 --timeout-method thread > "$OUT/fp8_tests.log" 2>&1
rc=$?
grep -E "fp8 vs bf16|MX-fp8 GEMM|config 5 losses|passed|failed|Error" "$OUT/fp8_tests.log" | tail -20
[ $rc -eq 0 ] || { tail -40 "$OUT/fp8_tests.log"; exit $rc; }
timeout -k 10 400 python -u bench.py --full --config 5 --steps 10 --warmup 3 --cpu-baseline 0 --kernel-table > "$OUT/bench_c5.log" 2> "$OUT/bench_c5.err" || { echo BENCH_FAILED; tail -30 "$OUT/bench_c5.err"; exit 1; }
cat "$OUT/bench_c5.log"
timeout -k 10 400 python -u bench.py --frames 16 --steps 10 --warmup 3 --cpu-baseline 0 > "$OUT/bench_c5_bf16.log" 2> "$OUT/bench_c5_bf16.err" || { echo BENCH_FAILED; tail -30 "$OUT/bench_c5_bf16.err"; exit 1; }
cat "$OUT/bench_c5_bf16.log"
