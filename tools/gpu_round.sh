# one GPU call: gpu tests (all, report failures), smoke, then the bench with the kernel table
# (run via gpurun from the repo root)
set -o pipefail
export TMPDIR=/tmp
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
timeout -k 10 900 python -u -m pytest tests -m gpu -q -rf --timeout 150 --timeout-method thread > "$OUT/gpu_tests.log" 2>&1
rc=$?
tail -25 "$OUT/gpu_tests.log"
if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then echo "TESTS_ABORTED rc=$rc"; exit $rc; fi
timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke()" > "$OUT/smoke.log" 2>&1 || { echo SMOKE_FAILED; tail -20 "$OUT/smoke.log"; exit 1; }
timeout -k 10 400 python -u bench.py --full --kernel-table > "$OUT/bench.log" 2> "$OUT/bench.err" || { echo BENCH_FAILED; tail -30 "$OUT/bench.err"; exit 1; }
cat "$OUT/bench.log"
exit $rc
