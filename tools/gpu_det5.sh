# deterministic-finalize check: targeted kernel tests, determinism / graph / training-step / parity
# suites, the traced bench line and an optional env A/B (gpu_check5.sh without the parity step repeated)
#   bash tools/gpu_det5.sh TAG "pytest -k expr"
set -o pipefail
export TMPDIR=/tmp
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
TAG=${1:-det}
KEXPR=${2:-layernorm}
PT="python -u -m pytest -x -q --timeout 200 --timeout-method thread"
timeout -k 10 400 $PT tests/test_kernels_gpu.py -k "$KEXPR" > "$OUT/${TAG}_ktest.log" 2>&1 || { echo KTEST_FAILED; tail -30 "$OUT/${TAG}_ktest.log"; exit 1; }
tail -1 "$OUT/${TAG}_ktest.log"
timeout -k 10 700 $PT tests/test_determinism_gpu.py tests/test_graph_gpu.py tests/test_parity_gpu.py tests/test_training_step_gpu.py > "$OUT/${TAG}_suites.log" 2>&1 || { echo SUITES_FAILED; tail -40 "$OUT/${TAG}_suites.log"; exit 1; }
tail -1 "$OUT/${TAG}_suites.log"
timeout -k 10 900 python3 bench.py --full --trace-steps 10 --trace-out "$OUT/${TAG}_kernel_stats.csv" > "$OUT/${TAG}_bench.log" 2> "$OUT/${TAG}_bench.err" || { echo BENCH_FAILED; tail -20 "$OUT/${TAG}_bench.err"; exit 1; }
cut -c1-200 "$OUT/${TAG}_bench.log"
python3 tools/step_profile.py "$OUT/${TAG}_kernel_stats.csv" "$OUT/${TAG}_kernel_stats_sorted.csv" --steps 10 --bench "$OUT/${TAG}_bench.log" > "$OUT/${TAG}_step_profile.txt" || exit 1
head -14 "$OUT/${TAG}_step_profile.txt"
echo CHECK_DONE
