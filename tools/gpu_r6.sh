# round-6 check: (optional) full GPU suite, smoke, the bench line with its traced roofline.
#   bash tools/gpu_r6.sh TAG [tests|notests] [extra bench args]
set -o pipefail
export TMPDIR=/tmp
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
TAG=${1:-r6}
MODE=${2:-tests}
shift 2 2>/dev/null
PT="python -u -m pytest -x -q --timeout 200 --timeout-method thread"
if [ "$MODE" = "tests" ]; then
  timeout -k 10 600 $PT tests -m gpu > "$OUT/${TAG}_gpu_tests.log" 2>&1 || { echo TESTS_FAILED; tail -60 "$OUT/${TAG}_gpu_tests.log"; exit 1; }
  tail -1 "$OUT/${TAG}_gpu_tests.log"
  timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke()" > "$OUT/${TAG}_smoke.log" 2>&1 || { echo SMOKE_FAILED; tail -30 "$OUT/${TAG}_smoke.log"; exit 1; }
  tail -2 "$OUT/${TAG}_smoke.log"
fi
timeout -k 10 900 python3 bench.py --full --trace-steps 10 --trace-out "$OUT/${TAG}_kernel_stats.csv" --shape-table "$OUT/${TAG}_shape_table.txt" "$@" > "$OUT/${TAG}_bench.log" 2> "$OUT/${TAG}_bench.err" || { echo BENCH_FAILED; tail -20 "$OUT/${TAG}_bench.err"; exit 1; }
cut -c1-300 "$OUT/${TAG}_bench.log"
python3 tools/step_profile.py "$OUT/${TAG}_kernel_stats.csv" "$OUT/${TAG}_kernel_stats_sorted.csv" --steps 10 --bench "$OUT/${TAG}_bench.log" > "$OUT/${TAG}_step_profile.txt" || exit 1
cat "$OUT/${TAG}_step_profile.txt"
echo CHECK_DONE
