# informational: the bench step with dropout off (bench.py --dropout 0) under the kernel trace, to price
# the dropout work inside the attention / GEMM kernels against the default trace of the same call
#   bash tools/gpu_drop0.sh TAG
set -o pipefail
export TMPDIR=/tmp
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
TAG=${1:-drop0}
timeout -k 10 600 python3 bench.py --full --dropout 0 --cpu-baseline 0 --trace-steps 10 --trace-out "$OUT/${TAG}_kernel_stats.csv" > "$OUT/${TAG}_bench.log" 2> "$OUT/${TAG}_bench.err" || { echo BENCH_FAILED; tail -20 "$OUT/${TAG}_bench.err"; exit 1; }
cut -c1-200 "$OUT/${TAG}_bench.log"
python3 tools/step_profile.py "$OUT/${TAG}_kernel_stats.csv" "$OUT/${TAG}_kernel_stats_sorted.csv" --steps 10 --bench "$OUT/${TAG}_bench.log" > "$OUT/${TAG}_step_profile.txt" || exit 1
head -12 "$OUT/${TAG}_step_profile.txt"
