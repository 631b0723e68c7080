#!/bin/bash
# rocprofv3 --kernel-trace --stats over bench.py itself (default workload, then BASELINE config 3), on an MI355X:
#   bash profiles/stats_bench.sh          summaries -> $OUT (default build/profiles)
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/build/profiles}
WORK=$(mktemp -d)
mkdir -p "$OUT"
rocprofv3 --kernel-trace --stats --output-format csv -d "$WORK/sb_l" -o s -- python3 "$R/bench.py" --steps 20 --warmup 3 --full --no-cpu-baseline > "$OUT/sb_lambert.log" 2>&1 || tail -5 "$OUT/sb_lambert.log"
rocprofv3 --kernel-trace --stats --output-format csv -d "$WORK/sb_c" -o s -- python3 "$R/bench.py" --config rpv_nan --steps 10 --warmup 3 --full --no-cpu-baseline > "$OUT/sb_config3.log" 2>&1 || tail -5 "$OUT/sb_config3.log"
cp "$(find "$WORK/sb_l" -name "*kernel_stats.csv" | head -1)" "$OUT/stats_bench_lambert.csv"
cp "$(find "$WORK/sb_c" -name "*kernel_stats.csv" | head -1)" "$OUT/stats_bench_config3.csv"
head -8 "$OUT/stats_bench_lambert.csv" | cut -c1-160
