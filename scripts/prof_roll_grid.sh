#!/bin/bash
# kernel trace of both rollout lines (C3 MAPPO, C2 IPPO; bench.py --full), grouped by (kernel, grid)
# usage: [OUT_DIR=prof_out] bash scripts/prof_roll_grid.sh
set -u
export TMPDIR=/tmp
out=${OUT_DIR:-prof_out}
mkdir -p $out
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $out/prof_rg -o trace --output-format csv -- python bench.py --full --steps 10 --warmup 3 --no-cpu-baseline > $out/prof_rg_bench.log 2>&1 || exit $?
python3 scripts/trace_by_grid.py $out/prof_rg $out/kernel_stats_by_grid_rollouts_s2.csv || exit $?
rm -rf $out/prof_rg
cut -c1-200 $out/kernel_stats_by_grid_rollouts_s2.csv | head -30
