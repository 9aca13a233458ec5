#!/bin/bash
# kernel stats of the C3 MAPPO rollout (bench.py --full); usage: [OUT_DIR=prof_out] bash scripts/prof_roll.sh
set -u
export TMPDIR=/tmp
out=${OUT_DIR:-prof_out}
mkdir -p $out
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $out/prof_roll -o trace --output-format csv -- python bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --rollout-T 100 > $out/prof_roll_bench.log 2>&1 || exit $?
find $out/prof_roll -name '*kernel_stats.csv' -exec cp {} $out/kernel_stats_roll.csv \;
rm -rf $out/prof_roll
cat $out/kernel_stats_roll.csv | cut -d, -f1-8 | head -40
