#!/bin/bash
# Run on the GPU box: re-collect the rocprofv3 kernel statistics that profiles/ holds.   tools/refresh_profiles.sh OUTDIR
# Output goes to OUTDIR/prof_*; copy the *_kernel_stats.csv files into profiles/ afterwards.
set -o pipefail
export TMPDIR=/tmp
O=$(realpath -m "${1:?usage: tools/refresh_profiles.sh OUTDIR}")
mkdir -p $O
rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_c2 -- python3 bench.py --full --steps 10 --warmup 3 --no-cpu-baseline > $O/prof_c2.log 2>&1 &&
rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_c345 -- python3 tools/bench_configs.py --configs c3,c4,c5 --reps 2 > $O/prof_c345.log 2>&1 &&
rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_rows -- python3 tools/bench_rows.py > $O/prof_rows.log 2>&1 &&
python3 bench.py --full --steps 10 --warmup 3 > $O/bench_n1.json 2> $O/bench_n1.err &&
python3 tools/bench_configs.py --configs c1,c3,c4,c5 --reps 3 > $O/configs.log 2>&1 &&
python3 tools/bench_rows.py > $O/rows.log 2>&1
echo "rc=$?"
find $O -name "*kernel_stats.csv" | head
