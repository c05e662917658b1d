#!/bin/bash
# rocprofv3 kernel statistics of one bench configuration:  bash tools/stats_config.sh c4   ->  results/stats_<cfg>.csv
set -u
ROOT=${GRAFT_REPO_ROOT:-$(pwd)}
CFG=$1
mkdir -p $ROOT/results
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats -d /tmp/stats_$CFG -o s --output-format csv -- \
  python3 $ROOT/bench.py --full --config $CFG --steps 3 --warmup 1 --no-cpu-baseline > $ROOT/results/stats_$CFG.json 2> $ROOT/results/stats_$CFG.err || exit 1
cp $(ls /tmp/stats_$CFG/*kernel_stats.csv /tmp/stats_$CFG/*/*kernel_stats.csv 2>/dev/null | head -1) $ROOT/results/stats_$CFG.csv
