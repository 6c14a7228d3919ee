#!/bin/bash
# rocprofv3 kernel trace of the C2 bench command with its untimed tapped pass (--full), summarised per kernel and engine op:
#   OUT=<dir> bash tools/prof_ops.sh TAG
set -u
TAG=${1:-x}
OUT=${OUT:?set OUT to the directory the results go to}
mkdir -p $OUT
OUT=$(cd $OUT && pwd); ROOT=$PWD
export TMPDIR=/tmp
cd /tmp && timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$TAG -o trace -- python $ROOT/bench.py --full --steps 1 --warmup 1 --no-cpu-baseline > $OUT/rocprof_$TAG.log 2>&1
cd $ROOT && python tools/rocprof_summary.py $OUT/prof_$TAG/trace_kernel_trace.csv $OUT/prof_$TAG/summary.md && tail -1 $OUT/prof_$TAG/summary.md
