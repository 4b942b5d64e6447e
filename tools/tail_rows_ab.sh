#!/bin/bash
# k_tail tile shape A/B: 32-, 4- and 16-row tiles forced through the test library's omds_debug_force_tile_rows
# (include/omds_test.h), kernel trace + bench per workload.  Needs libomds_hip_test.so (make -C optimalmodulationds_amd/csrc).
# usage: bash tools/tail_rows_ab.sh [workload ...]
R=$(cd "$(dirname "$0")/.." && pwd)
# the test hooks and the benchmark use the same library
export TMPDIR=/tmp OMDS_LIB=$R/optimalmodulationds_amd/csrc/libomds_hip_test.so
OUT=$PWD/gpurun_out/tail_rows; mkdir -p $OUT
cd /tmp
for wl in "${@:-franka_shelf_1024x32}"; do
for rows in 32 4 16; do
  rocprofv3 --kernel-trace --stats -d $OUT/kt -- python3 -c "
import sys
sys.path.insert(0, '$R')
from optimalmodulationds_amd import _lib
assert _lib.load_test_hooks().omds_debug_force_tile_rows(0, $rows) == 0
import bench
sys.argv = ['bench.py'] + sys.argv[1:]
bench.main()" --path fp32 --steps 2 --warmup 1 --workload $wl > $OUT/log_$rows.txt 2>&1
  echo "$wl tail_rows=$rows $(python3 $R/tools/rocprof_summary.py stats "$(find $OUT/kt -name '*_results.db' | head -1)" | grep k_tail | head -1)"
  rm -rf $OUT/kt
done
done
