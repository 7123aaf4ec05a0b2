#!/bin/bash
# A/B of the PLL walk between two product builds of the package, in turn, three rounds:
#   bash scripts/walk_trans_ab.sh PARENT_PKG_DIR [OUT]     (new: the in-tree build)
# Per round and build: the walk by its own clock (roofline.ms_per_launch of the --full
# 20-step bench), a rocprofv3 kernel trace with the early hand-off off (--kernel-trace
# --stats only: the launch's duration is then the walk), the plain 20-step and 100-step
# bench lines.  Every GPU step under its own time limit; the first failure ends the run.
cd "$(dirname "$0")/.." || exit 1
set -o pipefail
export TMPDIR=/tmp
parent=${1:?parent package dir}
out=${2:-bench_out/walk_trans_ab}
mkdir -p "$out"
B="python3 bench.py --gpus 1 --no-cpu-baseline --no-components"
for r in 1 2 3; do
  for b in parent new; do
    if [ $b = parent ]; then export LDSP_PKG_DIR=$parent; else unset LDSP_PKG_DIR; fi
    t=$out/${b}_r$r
    timeout -k 10 300 $B --full --steps 20 --warmup 5 > $t.full20.json 2> $t.full20.err &&
    timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $t.trace -o walk0 -- \
        $B --full --steps 20 --warmup 5 --walk-early 0 > $t.trace.log 2>&1 &&
    timeout -k 10 300 $B --steps 20 --warmup 5 > $t.plain20.json 2> $t.plain20.err &&
    timeout -k 10 300 $B > $t.plain100.json 2> $t.plain100.err ||
      { echo "$b round $r: a step failed (rc $?)"; tail -5 $t.*.err $t.trace.log; exit 1; }
  done
done
python3 scripts/walk_trans_ab_table.py "$out"
