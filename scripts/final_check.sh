#!/bin/bash
# Round-end rehearsal on one GPU: the GPU test suite, smoke(), the default bench
# line with everything beside the timed steps (--full), and the rocprofv3 evidence
# (kernel stats + PMC passes), into the directory given (default bench_out/final_check).
#   bash scripts/final_check.sh [DIR]
cd "$(dirname "$0")/.." || exit 1
o=${1:-bench_out/final_check}
mkdir -p "$o"
timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > "$o/pytest_gpu.log" 2>&1
rc=$?; echo "pytest gpu rc=$rc"; tail -1 "$o/pytest_gpu.log"; [ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > "$o/smoke.log" 2>&1
rc=$?; echo "smoke rc=$rc"; tail -1 "$o/smoke.log"; [ $rc -eq 0 ] || exit $rc
timeout -k 10 600 python bench.py --full > "$o/bench_full.log" 2>&1
rc=$?; echo "bench rc=$rc"; [ $rc -eq 0 ] || { tail -5 "$o/bench_full.log"; exit $rc; }
grep '^{' "$o/bench_full.log" | tail -1 > "$o/bench_full.json"; cut -c1-400 "$o/bench_full.json"
timeout -k 10 300 python scripts/chains_bench.py > "$o/chains.log" 2>&1 || exit $?
grep '^{' "$o/chains.log" | tail -1 > "$o/chains.json"
if [ -n "$PROF" ]; then bash scripts/prof_round.sh ${PROF} > "$o/prof.log" 2>&1; echo "prof rc=$?"; fi
