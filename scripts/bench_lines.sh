#!/bin/bash
# the bench lines of a round: bench_lines.sh <tag>  ->  $BENCH_OUT/<tag>_bench{_driver_cmd,,_paired,_300bp}.json  (copy them to profiles/)
# every line with --full: the docs' numbers (scripts/fill_docs.py, design_numbers.py) read the CPU baseline, rooflines and rows beside the headline
TAG=${1:-r05}
R=${GRAFT_REPO_ROOT:-$(cd "$(dirname "$0")/.." && pwd)}; cd $R
O=${BENCH_OUT:-$R/bench_out}; mkdir -p $O
export BENCH_INDEX_CACHE=${BENCH_INDEX_CACHE:-/tmp/bmh_cache}
( while true; do sleep 60; echo "[$(date +%T)] bench lines"; done ) &
HB=$!
python3 bench.py --full --gpus 1 --steps 20 --warmup 5 > $O/${TAG}_bench_driver_cmd.json 2> $O/${TAG}_bench_driver_cmd.err || { kill $HB; tail -5 $O/${TAG}_bench_driver_cmd.err; exit 1; }
python3 bench.py --full > $O/${TAG}_bench.json 2>/dev/null || { kill $HB; exit 1; }
python3 bench.py --full --paired --cpu-sample 20000 > $O/${TAG}_bench_paired.json 2>/dev/null || { kill $HB; exit 1; }
python3 bench.py --full --read-len 300 --cpu-sample 20000 > $O/${TAG}_bench_300bp.json 2>/dev/null || { kill $HB; exit 1; }
kill $HB
head -c 600 $O/${TAG}_bench_driver_cmd.json
