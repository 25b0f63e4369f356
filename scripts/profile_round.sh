# Round profile on the GPU box: bench lines + rocprofv3 kernel stats + PMC passes, condensed into profiles/<tag>*_{kernel_stats_bench.csv,pmc.json}.
# usage: bash scripts/profile_round.sh <tag> [variants]     (variants: also profile the --paired and --read-len 300 workloads, tags <tag>_paired / <tag>_300bp)
# The round's bench lines are --full runs (the docs read their CPU baseline, rooflines and rows after the hot path).
# Every rocprofv3 run is the same bench.py command (hg38-scale default workload, PCIe loop / CPU baseline / next rows off);
# counters are collected in their own runs, one counter group per run, without any trace option beside them; the program itself
# (python3 bench.py ...) stands directly behind `--`.
set -x
TAG=${1:-r05}
R=$GRAFT_REPO_ROOT; cd $R
O=${BENCH_OUT:-$R/bench_out}; mkdir -p $O
df -h /tmp /dev/shm | tail -2; free -g | head -2
export BENCH_INDEX_CACHE=${BENCH_INDEX_CACHE:-/tmp/bmh_cache}   # first run builds + saves genome and index, the rocprofv3 runs load them
python bench.py --full > $O/${TAG}_bench.json 2> $O/${TAG}_bench.err || { tail -5 $O/${TAG}_bench.err; exit 1; }
tail -c 300 $O/${TAG}_bench.json
if [ "$2" = "variants" ]; then
  python bench.py --full --paired --cpu-sample 20000 > $O/${TAG}_bench_paired.json 2>/dev/null || exit 1
  python bench.py --full --read-len 300 --cpu-sample 20000 > $O/${TAG}_bench_300bp.json 2>/dev/null || exit 1
fi
profile_one() {     # <tag> <extra bench args>
  local T=$1; shift
  local ARGS="--no-pcie --cpu-sample 0 --no-next-rows $*"
  cd /tmp; export TMPDIR=/tmp
  for d in prof pmc_fetch pmc_write pmc_sq; do rm -rf $O/${d}_${T}; mkdir -p $O/${d}_${T}; done
  rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_${T} -- python3 $R/bench.py --steps 5 --warmup 1 $ARGS > $O/prof_${T}/bench.json 2> $O/prof_${T}/err.log || return 1
  rocprofv3 --pmc FETCH_SIZE --output-format csv -d $O/pmc_fetch_${T} -- python3 $R/bench.py --steps 2 --warmup 1 $ARGS > $O/pmc_fetch_${T}/bench.json 2> $O/pmc_fetch_${T}/err.log || return 1
  rocprofv3 --pmc WRITE_SIZE --output-format csv -d $O/pmc_write_${T} -- python3 $R/bench.py --steps 2 --warmup 1 $ARGS > $O/pmc_write_${T}/bench.json 2> $O/pmc_write_${T}/err.log || return 1
  rocprofv3 --pmc SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAVES GRBM_GUI_ACTIVE --output-format csv -d $O/pmc_sq_${T} -- python3 $R/bench.py --steps 2 --warmup 1 $ARGS > $O/pmc_sq_${T}/bench.json 2> $O/pmc_sq_${T}/err.log || return 1
  cd $R
  find $O/prof_${T} -name "*kernel_trace.csv" -delete
  python scripts/summarize_profiles.py ${T} $O/prof_${T} $O/pmc_fetch_${T} $O/pmc_write_${T} $O/pmc_sq_${T} || return 1
  cp profiles/${T}_kernel_stats_bench.csv profiles/${T}_pmc.json $O/
  find $O/pmc_fetch_${T} $O/pmc_write_${T} $O/pmc_sq_${T} -name "*.csv" -size +1M -delete
}
profile_one ${TAG} || exit 1
if [ "$2" = "variants" ]; then
  profile_one ${TAG}_paired --paired || exit 1
  profile_one ${TAG}_300bp --read-len 300 || exit 1
fi
