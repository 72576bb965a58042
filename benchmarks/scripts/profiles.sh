# per-round evidence (RND=rNN, default r05): bench lines of every workload + rocprofv3 kernel stats, per-workload PMC traffic (FETCH_SIZE / WRITE_SIZE, separate passes) and
# MfmaUtil, written to $OUT (default profile_runs/).  usage: [RND=r05] [OUT=dir] profiles.sh <tag> <bench args...>   e.g.  profiles.sh c2 ; profiles.sh s1 --stage 1 ; profiles.sh c5 --config c5
set -x
RND=${RND:-r05}
R=$(cd "$(dirname "$0")/../.." && pwd); OUT=${OUT:-$R/profile_runs}; mkdir -p $OUT; TAG=$1; shift; ARGS="$@"
cd $R
timeout 900 python bench.py $ARGS --full --steps 30 --warmup 8 --no-other-workloads > $OUT/${RND}_bench_$TAG.json 2> $OUT/${RND}_bench_$TAG.err
cd /tmp; export TMPDIR=/tmp
ACT_OVERLAP_TEACHER=0 ACT_OVERLAP_DW=0 timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$TAG -- python $R/bench.py $ARGS --steps 16 --warmup 4 --no-cpu-baseline --no-instrument --no-other-workloads > $OUT/prof_$TAG.log 2>&1
timeout 900 rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d $OUT/pmc_fetch_$TAG -- python $R/bench.py $ARGS --steps 2 --warmup 1 --no-cpu-baseline --no-instrument --no-other-workloads > $OUT/pmc_fetch_$TAG.log 2>&1
timeout 900 rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d $OUT/pmc_write_$TAG -- python $R/bench.py $ARGS --steps 2 --warmup 1 --no-cpu-baseline --no-instrument --no-other-workloads > $OUT/pmc_write_$TAG.log 2>&1
ACT_OVERLAP_TEACHER=0 ACT_OVERLAP_DW=0 timeout 900 rocprofv3 --kernel-trace --pmc MfmaUtil --output-format csv -d $OUT/pmc_mfma_$TAG -- python $R/bench.py $ARGS --steps 2 --warmup 1 --no-cpu-baseline --no-instrument --no-other-workloads > $OUT/pmc_mfma_$TAG.log 2>&1
cd $R
python benchmarks/pmc_traffic.py $OUT/pmc_fetch_$TAG $OUT/pmc_write_$TAG $TAG > $OUT/${RND}_pmc_traffic_$TAG.json
python benchmarks/pmc_mfma_util.py $OUT/pmc_mfma_$TAG > $OUT/${RND}_pmc_mfma_util_$TAG.json
find $OUT/prof_$TAG -name "*kernel_stats.csv" | head -1 | xargs -I{} cp {} $OUT/${RND}_${TAG}_kernel_stats.csv
f=$(find $OUT/prof_$TAG -name "*kernel_trace.csv" | head -1); python benchmarks/trace_by_grid.py $f 23 > $OUT/${RND}_${TAG}_trace_by_grid.txt
rm -rf $OUT/prof_$TAG $OUT/pmc_fetch_$TAG $OUT/pmc_write_$TAG $OUT/pmc_mfma_$TAG
ls -la $OUT | grep ${RND}_ | tail -12
