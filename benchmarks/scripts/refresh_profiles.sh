set -x
R=$(cd "$(dirname "$0")/../.." && pwd); OUT=${OUT:-$R/profile_runs}; mkdir -p $OUT
cd $R
python bench.py --full --steps 50 --warmup 10 > $OUT/r3_c2.json 2> $OUT/r3_c2.err
python bench.py --full --stage 1 --steps 20 --warmup 5 --no-cpu-baseline > $OUT/r3_s1.json 2>/dev/null
python bench.py --full --config c5 --steps 10 --warmup 4 --no-cpu-baseline > $OUT/r3_c5.json 2>/dev/null
python bench.py --full --stage 3 --steps 50 --warmup 10 --no-cpu-baseline > $OUT/r3_s3.json 2>/dev/null
python bench.py --full --stage 4 --steps 50 --warmup 10 --no-cpu-baseline > $OUT/r3_s4.json 2>/dev/null
python bench.py --full --steps 300 --warmup 10 --no-cpu-baseline --no-instrument > $OUT/r3_sustained.json 2>/dev/null
cd /tmp; export TMPDIR=/tmp
ACT_OVERLAP_TEACHER=0 ACT_OVERLAP_DW=0 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_r3 -- python $R/bench.py --steps 16 --warmup 4 --no-cpu-baseline --no-instrument > $OUT/prof_r3.log 2>&1
rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d $OUT/pmc_fetch_r3 -- python $R/bench.py --steps 2 --warmup 1 --no-cpu-baseline --no-instrument > $OUT/pmc_fetch_r3.log 2>&1
rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d $OUT/pmc_write_r3 -- python $R/bench.py --steps 2 --warmup 1 --no-cpu-baseline --no-instrument > $OUT/pmc_write_r3.log 2>&1
ACT_OVERLAP_TEACHER=0 ACT_OVERLAP_DW=0 rocprofv3 --kernel-trace --pmc MfmaUtil --output-format csv -d $OUT/pmc_mfma_r3 -- python $R/bench.py --steps 2 --warmup 1 --no-cpu-baseline --no-instrument > $OUT/pmc_mfma_r3.log 2>&1
cd $R
python benchmarks/pmc_traffic.py $OUT/pmc_fetch_r3 $OUT/pmc_write_r3 > $OUT/r3_pmc_traffic.json
python benchmarks/pmc_mfma_util.py $OUT/pmc_mfma_r3 > $OUT/r3_pmc_mfma_util.json
find $OUT/prof_r3 -name "*kernel_stats.csv" | head -1 | xargs -I{} cp {} $OUT/r3_kernel_stats.csv
# keep the merged-back payload small: drop the raw traces
rm -rf $OUT/prof_r3 $OUT/pmc_fetch_r3 $OUT/pmc_write_r3 $OUT/pmc_mfma_r3
ls -la $OUT | tail -15
