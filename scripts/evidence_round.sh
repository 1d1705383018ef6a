#!/bin/bash
# Round evidence in one gpurun call (developer helper): GPU suite, the driver's bench command, its rocprofv3 kernel stats, the
# three PMC passes, the other workloads.  usage: [OUT=dir] scripts/evidence_round.sh TAG  -> OUT/TAG_* (default bench_logs/)
set -o pipefail
TAG=$1
ROOT=${GRAFT_REPO_ROOT:-$PWD}
OUT=${OUT:-$ROOT/bench_logs}; mkdir -p "$OUT"
cd $ROOT
scripts/gpu_round.sh $TAG || exit 1
timeout -k 10 300 python bench.py --gpus 1 --steps 20 --warmup 5 --full > $OUT/${TAG}_bench_driver_cmd.json.log 2> $OUT/${TAG}_bench_driver_cmd.err || exit 1
echo "driver-command bench done"
cd /tmp && export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/${TAG}_prof -o p -- python3 $ROOT/bench.py --gpus 1 --steps 20 --warmup 5 --full --no-cpu-baseline > $OUT/${TAG}_bench_profiled.json.log 2>&1 || exit 1
cd $ROOT
DB=$(find $OUT/${TAG}_prof -name "*.db" | head -1)
python scripts/rocpd_stats.py $DB $OUT/${TAG}_bench_kernel_stats.csv
rm -rf $OUT/${TAG}_prof
echo "kernel stats done"
scripts/pmc_round.sh $TAG || exit 1
timeout -k 10 300 python bench.py --full > $OUT/${TAG}_bench_default_50steps.json.log 2>/dev/null || exit 1
timeout -k 10 300 python bench.py --workload stage1 --steps 10 --warmup 2 > $OUT/${TAG}_bench_stage1.json.log 2>/dev/null || exit 1
timeout -k 10 300 python bench.py --workload pipeline --rounds 8 --steps 50 > $OUT/${TAG}_bench_pipeline_cfg5_bf16.json.log 2>/dev/null || exit 1
timeout -k 10 300 python bench.py --workload pipeline --rounds 8 --steps 50 --attn-precision fp8 > $OUT/${TAG}_bench_pipeline_cfg5_fp8.json.log 2>/dev/null || exit 1
timeout -k 10 200 python scripts/setup_breakdown_probe.py > $OUT/${TAG}_setup_probe.log 2>&1
tail -2 $OUT/${TAG}_setup_probe.log
echo "all done"
