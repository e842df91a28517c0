#!/bin/bash
# Run on the GPU box (via gpurun): kernel-trace stats + separate PMC passes of bench.py.
# Usage: tools/profile.sh <tag> [bench args...]   -> writes gpurun_out/prof_<tag>/
# Every pass runs under a time limit of its own and the script stops at the first pass that fails: nothing more is started on a
# card after a fault, an abort or a hang.
set -u
TAG=${1:-r01}; shift || true
REPO=$(cd "$(dirname "$0")/.." && pwd)
OUT=$REPO/gpurun_out/prof_$TAG
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
ARGS="--steps 10 --warmup 2 --passes-per-step 1 --full --no-cpu-baseline --no-secondary $*"
TRACE_ARGS="--full --no-cpu-baseline --no-secondary $*"   # the default bench.py run (50 steps / 5 warm-up) with the judged workload's side figures
# bench.py's default run takes ~30 s unprofiled (driver_run_s 30.9, BENCH_r06.json); the trace multiplies that by the cost of
# recording every launch, a 10-step counter pass stays below it: 10 x / 5 x headroom
TRACE_LIMIT=300; PMC_LIMIT=150
pass() {   # pass <seconds> <log> <command...>
  local limit=$1 log=$2; shift 2
  timeout -k 10 $limit "$@" > $log 2>&1
  local rc=$?
  if [ $rc -ne 0 ]; then echo "profile.sh: $log: exit status $rc (124 / 137: time limit of $limit s) - stopping here"; tail -5 $log; exit $rc; fi
}
pass $TRACE_LIMIT $OUT/trace.log rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/trace -o trace -- python3 $REPO/bench.py $TRACE_ARGS
for grp in "SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_INSTS_VALU SQ_INSTS_MFMA SQ_INSTS_SALU SQ_INSTS_LDS SQ_VALU_MFMA_BUSY_CYCLES" \
           "SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_ANY SQ_WAIT_INST_ANY SQ_WAIT_ANY SQ_INST_CYCLES_VMEM SQ_ACTIVE_INST_LDS SQ_LDS_BANK_CONFLICT SQ_INSTS_VALU_TRANS" \
           "GRBM_GUI_ACTIVE GRBM_COUNT" \
           "FETCH_SIZE" "WRITE_SIZE"; do
  name=$(echo $grp | tr ' ' '_' | cut -c1-40)
  pass $PMC_LIMIT $OUT/pmc_$name.log rocprofv3 --pmc $grp --output-format csv -d $OUT/pmc_$name -o pmc -- python3 $REPO/bench.py $ARGS
done
find $OUT -name "*.csv" | head -30
