#!/bin/bash
# describe: counters of k_describe (p1 issue mix incl. LDS conflicts, p2 waits, p3 fetch)
# Usage (needs a GPU, from any directory): tools/gpu_describe_pmc.sh <output dir>
out=$(realpath -m "${1:?usage: tools/gpu_describe_pmc.sh <output dir>}")
cd "$(dirname "$0")/.." || exit 1
export TMPDIR=/tmp
mkdir -p $out
cmd="python $PWD/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-ba --overlap 0 --batch 128 --fast-split 0"
( cd $out
  timeout 300 rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d $out/p3 -o p3 -- $cmd > $out/p3.log 2>&1
  timeout 300 rocprofv3 --kernel-trace --pmc SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_ACTIVE_INST_VALU SQ_LDS_BANK_CONFLICT --output-format csv -d $out/p1 -o p1 -- $cmd > $out/p1.log 2>&1
  timeout 300 rocprofv3 --kernel-trace --pmc SQ_WAIT_INST_ANY SQ_WAIT_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_LDS SQ_WAIT_INST_LDS SQ_INSTS_VMEM_RD SQ_LDS_IDX_ACTIVE SQ_LDS_ADDR_CONFLICT --output-format csv -d $out/p2 -o p2 -- $cmd > $out/p2.log 2>&1
)
python tools/pmc_summary.py $out > $out/summary.txt 2>&1
find $out -name '*.csv' -size +8M -delete
grep -A24 "k_describe" $out/summary.txt | head -30
