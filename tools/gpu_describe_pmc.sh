#!/bin/bash
# describe: counters of k_describe alone (p1 issue mix incl. LDS conflicts, p2 waits and LDS cycles, p3 fetch): tools/ab_extract.py's child
# (64 frames, 3 repetitions) under rocprofv3, once per variant. Usage (GPU box, repo root): tools/gpu_describe_pmc.sh <output dir> "<VAR=VAL,VAR=VAL>" ...
# (a variant is an environment, e.g. OVS_LIB_PATH=<another build of the library>; "" = the tree's). One counter group per run, kernel trace
# only. A pass that fails or runs into its time limit ends the script with that status: nothing more is started on a card after a fault or a
# hang (the log of the failing pass is v<i>p<pass>.log in the output directory).
out=$(realpath -m "${1:?usage: tools/gpu_describe_pmc.sh <output dir> [VAR=VAL,...] ...}"); shift
[ $# -eq 0 ] && set -- ""
export TMPDIR=/tmp
mkdir -p $out
i=0
for v in "$@"; do
  i=$((i+1))
  envs=$(echo "$v" | tr ',' ' ')
  for pass in 1 2 3; do
    case $pass in
      1) ctr="SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_ACTIVE_INST_VALU SQ_LDS_BANK_CONFLICT" ;;
      2) ctr="SQ_WAIT_INST_ANY SQ_WAIT_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_LDS SQ_WAIT_INST_LDS SQ_INSTS_VMEM_RD SQ_LDS_IDX_ACTIVE SQ_LDS_ADDR_CONFLICT" ;;
      3) ctr="FETCH_SIZE" ;;
    esac
    ( cd /tmp && env $envs OVS_AB_CHILD=1 timeout -k 10 300 rocprofv3 --kernel-trace --pmc $ctr --output-format csv -d $out/v${i}p${pass} -o p -- python $OLDPWD/tools/ab_extract.py 64 3 > $out/v${i}p${pass}.log 2>&1 )
    rc=$?
    if [ $rc -ne 0 ]; then
      echo "variant $i ($v) pass $pass: exit status $rc, stopping" | tee -a $out/summary.txt
      tail -n 20 $out/v${i}p${pass}.log
      exit $rc
    fi
  done
  echo "== variant $i: $v" | tee -a $out/summary.txt
  python - $out $i <<'PY' | tee -a $out/summary.txt
import csv, glob, os, sys
from collections import defaultdict
root, i = sys.argv[1], sys.argv[2]
acc = defaultdict(list)
for f in glob.glob(os.path.join(root, "v%sp*" % i, "**", "*counter_collection.csv"), recursive=True):
    for row in csv.DictReader(open(f)):
        if "k_describe" in row.get("Kernel_Name", ""):
            acc[row["Counter_Name"]].append(float(row["Counter_Value"]))
for c in sorted(acc):
    print("    %-24s n=%-3d mean=%.5g" % (c, len(acc[c]), sum(acc[c]) / len(acc[c])))
if "SQ_WAVE_CYCLES" in acc and "SQ_BUSY_CYCLES" in acc:
    # resident wave-cycles per busy cycle of the counting units: compare it BETWEEN variants (its ratio is the ratio of the mean residency)
    print("    SQ_WAVE_CYCLES / SQ_BUSY_CYCLES = %.2f" % (sum(acc["SQ_WAVE_CYCLES"]) / sum(acc["SQ_BUSY_CYCLES"])))
PY
done
find $out -name '*.csv' -size +2M -delete; find $out -name '*.db' -delete
