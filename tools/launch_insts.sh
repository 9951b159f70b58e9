#!/bin/bash
# Instructions a k_sfm_step launch executes with 1 and with 20 fused substeps (cfg3), per wavefront: the difference / 19 is a substep, the rest is
# what a launch executes around its substeps.  Counter passes in runs of their own, no trace domain beside --pmc (tools/prologue_insts.sh took a
# kernel trace in the same run).  usage (on the GPU): tools/launch_insts.sh OUTDIR LIBRARY -> OUTDIR.txt, OUTDIR_ns{1,20}_pmc.csv
O=$(mkdir -p "$1" && cd "$1" && pwd); LIB=$2
R=$(cd "$(dirname "$0")/.." && pwd)
rm -rf $O/ns1 $O/ns20 $O/ns1b $O/ns20b
export CROWDSTEP_LIB=$LIB
cd $O
for ns in 1 20; do
  timeout -k 10 240 rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAVES SQ_WAVE_CYCLES SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_INSTS_SMEM --output-format csv -d $O/ns$ns -- python3 $R/bench.py --no-cpu-baseline --no-other-configs --no-gym-step --full-json $O/ns$ns.json --steps 20 --warmup 5 --repeats 1 --substeps $ns > $O/ns$ns.log 2>&1 || { echo "rocprofv3 ns=$ns failed: $?"; tail -5 $O/ns$ns.log; exit 1; }
done
# branch instructions in a pass of their own (the eight counters above fill one), where the machine lists the counter
if rocprofv3 --list-avail 2>/dev/null | grep -qw SQ_INSTS_BRANCH; then
  rm -rf $O/ns1b $O/ns20b
  for ns in 1 20; do
    timeout -k 10 240 rocprofv3 --pmc SQ_INSTS_BRANCH --output-format csv -d $O/ns${ns}b -- python3 $R/bench.py --no-cpu-baseline --no-other-configs --no-gym-step --full-json $O/ns$ns.json --steps 20 --warmup 5 --repeats 1 --substeps $ns > $O/ns${ns}b.log 2>&1 || { echo "rocprofv3 (branch pass) ns=$ns failed: $?"; tail -5 $O/ns${ns}b.log; exit 1; }
  done
fi
python3 $R/tools/launch_insts_reduce.py $O | tee $O.txt
find $O -name "*.csv" -size +200k -delete
