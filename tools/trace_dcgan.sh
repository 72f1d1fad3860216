#!/bin/bash
# kernel trace of the DCGAN bench run with its roofline and secondary passes (--full); results in $OUT_DIR (default trace_out/)
cd /tmp && export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
O=${OUT_DIR:-$R/trace_out}; mkdir -p $O
rocprofv3 --kernel-trace --stats -d $O/dc_trace -- python $R/bench.py --full --steps 6 --warmup 6 --no_cpu_baseline > $O/dc_trace.json 2> $O/dc_trace.err
f=$(find $O/dc_trace -name "*.db" | head -1)
python $R/tools/rocpd_shapes.py $f 60 > $O/dc_shapes.txt
python $R/tools/rocpd_stats.py $f $O/dc_kernel_stats.csv > /dev/null
rm -rf $O/dc_trace
