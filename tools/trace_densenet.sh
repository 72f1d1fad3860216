#!/bin/bash
# kernel trace of the DenseNet bench run with its roofline and secondary passes (--full); results in $OUT_DIR (default trace_out/)
cd /tmp && export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
O=${OUT_DIR:-$R/trace_out}; mkdir -p $O
rocprofv3 --kernel-trace --stats -d $O/dn_trace -- python $R/bench.py --full --model densenet --steps 6 --warmup 3 --no_cpu_baseline > $O/dn_trace.json 2> $O/dn_trace.err
f=$(find $O/dn_trace -name "*.db" | head -1)
python $R/tools/rocpd_shapes.py $f 70 > $O/dn_shapes.txt
python $R/tools/class_stats.py $f > $O/dn_class.txt 2>&1
cat $O/dn_trace.json
