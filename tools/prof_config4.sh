#!/bin/bash
# config-4 kernel trace (F = 30 fp16, 2x160x160x80) -> $RU3D_OUT/c4_trace.txt (default evidence_out/)
root=$(pwd); cd /tmp && export TMPDIR=/tmp && cd "$root"
outdir=${RU3D_OUT:-evidence_out}; mkdir -p "$outdir"
rocprofv3 --kernel-trace --stats --output-format csv -d $outdir/prof_c4 -o runc -- python3 bench.py --features 30 --dtype fp16 --patch 160 160 80 --steps 2 --warmup 1 --no-probe --launch eager > $outdir/prof_c4.log 2>&1
python3 tools/ktrace.py $outdir/prof_c4 3 70 > $outdir/c4_trace.txt
head -60 $outdir/c4_trace.txt
