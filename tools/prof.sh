#!/bin/bash
# usage (MI355X, from the repository root): tools/prof.sh <tag> [bench args...]
# kernel-trace + stats of a short plain bench run -> $RU3D_OUT/prof_<tag>/ (default evidence_out/) and a per-kernel
# summary on stdout
tag=$1; shift
root=$(pwd)
cd /tmp && export TMPDIR=/tmp && cd "$root"
outdir=${RU3D_OUT:-evidence_out}; mkdir -p "$outdir"
rocprofv3 --kernel-trace --stats --output-format csv -d $outdir/prof_$tag -o runc -- python3 bench.py --steps 2 --warmup 1 --no-probe "$@" > $outdir/prof_$tag.log 2>&1
python3 tools/kstats.py $outdir/prof_$tag 3 60 > $outdir/prof_$tag.txt
head -50 $outdir/prof_$tag.txt
