#!/bin/bash
# usage (MI355X, from the repository root): tools/pmc_step.sh <tag> [bench args]   -> whole-step HBM traffic from two PMC
# passes over a plain eager bench run, under $RU3D_OUT (default evidence_out/)
# (FETCH_SIZE and WRITE_SIZE cannot share a pass on gfx950), per kernel and in total, with the guide's corrections
tag=$1; shift
root=$(pwd)
cd /tmp && export TMPDIR=/tmp && cd "$root"
outdir=${RU3D_OUT:-evidence_out}; mkdir -p "$outdir"
B="bench.py --steps 2 --warmup 1 --no-probe --launch eager $@"
rocprofv3 --pmc FETCH_SIZE --output-format csv -d $outdir/pmcstep_${tag}_fetch -- python3 $B > $outdir/pmcstep_${tag}_fetch.log 2>&1
rocprofv3 --pmc WRITE_SIZE --output-format csv -d $outdir/pmcstep_${tag}_write -- python3 $B > $outdir/pmcstep_${tag}_write.log 2>&1
python3 tools/pmc_step.py $outdir/pmcstep_${tag}_fetch $outdir/pmcstep_${tag}_write 3 $outdir/pmcstep_${tag}.json > $outdir/pmcstep_${tag}.txt
head -40 $outdir/pmcstep_${tag}.txt
