#!/bin/bash
# usage: [PMC_DIM=128] tools/pmc.sh <outdir> <counters...> -- runs the reduced bench under rocprofv3 --pmc
tag=$1; shift
cd /tmp && export TMPDIR=/tmp && cd "${GRAFT_REPO_ROOT:?run on the GPU box through gpurun}" || exit 1
out=${EACHAM_OUT_DIR:-results}; mkdir -p "$out"   # results of this script (EACHAM_OUT_DIR, default results/)
rocprofv3 --pmc "$@" --kernel-trace --output-format csv -d $out/$tag -- python3 bench.py --full --steps 2 --warmup 1 --frames 64 --landmarks 16000 --dim ${PMC_DIM:-256} --cpu-pairs 0 --ba-solves 1 --lines none > $out/$tag.log 2>&1
echo "exit $?"
