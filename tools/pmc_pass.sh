#!/bin/bash
# One rocprofv3 --pmc pass per argument (a quoted, space-separated counter group) over a short bench run; prints
# per-launch means of render_wavefront_kernel.  Run from the repo root ON THE GPU BOX.  Counters are collected in runs of
# their own: no trace domain beside --pmc (tools/summarize_pmc.py reads only the *counter_collection.csv files).
# usage: [OUT=<directory for the results, default profile_out>] tools/pmc_pass.sh TAG "CTR_A CTR_B" "CTR_C" ...
TAG=${1:?tag}; shift
R=$PWD
OUT=${OUT:-$R/profile_out}
case $OUT in /*) ;; *) OUT=$R/$OUT;; esac
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
i=0
for c in "$@"; do
  i=$((i+1))
  rocprofv3 --pmc $c --output-format csv -d $OUT/pmcx_$TAG -o g$i -- python3 $R/bench.py --steps 2 --warmup 1 --no-cpu-baseline ${BENCH_ARGS} > $OUT/pmcx_${TAG}_g$i.log 2>&1 || echo "pass '$c' failed: $(tail -2 $OUT/pmcx_${TAG}_g$i.log | cut -c1-300)"
done
cd $R
python3 tools/summarize_pmc.py $OUT/pmcx_$TAG > $OUT/pmcx_$TAG.json
python3 - <<PY
import json; d=json.load(open('$OUT/pmcx_$TAG.json'))
for k,v in d.items():
    if isinstance(v, dict) and 'per_launch_mean' in v: print(k, '%.4g'%v['per_launch_mean'])
PY
