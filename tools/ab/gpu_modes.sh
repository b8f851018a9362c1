#!/bin/bash
# The other bench modes at the default batch: ct x pt diagonals, and the row-sharded (cfg4) leg at world 1.
# usage: bash tools/gpu_modes.sh <tag>
set -o pipefail
OUT=${OUT:-results}  # where the logs and bench lines go
cd $GRAFT_REPO_ROOT
T=$1
mkdir -p $OUT/$T
timeout -k 10 400 python bench.py --full --variant ctpt --no-cpu-baseline > $OUT/$T/ctpt.json 2> $OUT/$T/ctpt.err || { tail $OUT/$T/ctpt.err; exit 1; }
tail -1 $OUT/$T/ctpt.json | cut -c1-250
timeout -k 10 500 python bench.py --full --mode sharded --no-cpu-baseline > $OUT/$T/sharded1.json 2> $OUT/$T/sharded1.err || { tail $OUT/$T/sharded1.err; exit 1; }
tail -1 $OUT/$T/sharded1.json | cut -c1-250
python3 -c "
import json; d=json.loads(open('$OUT/$T/sharded1.json').read().strip().splitlines()[-1]); print(d.get('sharded'), d['roofline']['frac'])"
