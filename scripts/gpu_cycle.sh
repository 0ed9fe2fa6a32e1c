#!/bin/bash
# One GPU cycle: parity tests, bench line, single-stream per-kernel trace.  Usage: scripts/gpu_cycle.sh TAG OUT_DIR
TAG=$1
R=$GRAFT_REPO_ROOT
O=${2:?usage: scripts/gpu_cycle.sh TAG OUT_DIR}; mkdir -p $O
timeout -k 10 600 python -m pytest tests -m gpu -x -q > $O/${TAG}_gpu_tests.log 2>&1 || { tail -30 $O/${TAG}_gpu_tests.log; exit 1; }
tail -1 $O/${TAG}_gpu_tests.log
timeout -k 10 900 python bench.py --full > $O/${TAG}_bench.json 2> $O/${TAG}_bench.err || { tail $O/${TAG}_bench.err; exit 1; }
python - <<PY
import json
d=json.load(open('$O/${TAG}_bench.json'))
print('reads/s', d['value'], 'ms/step', d['ms_per_step'], 'fill alone ms', d['valu_roofline']['launch_ms_alone'])
PY
cd /tmp && export TMPDIR=/tmp
WSX_STREAMS=1 timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/${TAG}_prof -o p -- python3 $R/bench.py --steps 3 --warmup 1 > $O/${TAG}_prof.log 2>&1
python3 $R/scripts/kstats.py $O/${TAG}_prof/p_kernel_trace.csv 5
