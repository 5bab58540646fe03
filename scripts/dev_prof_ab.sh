#!/bin/bash
# dev helper: rocprofv3 kernel stats of the graph-replayed bench for TG_GEMM_FLAGS variants + clock / power samples of un-profiled runs
#   scripts/dev_prof_ab.sh "0 0x401" [output folder, default /tmp/dev_prof_ab]
R=${GRAFT_REPO_ROOT:-/root/repo}
O=$(realpath -m "${2:-/tmp/dev_prof_ab}"); mkdir -p $O
cd /tmp && export TMPDIR=/tmp
for v in $1; do
  ( while true; do rocm-smi --showclocks --showpower --json 2>/dev/null | head -c 2000; echo; sleep 0.5; done ) > $O/smi_$v.log 2>&1 &
  SMI=$!
  TG_GEMM_FLAGS=$v timeout 600 python $R/bench.py --full --steps 4 --warmup 1 --no-cpu-baseline --no-roofline 2>/dev/null | tail -1 > $O/ab_$v.json
  kill $SMI
  TG_GEMM_FLAGS=$v timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_$v -- \
    python $R/bench.py --full --steps 1 --warmup 1 --ddim-steps 10 --no-cpu-baseline --no-roofline > $O/prof_$v.log 2>&1
done
