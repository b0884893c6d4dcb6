#!/bin/bash
# rocprofv3 kernel trace of the fp32 parity path on one stream (bench.py --full --dtype f32 --streams 1): the per-step kernel
# table ($O/<TAG>_steps_f32.txt).
R=$(cd "$(dirname "$0")/.." && pwd); O=${DAMVS_OUT:-bench_out}; mkdir -p $R/$O
T=${TAG:-prof_f32}
cd /tmp && export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $R/$O/${T}_q -o run -- python $R/bench.py --full --dtype f32 --streams 1 --steps 5 --warmup 2 --no-cpu-baseline --no-shard-latency > $R/$O/${T}_q.log 2>&1 || exit $?
cd $R && python tools/prof_steps.py $O/${T}_q/run_kernel_trace.csv > $O/${T}_steps_f32.txt && head -45 $O/${T}_steps_f32.txt
