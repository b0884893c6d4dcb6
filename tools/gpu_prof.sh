#!/bin/bash
# 1) rocprofv3 kernel trace + stats of the default bench command (timed steps on 2 streams, attribution
#    pass on one): stats CSV, its bench line, and the roofline kernel's per-grid means (roofline_check.txt);
# 2) the same with --streams 1 for the per-step kernel table (steps.txt) and per-launch table (launches.txt).
R=$(cd "$(dirname "$0")/.." && pwd); O=${DAMVS_OUT:-bench_out}; mkdir -p $R/$O
cd /tmp && export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $R/$O/prof_default -o run -- python $R/bench.py --full --no-cpu-baseline > $R/$O/prof_default.log 2>&1 || exit $?
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $R/$O/prof_q -o run -- python $R/bench.py --full --streams 1 --steps 5 --warmup 2 --no-cpu-baseline > $R/$O/prof_q.log 2>&1 || exit $?
cd $R && python tools/prof_roofline_kernel.py $O/prof_default/run_kernel_trace.csv > $O/roofline_check.txt && \
  grep '^{"metric"' $O/prof_default.log | tail -1 | python -c 'import json,sys; d=json.loads(sys.stdin.read()); print("bench line (under rocprofv3): value %s, roofline ms_per_launch %s, isolated_ms_per_launch %s" % (d["value"], d["roofline"]["ms_per_launch"], d["roofline"]["isolated_ms_per_launch"]))' >> $O/roofline_check.txt && \
  python tools/prof_damvs_launches.py $O/prof_q/run_kernel_trace.csv 4 > $O/launches.txt && \
  python tools/prof_steps.py $O/prof_q/run_kernel_trace.csv > $O/steps.txt && cat $O/roofline_check.txt && head -3 $O/steps.txt
