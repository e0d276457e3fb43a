#!/bin/bash
# round-4 evidence: full GPU tests, rocprofv3 stats + PMC passes, the default bench line, per-GPU-share sizes, long run, NVE run
set -uo pipefail
cd /tmp && export TMPDIR=/tmp && cd "${GRAFT_REPO_ROOT:?}" || exit 1
O=gpurun_out/r4final; mkdir -p $O
timeout -k 10 900 python -m pytest tests -m gpu -q > $O/gpu_tests.log 2>&1; tail -3 $O/gpu_tests.log
bash tools/profile_round.sh r04 > $O/profile_round.log 2>&1; tail -12 $O/profile_round.log
timeout -k 10 600 python bench.py --full > $O/bench_default.json 2> $O/bench_default.err
for n in 12501 25002 50001; do timeout -k 10 300 python bench.py --full --no-cpu-baseline --no-dense-pass --no-extra --atoms $n > $O/bench_$n.json 2> $O/bench_$n.err; done
timeout -k 10 300 python bench.py --full --steps 20 --warmup 5 > $O/bench_steps20_warmup5.json 2> /dev/null
timeout -k 10 300 python tools/long_run.py > $O/md_long_run.json 2> $O/md_long_run.err
timeout -k 10 300 python tools/md_probe.py 100002 1000 0.25 1 300 > $O/md_nve_100k_1000steps.log 2>&1
timeout -k 10 300 python tools/members_probe.py "" > $O/members_probe.log 2>&1
echo done
