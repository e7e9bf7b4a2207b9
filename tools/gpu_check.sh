#!/bin/bash
# One GPU session: parity tests, smoke, bench, rocprofv3 kernel stats.
# Every GPU step has its own time limit; steps are chained with && so the
# first failure ends the session.
set -o pipefail
R=${GRAFT_REPO_ROOT:-$(pwd)}
cd "$R"
mkdir -p bench_out
timeout -k 10 600 python -m pytest tests -m gpu -x -q > bench_out/pytest_gpu.log 2>&1 \
 && timeout -k 10 120 python -c "import __graft_entry__ as g; g.smoke()" > bench_out/smoke.log 2>&1 \
 && timeout -k 10 400 python bench.py --full --steps 20 --warmup 3 > bench_out/bench.log 2>&1 \
 && (cd /tmp && export TMPDIR=/tmp && timeout -k 10 300 rocprofv3 --kernel-trace --stats \
      --output-format csv -d "$R/bench_out/prof" -o run -- python "$R/bench.py" --full --steps 5 \
      --warmup 1 --no-cpu-baseline --no-secondary > "$R/bench_out/prof.log" 2>&1)
rc=$?
echo "session exit $rc"
tail -3 bench_out/pytest_gpu.log; tail -2 bench_out/smoke.log; tail -1 bench_out/bench.log
exit $rc
