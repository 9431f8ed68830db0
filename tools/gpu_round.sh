#!/bin/bash
# One GPU call of the build loop, every step under its own limit, stopping at the first failure:
#   bash tools/gpu_round.sh TAG [tests|suite|none] [bench|nobench] [prof|noprof] [pmc|nopmc]
# tests: the learner / chain tests ($TESTS overrides); suite: the whole -m gpu suite; then the whole bench
# line (bench.py --full), a rocprofv3 --kernel-trace --stats run of the plain bench with one graph-replayed
# step's window (tools/step_window.py), and optionally the PMC passes of tools/pmc_run.sh
# (tools/pmc_summary.py). Everything is written under $OUT (default bench_out/, ignored by git).
set -o pipefail
cd "$(dirname "$0")/.." || exit 1
OUT=$(realpath -m "${OUT:-bench_out}")
mkdir -p "$OUT"
export PYTHONUNBUFFERED=1
T=${1:-r04}
WHAT=${2:-tests}
TESTS=${TESTS:-"tests/test_chain_schedule_gpu.py tests/test_critic_fused_gpu.py tests/test_learner_golden_gpu.py"}
if [ "$WHAT" = suite ]; then
  timeout -k 10 1000 python -u -m pytest tests -m gpu -x -v --timeout 200 --timeout-method thread \
    > $OUT/${T}_pytest_gpu.log 2>&1 || { tail -30 $OUT/${T}_pytest_gpu.log; exit 2; }
  tail -3 $OUT/${T}_pytest_gpu.log
  timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke()" > $OUT/${T}_smoke.log 2>&1 || exit 2
elif [ "$WHAT" = tests ]; then
  timeout -k 10 700 python -u -m pytest -x -v --timeout 200 --timeout-method thread $TESTS \
    > $OUT/${T}_pytest.log 2>&1 || { tail -30 $OUT/${T}_pytest.log; exit 2; }
  tail -3 $OUT/${T}_pytest.log
fi
if [ "${3:-bench}" = bench ]; then
  timeout -k 10 400 python -u bench.py --steps 20 --warmup 5 --full > $OUT/${T}_bench.json 2> $OUT/${T}_bench.err \
    || { tail -20 $OUT/${T}_bench.err; exit 3; }
  python -c "import json; d=json.load(open('$OUT/${T}_bench.json')); print(d['ms_per_step'], d['value'], d['roofline']['ms_per_launch'], d['roofline']['frac'])"
fi
if [ "${4:-prof}" = prof ]; then
  R=$PWD
  (cd /tmp && export TMPDIR=/tmp && rm -rf $OUT/${T}_prof && \
   timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/${T}_prof -o run --output-format csv rocpd \
     -- python3 $R/bench.py --steps 50 --warmup 10 > $OUT/${T}_prof.json 2> $OUT/${T}_prof.err) || exit 4
  python tools/step_window.py $OUT/${T}_prof/run_results.db > $OUT/${T}_step_window.txt 2>&1
  head -20 $OUT/${T}_step_window.txt
fi
if [ "${5:-nopmc}" = pmc ]; then
  rm -rf $OUT/pmc
  BENCH_ARGS="--steps 10 --warmup 5" PMC_OUT="$OUT/pmc" \
    PMC_EXTRA=1 timeout -k 10 1200 bash tools/pmc_run.sh || exit 5
  python tools/pmc_summary.py $OUT/pmc --json $OUT/${T}_pmc_summary.json > $OUT/${T}_pmc_summary.txt 2>&1
fi
exit 0
