# GPU parity suite + smoke + one bench line (no profiling passes)
cd $GRAFT_REPO_ROOT
export TMPDIR=/tmp
TAG=${TAG:-rx}
OUT=${OUT:-bench_out}   # where the logs go
mkdir -p $OUT
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > $OUT/${TAG}_tests.log 2>&1 || { echo TESTS FAILED; tail -30 $OUT/${TAG}_tests.log; exit 1; }
tail -1 $OUT/${TAG}_tests.log
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/${TAG}_smoke.log 2>&1 || { echo SMOKE FAILED; tail -20 $OUT/${TAG}_smoke.log; exit 1; }
tail -1 $OUT/${TAG}_smoke.log
timeout -k 10 600 python bench.py --full $BENCH_ARGS --kernel-report $OUT/${TAG}_kreport.json > $OUT/${TAG}_bench.log 2>&1 || { echo BENCH FAILED; tail -20 $OUT/${TAG}_bench.log; exit 1; }
tail -1 $OUT/${TAG}_bench.log
