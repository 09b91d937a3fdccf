# Round artefacts on one MI355X: GPU parity tests, smoke, bench (with CPU
# baseline), rocprofv3 kernel stats of the bench command, PMC HBM traffic passes.
# BENCH_ARGS="--image-model nest_small" gives the NesT (configs[3]) artefacts.
cd $GRAFT_REPO_ROOT
export TMPDIR=/tmp
TAG=${TAG:-r1}
OUT=${OUT:-bench_out}   # where the logs and profiles go
mkdir -p $OUT
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > $OUT/${TAG}_tests.log 2>&1 || { echo TESTS FAILED; tail -30 $OUT/${TAG}_tests.log; exit 1; }
tail -1 $OUT/${TAG}_tests.log
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/${TAG}_smoke.log 2>&1 || { echo SMOKE FAILED; tail -20 $OUT/${TAG}_smoke.log; exit 1; }
tail -1 $OUT/${TAG}_smoke.log
timeout -k 10 600 python bench.py --full $BENCH_ARGS --kernel-report $OUT/${TAG}_kreport.json > $OUT/${TAG}_bench.log 2>&1 || { echo BENCH FAILED; tail -20 $OUT/${TAG}_bench.log; exit 1; }
tail -1 $OUT/${TAG}_bench.log
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${TAG}_prof -o stats -- python bench.py --full $BENCH_ARGS --no-cpu-baseline --no-loss-check --pcie-steps 0 > $OUT/${TAG}_prof.log 2>&1 || { echo PROF FAILED; tail -20 $OUT/${TAG}_prof.log; exit 1; }
tail -1 $OUT/${TAG}_prof.log
timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/${TAG}_pmc -o fetch -- python bench.py --full $BENCH_ARGS --steps 2 --warmup 1 --no-cpu-baseline --no-loss-check --pcie-steps 0 > $OUT/${TAG}_pmcf.log 2>&1 || { echo PMC1 FAILED; tail -20 $OUT/${TAG}_pmcf.log; exit 1; }
timeout -k 10 300 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/${TAG}_pmc -o write -- python bench.py --full $BENCH_ARGS --steps 2 --warmup 1 --no-cpu-baseline --no-loss-check --pcie-steps 0 > $OUT/${TAG}_pmcw.log 2>&1 || { echo PMC2 FAILED; tail -20 $OUT/${TAG}_pmcw.log; exit 1; }
find $OUT/${TAG}_prof $OUT/${TAG}_pmc -name "*.csv" | head -20
