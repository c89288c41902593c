set -o pipefail
cd $GRAFT_REPO_ROOT
export OUT=${OUT:-bench_out}   # where the results go
mkdir -p $OUT
export TMPDIR=/tmp
mkdir -p $OUT/m1
timeout -k 10 300 python -u -m pytest tests/test_gpu_reuse.py tests/test_gpu_parity.py -x -q --timeout 200 --timeout-method thread > $OUT/m1/t.log 2>&1 || { tail -30 $OUT/m1/t.log; exit 1; }
tail -1 $OUT/m1/t.log
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/m1/prof -o t -- python3 bench.py --full --config c4 --global-batch 512 --steps 10 --warmup 3 --prof-steps 1 --no-cpu-baseline --no-secondary > $OUT/m1/prof.log 2>&1 || exit 1
