#!/bin/bash
# parity suite, then a short bench if the suite did not crash (rc 0 = pass, 1 = test failures)
cd "$GRAFT_REPO_ROOT" || exit 1
export OUT=${OUT:-bench_out}    # where the logs, traces and profiles go
mkdir -p ${OUT}
timeout -k 10 900 python -m pytest tests/test_gpu_parity.py -q -m gpu -p no:cacheprovider -x > ${OUT}/pytest_gpu.log 2>&1
rc=$?
echo "pytest rc=$rc"
tail -30 ${OUT}/pytest_gpu.log
if [ $rc -le 1 ]; then
  timeout -k 10 300 python bench.py --full --steps 3 --warmup 1 --no-cpu-baseline > ${OUT}/bench.log 2>&1
  echo "bench rc=$?"
  tail -5 ${OUT}/bench.log
fi
