#!/bin/bash
# One GPU call: a -k subset of the -m gpu suite, then bench.py on one config (its own limits).
#   PYK="two_pass or rc2pass" CFG=4k_rc2pass TAG=x bash tools/gpu_quick.sh
cd "$GRAFT_REPO_ROOT" || exit 1
export TMPDIR=/tmp
export OUT=${OUT:-bench_out}    # where the logs, traces and profiles go
mkdir -p ${OUT}
T=${TAG:-quick}
if [ -n "$PYK" ]; then
  timeout -k 10 600 python -u -m pytest tests -x -q -m gpu -k "$PYK" --timeout 200 --timeout-method thread \
      -p no:cacheprovider > ${OUT}/pytest_${T}.log 2>&1
  rc=$?; echo "pytest rc=$rc"; tail -3 ${OUT}/pytest_${T}.log; [ $rc -ne 0 ] && exit $rc
fi
for c in ${CFG:-4k}; do
  timeout -k 10 300 python -u bench.py --full --config $c --no-cpu-baseline --no-pcie --no-records ${BENCH_ARGS} \
      --detail-out ${OUT}/${T}_$c.json > ${OUT}/bench_${T}_$c.log 2>&1
  rc=$?; echo "bench $c rc=$rc"; [ $rc -ne 0 ] && { tail -5 ${OUT}/bench_${T}_$c.log; exit $rc; }
  python3 -c "import json; d=json.loads(open('${OUT}/bench_${T}_$c.log').read().strip().splitlines()[-1]); print('$c', d['ms_per_step'], d['parity'], d['roofline'])"
done
