#!/bin/bash
# tools/gpu_traffic.sh over every record config (PMC traffic + VALU issue counters), one call;
# tools/traffic_json.py reduces each config where it ran (the raw counter CSVs are large and are
# deleted), and the merged profiles/pmc_me_traffic.json is also left as
# $OUT/pmc_me_traffic.json.
cd "$GRAFT_REPO_ROOT" || exit 1
export OUT=${OUT:-bench_out}    # where the logs, traces and profiles go (tools/gpu_traffic.sh writes $OUT/traffic)
mkdir -p ${OUT}
T=${TAG:-r06c}
for cfg in ${CFGS:-4k 1080p 4k_vbs 4k_rc2pass 4k_noise 4k_lowtex}; do
  bash tools/gpu_traffic.sh $T $cfg || exit $?
  python3 tools/traffic_json.py ${OUT}/traffic $T $cfg > ${OUT}/traffic_json_$cfg.log 2>&1 || exit $?
  rm -rf ${OUT}/traffic/${T}_${cfg}_*
done
cp profiles/pmc_me_traffic.json ${OUT}/pmc_me_traffic.json
rm -rf ${OUT}/traffic
