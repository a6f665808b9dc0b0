#!/bin/bash
# Final round-3 profiles (one gpurun call): headline bench with trace / HBM traffic / SQ counters, the 54 x 144 stress
# leg and the jpl52 x 24 leg (both long-horizon kernel, scalar-resident descriptor since the store-hazard fix).
set -o pipefail
export TMPDIR=/tmp
cd "${GRAFT_REPO_ROOT:-.}"
PMC_SQ=1 bash tools/profile_r03.sh r03e_bench bench.py --full --steps 16 --warmup 8 --no-cpu-baseline --no-other-configs || exit 1
OUT=gpurun_out/prof_r03e_bench
rocprofv3 --pmc SQ_WAIT_INST_ANY SQ_WAIT_INST_LDS SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_INSTS_VMEM SQ_ACTIVE_INST_SCA SQ_INSTS_MFMA SQ_VALU_MFMA_BUSY_CYCLES --output-format csv -d $OUT/pmc_sq2 -- python3 bench.py --full --steps 16 --warmup 8 --no-cpu-baseline --no-other-configs > $OUT/out_sq2.json 2> $OUT/sq2.err || exit 1
echo "sq2 rc=$?"
bash tools/profile_r03.sh r03e_stress tools/run_config.py stress144 || exit 1
bash tools/profile_r03.sh r03e_cfg2j tools/run_config.py cfg2-jpl || exit 1
