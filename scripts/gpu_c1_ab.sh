#!/bin/bash
# C1 insert ablations (experiment build): DBG_X_SHORT 1 = full, 3 = no flush, 4 = no adds / flush,
# 5 = loads + predicate only.  Each variant writes to gpu_cfg.sh's default folder for the config.
export DBGPU_LIB=$PWD/databend_amd/libdbgpu_agg_exp.so
for v in ${VARIANTS:-1 3 4 5}; do
  DBG_X_SHORT=$v CFG=1 STEPS=200 WARM=20 NO_PROF=1 bash scripts/gpu_cfg.sh | grep cfg | sed "s/^/short=$v /" || exit 1
done
