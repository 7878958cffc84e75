#!/bin/bash
# C2 phase trace: the fused insert+finalize launch's timestamps (DBG_X_TRACE, medians over launches),
# where each launch starts against the one before it, and the host's turn between batches.
#   scripts/gpu_trace_c2.sh [dual|single|pool]   (the pipeline mode, passed on as DBG_PIPE_MODE)
# Needs a library built with phase tracing:
#   make -C databend_amd/csrc TRACE=1
# (it builds databend_amd/libdbgpu_agg_exp.so; the shipped library is untouched).  DBGPU_TRACE_LIB
# names another such build, DBG_TRACE_OUT another output folder than bench_out/.
set -o pipefail
MODE=${1:-dual}
case "$MODE" in dual|single|pool) ;; *) echo "usage: $0 [dual|single|pool]"; exit 2;; esac
ROOT=$(cd "$(dirname "$0")/.." && pwd)
cd "$ROOT"
DIR=${DBG_TRACE_OUT:-bench_out}
mkdir -p "$DIR"
LIB=${DBGPU_TRACE_LIB:-$ROOT/databend_amd/libdbgpu_agg_exp.so}
OUT=$DIR/trace_c2_$MODE
DBG_PIPE_MODE=$MODE DBG_X_TRACE=1 DBGPU_LIB=$LIB timeout -k 10 120 python -u bench.py --config 2 --steps 200 --warmup 10 --no-cpu-baseline --extra-configs none \
  > $OUT.json 2> $OUT.err || { echo "trace failed"; tail -20 $OUT.err; exit 1; }
grep trace $OUT.err
cut -c1-300 $OUT.json
