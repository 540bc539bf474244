#!/bin/bash
# The parity suite under every diagnostic toggle of the engine (each run: a fresh process with the variable set globally).
#   bash tools/toggle_matrix.sh [TOGGLE=VALUE ...]       (about 40 s per toggle; no arguments: all of them)
# A run that ends on a time limit or a signal (a fault, an abort) ends the matrix: nothing more is started on that GPU.
set -u
ROOT=${GRAFT_REPO_ROOT:-$(cd "$(dirname "$0")/.." && pwd)}
OUT=$ROOT/gpurun_out/toggles
mkdir -p $OUT
cd $ROOT
[ $# -gt 0 ] || set -- "PAL_FUSED=0" "PAL_PFA=0" "PAL_FOUR_REG=0" "PAL_XCD_ROWS=0" "PAL_PFA_BIG=0" "PAL_OVERLAP=0" "PAL_RADER=0" "PAL_PFA_FWD=0" "PAL_RADIX3=0" "PAL_FIN=0" "PAL_R89=0" "PAL_FIN_SERIAL=1" "PAL_LEAN_STORE=0" "PAL_ROWS_LEAN=0"
for t in "$@"; do
  name=$(echo $t | tr '=' '_')
  env $t timeout -k 10 600 python -m pytest tests/test_gpu_parity.py tests/test_gpu_stream.py -m gpu -q -p no:cacheprovider > $OUT/$name.log 2>&1
  rc=$?
  echo "$t rc=$rc $(grep -E "passed|failed" $OUT/$name.log | tail -1)"; grep -E "^FAILED" $OUT/$name.log | cut -c1-150
  [ $rc -lt 124 ] || { echo "stopped after $t (rc=$rc)"; exit $rc; }
done
