#!/bin/bash
OUT=gpurun_out/r04c; mkdir -p $OUT
for v in "graph 64" "eager 64" "eager 0" "graph 0"; do
  set -- $v
  echo "== MODE=$1 FLAGS=$2 (64 = TDRN_PLAN_NO_PP_SK: no chained split)" | tee -a $OUT/two.txt
  MODE=$1 FLAGS=$2 timeout 300 python scripts/dev/two_in_flight.py 2 2>&1 | grep -v amdgpu.ids | tail -6 | tee -a $OUT/two.txt
done
