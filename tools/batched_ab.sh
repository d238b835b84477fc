#!/bin/bash
# A/B of the batched GEMM kernels in one box: per-dispatch durations from rocprofv3 --kernel-trace
#   lds    - the planned cut (one launch of gemm_batched_cols_kernel per layer where a height fills whole rounds)
#   legacy - BVC_TILE_CUT=legacy: 128-row tiles of gemm_batched_lds_kernel plus the tail launch (the cut of before the plan)
#   nolds  - the register-only kernel
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
for v in lds legacy nolds; do
  unset BVC_TILE_CUT
  if [ $v = legacy ]; then export BVC_TILE_CUT=legacy; fi
  if [ $v = nolds ]; then export BVC_NO_LDS_GEMM=1; fi
  timeout -k 10 300 rocprofv3 --kernel-trace -f csv -d gpurun_out/bt_$v -o bt -- python3 tools/batched_trace.py > gpurun_out/bt_$v.log 2>&1 || exit 1
  echo "== $v"; grep -E "gemm_batched" gpurun_out/bt_$v/bt_kernel_trace.csv | python3 -c "
import sys,csv
for row in csv.reader(sys.stdin):
    nm=[c for c in row if 'bvc::' in c][0][10:40]
    nums=[int(c) for c in row if c.isdigit() and len(c)>12]
    print(nm, (nums[1]-nums[0])/1e3)
" | tail -8
  rm -rf gpurun_out/bt_$v
done
