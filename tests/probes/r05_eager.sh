#!/bin/bash
R=${GRAFT_REPO_ROOT:-$PWD}; O=$R/gpurun_out/r05_eager; mkdir -p $O; cd $R
export MXF_GP_LIB=$R/mxfusion_amd/libmxf_gp_probe.so
for rep in 1 2; do for e in 0 2 3 4 8; do
  echo "eager=$e: $(MXF_POTRF_EAGER_INV=$e python bench.py --workload gp --dtype float64 --N 8192 --steps 8 --warmup 3 --no-cpu-baseline 2>/dev/null | python -c "import sys,json; d=json.loads(sys.stdin.readlines()[-1]); print(round(d['ms_per_step'],3))")"
done; done 2>&1 | tee $O/eager3.log
