#!/bin/bash
# time every build/ab/*/libbedgpu.so on the loader stage (GPU box); prints kernel avg per variant
cd $GRAFT_REPO_ROOT
BO=${OUT_DIR:-bench_out}; mkdir -p $BO
for d in build/ab/*/; do
  n=$(basename $d)
  BEDGPU_LIB=$d/libbedgpu.so timeout -k 10 200 python3 bench.py --full --load-only --steps ${STEPS:-6} --warmup 1 --no-verify --no-cpu-baseline > $BO/ab_$n.json 2> $BO/ab_$n.err || { echo "$n FAILED"; exit 1; }
  python3 -c "import json;d=json.load(open('$BO/ab_$n.json'));r=d['roofline'];print('%-12s %s avg %.4f ms  frac %.3f  step %.3f'%('$n',r['kernel'],r['avg_ms'],r['frac'],d['ms_per_step']))"
done
