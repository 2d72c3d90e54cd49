#!/bin/bash
# other BASELINE configs on one GPU + the 2-rank control flow (gloo on one GPU), default and exact-BN mode
set -u
export KG_OUT=${KG_OUT:-runs}; OUT=$KG_OUT      # output folder, relative to the repository root
mkdir -p $OUT
python -c "import __graft_entry__ as g; g.build()" > $OUT/build.log 2>&1 || { cat $OUT/build.log; exit 1; }
: > $OUT/r05_final_other_configs.log
for c in ${R4K_CONFIGS:-"stress 64" "ntu120 32" "h36m 64"}; do set -- $c
  echo "== --config $1 --batch $2" >> $OUT/r05_final_other_configs.log
  timeout 600 python bench.py --full --config $1 --batch $2 --steps 20 --warmup 5 --no-cpu-baseline --no-roofline --no-extras 2>&1 | tail -1 | cut -c1-700 >> $OUT/r05_final_other_configs.log
done
cat $OUT/r05_final_other_configs.log | cut -c1-260
export KG_BENCH_BACKEND=gloo KG_BENCH_DEVICE=0
: > $OUT/r05_dp2_one_gpu_gloo.log
for extra in "" "--exact-bn"; do
  echo "== 2 ranks on one GPU over gloo $extra" >> $OUT/r05_dp2_one_gpu_gloo.log
  timeout 300 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29577 bench.py --full --gpus 2 --steps 10 --warmup 3 --no-cpu-baseline --no-roofline --no-extras $extra 2>&1 | grep -v "amdgpu.ids\|Warning\|warn" | tail -2 | cut -c1-900 >> $OUT/r05_dp2_one_gpu_gloo.log
done
cat $OUT/r05_dp2_one_gpu_gloo.log | cut -c1-400
