#!/bin/bash
# GPU visit: kernel + parity tests (detail log), rocprofv3 kernel stats of the eager step, benches.
set -u
export KG_OUT=${KG_OUT:-runs}; OUT=$KG_OUT      # output folder, relative to the repository root
mkdir -p $OUT
export TMPDIR=/tmp
python -c "import __graft_entry__ as g; g.build()" > $OUT/build.log 2>&1
rm -f $OUT/parity_detail.log
timeout 600 python -m pytest tests/test_kernels_gpu.py -q -m gpu --tb=short -p no:cacheprovider > $OUT/kernels.log 2>&1
echo "kernels rc=$?" >> $OUT/kernels.log; tail -15 $OUT/kernels.log
timeout 600 python -m pytest tests/test_parity_gpu.py -q -m gpu --tb=short -p no:cacheprovider > $OUT/parity.log 2>&1
echo "parity rc=$?" >> $OUT/parity.log
tail -15 $OUT/parity.log
R=$(pwd)
cd /tmp
timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $R/$OUT/prof_eager -o r01 -- python3 $R/bench.py --full --steps 3 --warmup 2 --no-graph --no-cpu-baseline --no-roofline --no-extras > $R/$OUT/prof_eager.log 2>&1
echo "prof rc=$?"
cd $R
find $OUT/prof_eager -type f | head
find $OUT/prof_eager -type f ! -name "*stats*" -delete
timeout 400 python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline > $OUT/bench_graph.log 2>&1; tail -2 $OUT/bench_graph.log
