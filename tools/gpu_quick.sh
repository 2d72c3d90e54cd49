#!/bin/bash
# quick visit: build, parity tests, eager kernel stats + last-step timeline, hipGraph bench line
set -u
export KG_OUT=${KG_OUT:-runs}; OUT=$KG_OUT      # output folder, relative to the repository root
TAG=${1:-r02}
mkdir -p $OUT
export TMPDIR=/tmp
python -c "import __graft_entry__ as g; g.build()" > $OUT/build.log 2>&1 || { cat $OUT/build.log; exit 1; }
rm -f $OUT/parity_detail.log
if [ "${SKIP_TESTS:-0}" != "1" ]; then
timeout 900 python -m pytest tests/test_kernels_gpu.py -q -m gpu --tb=short -p no:cacheprovider -x > $OUT/kernels.log 2>&1
echo "kernels rc=$?" >> $OUT/kernels.log; tail -5 $OUT/kernels.log
timeout 900 python -m pytest tests/test_parity_gpu.py -q -m gpu --tb=short -p no:cacheprovider > $OUT/parity.log 2>&1
echo "parity rc=$?" >> $OUT/parity.log; tail -15 $OUT/parity.log
fi
R=$(pwd)
cd /tmp
timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $R/$OUT/prof_eager -o $TAG -- python3 $R/bench.py --full --steps 3 --warmup 2 --no-graph --no-cpu-baseline --no-roofline --no-extras > $R/$OUT/prof_eager.log 2>&1
echo "prof rc=$?"
cd $R
python tools/last_step.py $OUT/prof_eager/${TAG}_kernel_trace.csv > $OUT/${TAG}_last_step.txt 2> $OUT/last_step.err; tail -3 $OUT/${TAG}_last_step.txt
cp $OUT/prof_eager/${TAG}_kernel_stats.csv $OUT/${TAG}_eager_kernel_stats.csv
find $OUT/prof_eager -type f ! -name "*stats*" -delete
timeout 600 python bench.py --full --steps 50 --warmup 10 --no-cpu-baseline > $OUT/bench_graph.log 2>&1; tail -1 $OUT/bench_graph.log
