#!/bin/bash
# round-3 final measurement set: everything lands in $O (the output directory the caller names), copied to profiles/ afterwards
O=$(realpath -m "${O:?set O to the output directory}")
R=$PWD
mkdir -p $O
python bench.py --full --dtype fp8 --steps 3 --warmup 1 --by-shape $O/r03_by_shape_fp8_v1.txt > $O/r03_bench_fp8_v1.json 2> $O/r03_bench_fp8_v1.err
tail -c 600 $O/r03_bench_fp8_v1.json | head -c 300; echo
python bench.py --full --steps 3 --warmup 1 --by-shape $O/r03_by_shape_fp16_v2.txt > $O/r03_bench_fp16_v3.json 2> $O/r03_bench_fp16_v3.err
head -c 400 $O/r03_bench_fp16_v3.json; echo
python tools/bench_extras.py config4 --dtype fp16 > $O/r03_bench_extras.jsonl 2> $O/r03_bench_extras.err
python tools/bench_extras.py config4 --dtype fp8 >> $O/r03_bench_extras.jsonl 2>> $O/r03_bench_extras.err
cat $O/r03_bench_extras.jsonl | cut -c 1-220
timeout 300 python tools/vs_hipblaslt.py --rounds 3 > $O/r03_vs_hipblaslt_v3.log 2>&1
tail -11 $O/r03_vs_hipblaslt_v3.log
python tools/attn_bench.py > $O/r03_attn_bench.log 2>&1; tail -7 $O/r03_attn_bench.log
cd /tmp && export TMPDIR=/tmp
timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $O/r03_rocprof -o r03 -- python $R/bench.py --steps 1 --warmup 0 --no-cpu-baseline --no-roofline --no-graph --dedup-steps 0 > $O/r03_rocprof_bench.log 2>&1
ls -R $O/r03_rocprof | head;
f=$(find $O/r03_rocprof -name "*kernel_stats.csv" | head -1); head -12 "$f"
# keep only the stats (the trace itself is hundreds of MB)
find $O/r03_rocprof -name "*kernel_trace.csv" -delete
find $O/r03_rocprof -name "*.db" -delete
