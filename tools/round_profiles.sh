#!/bin/bash
# Everything the round's committed profiles / bench lines come from, in one GPU call.  usage: bash tools/round_profiles.sh <tag> [bench line dir, default bench_lines]
# Afterwards, locally: python tools/summarize_prof.py <tag> <label>; python tools/traffic.py <tag> <label>; copy the stats CSVs / JSON lines.
TAG=${1:-r04}
R=${GRAFT_REPO_ROOT:-$(pwd)}
cd $R
OUT=${2:-bench_lines}  # the bench JSON lines; the sampling ones run --full for the roofline, box_mfma_tfps and secondary legs
mkdir -p $OUT
bash tools/prof.sh ${TAG} > gpurun_out/${TAG}_prof.log 2>&1
bash tools/prof_train.sh ${TAG}t > /dev/null 2>&1
bash tools/prof_sample.sh ${TAG}i --model iddpm64 --batch 32 > /dev/null 2>&1
bash tools/prof_train.sh ${TAG}it --model iddpm64 --batch 32 > /dev/null 2>&1
bash tools/prof_sample.sh ${TAG}x --precision bf16x3 > /dev/null 2>&1
bash tools/prof_sample.sh ${TAG}r --precision fp16r32 > /dev/null 2>&1
bash tools/prof_train.sh ${TAG}th --precision fp16 > /dev/null 2>&1
python bench.py --full --steps 100 --warmup 20 > $OUT/${TAG}_bench_n1.json 2> $OUT/${TAG}_bench_n1.err
python bench.py --full --mode ddim --batch 512 --steps 50 --warmup 10 --no-cpu-baseline --no-accurate-leg --train-steps 0 > $OUT/${TAG}_bench_ddim_b512_n1.json 2>/dev/null
python bench.py --mode train --steps 50 --warmup 5 > $OUT/${TAG}_bench_train_n1.json 2>/dev/null
python bench.py --full --model iddpm64 --batch 32 --steps 50 --warmup 10 --no-cpu-baseline --no-accurate-leg --train-steps 0 > $OUT/${TAG}_bench_iddpm64_b32_n1.json 2>/dev/null
python bench.py --model iddpm64 --batch 32 --mode train --steps 30 --warmup 5 > $OUT/${TAG}_bench_iddpm64_train_b32_n1.json 2>/dev/null
python bench.py --full --precision bf16x3 --steps 20 --warmup 5 --no-cpu-baseline --train-steps 0 > $OUT/${TAG}_bench_x3_n1.json 2>/dev/null
python bench.py --full --precision fp16r32 --steps 50 --warmup 10 --no-cpu-baseline --train-steps 0 > $OUT/${TAG}_bench_fp16r32_n1.json 2>/dev/null
python bench.py --full --model iddpm64 --batch 32 --precision fp16r32 --steps 50 --warmup 10 --no-cpu-baseline --no-accurate-leg --train-steps 0 > $OUT/${TAG}_bench_iddpm64_fp16r32_b32_n1.json 2>/dev/null
python bench.py --mode train --precision fp16 --steps 50 --warmup 5 > $OUT/${TAG}_bench_train_fp16_n1.json 2>/dev/null
python bench.py --full --precision fp32 --steps 10 --warmup 3 --no-cpu-baseline --train-steps 0 > $OUT/${TAG}_bench_fp32_n1.json 2>/dev/null
for b in 1 32; do python bench.py --full --batch $b --steps 300 --warmup 30 --no-cpu-baseline --no-accurate-leg --train-steps 0 > $OUT/${TAG}_bench_b${b}_n1.json 2>/dev/null; done
ls -la $OUT/${TAG}_bench_*.json | awk '{print $5, $9}'
du -sh gpurun_out/prof_${TAG}* | tail -12
