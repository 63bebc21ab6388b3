#!/bin/bash
# BASELINE configs[3] / configs[4] (OCTO-base 2-cam, OCTO-base hi-res ToMe r=32 fp8) at B = 32:
# bench lines (with the block-0 probes, incl. the fp8 GEMM probe and its bf16 twin), the fp8 path
# A/B (--set fp8=0), and rocprofv3 kernel stats of each step (logs under $OUT, default bench_out)
set -o pipefail
export TMPDIR=/tmp
OUT=${OUT:-bench_out}
mkdir -p $OUT
P="--batch 32"                        # plain runs: the step alone
B="$P --full --no-cpu-baseline"       # with the kernel probes
timeout -k 10 400 python bench.py --config octo-base-2cam $B --steps 30 --warmup 5 > $OUT/base2cam.log 2>&1 &&
timeout -k 10 400 python bench.py --config octo-base-hires-tome32 $B --steps 30 --warmup 5 > $OUT/hires.log 2>&1 &&
timeout -k 10 400 python bench.py --config octo-base-hires-tome32 $P --steps 30 --warmup 5 --set fp8=0 > $OUT/hires_bf16.log 2>&1 &&
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $OUT/prof_base2cam -o run --output-format csv -- python bench.py --config octo-base-2cam $P --steps 5 --warmup 2 > $OUT/prof_base2cam.log 2>&1 &&
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $OUT/prof_hires -o run --output-format csv -- python bench.py --config octo-base-hires-tome32 $P --steps 5 --warmup 2 > $OUT/prof_hires.log 2>&1
