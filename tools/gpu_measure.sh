#!/bin/bash
# Round-end measurement at the default batch: probe PMC traffic passes (FETCH_SIZE, WRITE_SIZE),
# the full bench line (probes + cpu_baseline) reading that traffic, and a kernel-trace profile of
# the step. Usage: tools/gpu_measure.sh TAG   (logs and traces under $OUT, default bench_out)
set -o pipefail
export TMPDIR=/tmp
TAG=${1:-r02_b512}
OUT=${OUT:-bench_out}
mkdir -p $OUT
if [ -z "$SKIP_PMC" ]; then  # SKIP_PMC=1: the bench / profile legs only (kernel sources unchanged)
timeout -k 10 200 python bench.py --probe-only > $OUT/${TAG}_probes.json 2> $OUT/${TAG}_probes.err &&
timeout -s KILL 200 rocprofv3 --pmc FETCH_SIZE --kernel-trace -d $OUT/${TAG}_pmc_fetch -o run --output-format csv -- python bench.py --probe-only > $OUT/${TAG}_pmc1.log 2>&1 &&
timeout -s KILL 200 rocprofv3 --pmc WRITE_SIZE --kernel-trace -d $OUT/${TAG}_pmc_write -o run --output-format csv -- python bench.py --probe-only > $OUT/${TAG}_pmc2.log 2>&1 &&
python tools/pmc_traffic.py $OUT/${TAG}_pmc_fetch $OUT/${TAG}_pmc_write --probes $OUT/${TAG}_probes.json --out $OUT/${TAG}_probe_pmc.json > $OUT/${TAG}_pmc3.log 2>&1 &&
cp $OUT/${TAG}_probe_pmc.json profiles/ || exit 1
fi
timeout -k 10 400 python bench.py --full > $OUT/${TAG}_bench.log 2>&1 &&
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $OUT/${TAG}_benchprof -o run --output-format csv -- python bench.py --full --no-cpu-baseline > $OUT/${TAG}_benchprof.log 2>&1 &&
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $OUT/${TAG}_prof -o run --output-format csv -- python bench.py --steps 6 --warmup 2 > $OUT/${TAG}_prof.log 2>&1
