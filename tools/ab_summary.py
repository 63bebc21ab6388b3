"""Summary of tools/gpu_step_ab.sh logs: step value and probe launch times per build and round.
Usage: ab_summary.py TAG   (reads the logs under $OUT, default bench_out, as the script wrote them)"""
import glob
import json
import os
import sys

tag = sys.argv[1]
out = os.environ.get("OUT", "bench_out")
for f in sorted(glob.glob(f"{out}/{tag}_*[0-9].log")):
    for line in open(f):
        if line.startswith("{"):
            d = json.loads(line)
            ks = (d.get("roofline") or {}).get("kernels", [])  # null without bench.py --full
            print(f"{f.split('/')[-1]:28s} {d['value']:9.1f}  " +
                  " ".join(f"{k['name']}={k['avg_launch_us']:.1f}" for k in ks))
for f in sorted(glob.glob(f"{out}/{tag}_t5*.log")):
    print(f, [l.strip() for l in open(f) if "T5" in l])
