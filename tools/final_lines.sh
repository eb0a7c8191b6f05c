#!/bin/bash
# Run ON the GPU box (through gpurun): the bench lines that go to profiles/ -- the driver's command, one pass over the ring, synchronous delivery, the other workloads.
cd $GRAFT_REPO_ROOT
o=${1:?usage: tools/final_lines.sh <output directory>}; mkdir -p $o
timeout 600 python3 bench.py --gpus 1 --steps 20 --warmup 5 --full 2>$o/driver.err | tail -1 > $o/driver_bench_line.json
timeout 600 python3 bench.py --full 2>$o/default.err | tail -1 > $o/default_bench_line.json
timeout 300 python3 bench.py --sync --full --no-cpu-baseline --no-also 2>/dev/null | tail -1 > $o/sync_bench_line.json
rm -f $o/other_workloads.jsonl
for w in cfg1 cfg2 cfg3 cfg5; do timeout 400 python3 bench.py --workload $w --steps 40 --warmup 5 --full --no-cpu-baseline --no-also 2>/dev/null | tail -1 >> $o/other_workloads.jsonl; done     # (each line: exact `value` + a `fast` block)
python3 - <<P
import json
for f in ("driver", "default", "sync"):
    d = json.load(open(f"$o/{f}_bench_line.json")); r = d["roofline"]
    print(f, d["value"], d["ms_per_step"], "fast", (d.get("fast") or {}).get("value"), (d.get("fast") or {}).get("ms_per_step"), r["kernel"], r["avg_launch_ms"], r.get("n_samples"), r.get("rocprof_avg_launch_ms"), "e2e", d["pipeline"]["hbm_frac_end_to_end"], "also", (d.get("also") or {}).get("value"), "cpu", (d.get("cpu_baseline") or {}).get("value"), (d.get("cpu_baseline") or {}).get("gpu_matches_oracle_on_sample"))
for l in open("$o/other_workloads.jsonl"):
    d = json.loads(l); print(d["config"]["workload"][:6], d["value"], d["ms_per_step"], d["pipeline"]["launch_path"], "fast", (d.get("fast") or {}).get("value"), (d.get("fast") or {}).get("ms_per_step"))
P
