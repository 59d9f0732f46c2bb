#!/bin/bash
# Collects the rocprofv3 evidence behind bench.py's numbers on the GPU box and writes the summaries to
# gpurun_out/profile/ (copy what should be judged into profiles/<round>/).  Three runs, as the profiling rules ask:
# kernel trace + stats, then one --pmc pass per HBM counter.  Usage: bash tools/profile_round.sh
set -e
R=${GRAFT_REPO_ROOT:-$(cd "$(dirname "$0")/.." && pwd)}
OUT=$R/gpurun_out/profile
mkdir -p "$OUT"
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/stats" -- python3 "$R/bench.py" --full --skip-cpu --skip-configs > "$OUT/bench_stats.log" 2>&1
rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d "$OUT/fetch" -- python3 "$R/bench.py" --full --steps 3 --warmup 1 --skip-cpu --skip-configs > "$OUT/bench_fetch.log" 2>&1
rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d "$OUT/write" -- python3 "$R/bench.py" --full --steps 3 --warmup 1 --skip-cpu --skip-configs > "$OUT/bench_write.log" 2>&1
rocprofv3 --pmc SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU --kernel-trace --output-format csv -d "$OUT/sq" -- python3 "$R/bench.py" --full --steps 3 --warmup 1 --skip-cpu --skip-configs > "$OUT/bench_sq.log" 2>&1
rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/detector" -- python3 "$R/tools/bench_detector.py" > "$OUT/detector.log" 2>&1
python3 - "$OUT" <<'PY'
import csv, glob, json, os, sys
out = sys.argv[1]
newest = lambda pat: max(glob.glob(os.path.join(out, pat)), key=os.path.getmtime)
# kernel stats of the bench run
os.replace(newest("stats/*/*_kernel_stats.csv"), os.path.join(out, "bench_kernel_stats.csv"))
rows = [r for r in csv.DictReader(open(newest("stats/*/*_kernel_trace.csv"))) if "trace_kernel" in r["Kernel_Name"]]
main = rows[0]["Kernel_Name"]  # the timed configuration comes first; the secondary no_pol launches follow it
rows = [r for r in rows if r["Kernel_Name"] == main]
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
ms = [round((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6, 4) for r in rows]
# launch order of bench.py: 1 small set-up trace, S settle traces (set-up, untimed: `settle_launches` of the JSON line),
# W warm-up traces, K timed traces (Raytracer.trace), then raw back-to-back launches and one more trace for the detector image
log = open(os.path.join(out, "bench_stats.log")).read().splitlines()
line = [l for l in log if l.startswith("{")]
if not line:  # bench.py failed under the profiler: say so instead of dying on an index
    sys.exit("no JSON line in bench_stats.log; its tail:\n" + "\n".join(log[-15:]))
bl = json.loads(line[-1])
i0 = 1 + int(bl.get("settle_launches", 0)) + int(bl["warmup"])
assert i0 + int(bl["steps"]) <= len(ms), f"{len(ms)} traced launches of {main[:40]}, the timed window ends at {i0 + int(bl['steps'])}"
timed = ms[i0:i0 + int(bl["steps"])]
json.dump({"command": "rocprofv3 --kernel-trace --stats --output-format csv -- python3 bench.py --full --skip-cpu --skip-configs   (1 set-up + settle + warm-up + timed Raytracer.trace calls, then raw launches + 1; counts in bench_line)",
           "timed_launch_index_range": [i0, i0 + int(bl["steps"])],
           "kernel": rows[0]["Kernel_Name"][:40], "launch_ms": ms, "timed_mean_ms": sum(timed) / len(timed),
           "bench_line": bl}, open(os.path.join(out, "trace_kernel_launches.json"), "w"), indent=1)
pmc = {"rays": 10000000, "pol": True, "unit": "KB per launch",
       "command": "rocprofv3 --pmc FETCH_SIZE (and, separately, --pmc WRITE_SIZE) --kernel-trace --output-format csv -- python3 bench.py --full --steps 3 --warmup 1 --skip-cpu --skip-configs"}
for name, d in (("FETCH_SIZE", "fetch"), ("WRITE_SIZE", "write")):
    rows = [r for r in csv.DictReader(open(newest(d + "/*/*_counter_collection.csv"))) if r["Kernel_Name"] == main and r["Counter_Name"] == name]
    vals = [float(r["Counter_Value"]) for r in rows]
    pmc[name] = [v for v in vals if v > 0.5 * max(vals)] if name == "WRITE_SIZE" else vals[1:]  # full-size launches only (the first is the 100 k-ray set-up trace)
json.dump(pmc, open(os.path.join(out, "trace_kernel_pmc.json"), "w"), indent=1)
sq = {}
for r in csv.DictReader(open(newest("sq/*/*_counter_collection.csv"))):
    if r["Kernel_Name"] == main:
        sq.setdefault(r["Counter_Name"], []).append(float(r["Counter_Value"]))
# full-size launches only: the set-up trace of bench.py has 1/100 of the waves
full = [i for i, w in enumerate(sq["SQ_WAVES"]) if w > 0.5 * max(sq["SQ_WAVES"])]
json.dump({"rays": 10000000, "pol": True, **{k: sum(v[i] for i in full) / len(full) for k, v in sq.items()}},
          open(os.path.join(out, "trace_kernel_sq.json"), "w"), indent=1)
os.replace(newest("detector/*/*_kernel_stats.csv"), os.path.join(out, "detector_kernel_stats.csv"))
print(open(os.path.join(out, "trace_kernel_sq.json")).read())
print("timed mean ms", sum(timed) / len(timed))
PY
grep -v amdgpu.ids "$OUT/detector.log" | grep "rays/s" > "$OUT/detector_full_size_profiled.txt" || true
