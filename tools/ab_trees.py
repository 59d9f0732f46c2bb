#!/usr/bin/env python3
"""A/B of whole source trees on ONE box (each with its own package and built library): runs `bench.py --gpus 1 --steps 50
--warmup 30` once per tree and round, interleaved, and prints kernel ms / step ms per run, the medians, the run-to-run spreads
(max - min) and the gain in units of the larger spread.  Stops at the first run that does not end cleanly, after printing what
it has.  (tools/ab_bench.py swaps the library under ONE tree's Python; this is for changes whose Python side differs too.)
Usage: ab_trees.py [--rounds R] name=dir name=dir"""
import json
import pathlib
import statistics
import subprocess
import sys

args = sys.argv[1:]
rounds = 5
if args and args[0] == "--rounds":
    rounds, args = int(args[1]), args[2:]
arms = [(n, pathlib.Path(d).resolve()) for n, d in (a.split("=", 1) for a in args)]
res = {n: [] for n, _ in arms}
for r in range(rounds):
    for name, cwd in arms:
        p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "50", "--warmup", "30"], cwd=cwd,
                           capture_output=True, text=True, timeout=300)
        if p.returncode != 0:
            print(f"{name} round {r}: exit status {p.returncode}\n{p.stderr[-1500:]}\nruns so far (kernel_ms, ms_per_step): {res}")
            sys.exit(1)
        d = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
        res[name].append((d["roofline"]["kernel_ms"], d["ms_per_step"]))
        print(f"round {r} {name:10s} kernel_ms {res[name][-1][0]:.4f}  ms_per_step {res[name][-1][1]:.4f}", flush=True)
med = {n: statistics.median(x[0] for x in v) for n, v in res.items()}
spread = {n: max(x[0] for x in v) - min(x[0] for x in v) for n, v in res.items()}
for n in res:
    print(f"{n:10s} median kernel_ms {med[n]:.4f}  spread {spread[n]:.4f}  median ms_per_step "
          f"{statistics.median(x[1] for x in res[n]):.4f}")
if len(arms) == 2:
    (a, _), (b, _) = arms
    print(f"{a} - {b}: {med[a] - med[b]:.4f} ms = {(med[a] - med[b]) / max(spread.values()):.2f} x the larger spread; "
          f"{b} / {a} = {med[b] / med[a]:.4f}")
