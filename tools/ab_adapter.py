#!/usr/bin/env python3
"""Developer tool: what `fqtk demux --adapter-metrics` costs, on one box, at scope E's shape (cfg 3: R1 150T, I1 8B, I2 8B, R2 150T,
384 samples, plain text, the first 1 M templates repeated), with the TruSeq pair of 33-base adapters and the default rule.

  ab       alternating runs of `fqtk demux`: [another build's binary with the flag off,] this build with the flag off, this build
           with the flag on -- the steady rate (fqtk's own clock, first chunk submitted -> last byte written) and the wall clock of
           every run, the spread of every arm and the differences between the arms;
  profile  one run with the flag on under `rocprofv3 --kernel-trace --stats` (FQTK_CLEAN_EXIT=1): k_adapter's time per chunk, its
           rate in items (template x scanned read) per second, and the vector lane-operations that rate stands for by the
           kernel's instruction count -- 16 lanes an item x (12 a base of the adapter in the scan + about 140 a 256-byte pass of
           the encode + about 150 of set-up, decision and tally) -- to set beside tools/valu_peak.hip's figure.

usage: python tools/ab_adapter.py ab [--templates N] [--reps R] [--other-exe PATH/fqtk]
       python tools/ab_adapter.py profile [--templates N]          (run on the GPU box; profiles/adapter_ab.txt keeps its lines)"""
import argparse
import csv
import glob
import os
import shutil
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import scope_bench  # noqa: E402

EXE = os.path.join(ROOT, "fqtk_amd", "bin", "fqtk")
CHUNK = 262144
ADAPTERS = "AGATCGGAAGAGCACACGTCTGAACTCCAGTCA,AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGT"
LANE_OPS_PER_ITEM = 16 * (12 * 33 + 2 * 140 + 150)   # a 150-base span that does not start on a 16-byte boundary takes two passes


def demux(exe, paths, meta, out, threads, extra, wrap=(), env=None):
    cmd = [*wrap, exe, "demux", "-i", *paths, "-r", "150T", "8B", "8B", "150T", "-s", meta, "-o", out, "-t", str(threads), *extra]
    t0 = time.perf_counter()
    r = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, **(env or {})))
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr[-2000:]
    steady = [float(ln.split("(")[1].split(" M templates/s")[0]) for ln in r.stderr.splitlines() if "GPU record pipeline:" in ln]
    report = os.path.join(out, "adapter-metrics.txt")
    text = open(report).read() if os.path.exists(report) else None
    shutil.rmtree(out, ignore_errors=True)
    return steady[0], wall, text


ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=["ab", "profile"])
ap.add_argument("--templates", type=int, default=64_000_000)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--other-exe", default="")
a = ap.parse_args()
tmp = scope_bench.scratch_dir(a.templates * 900)
try:
    paths, meta, _ = scope_bench.make_inputs(tmp, a.templates, False, repeat_first_block=a.templates > 1_000_000)
    out = os.path.join(tmp, "out")
    on = ["--adapter-metrics", ADAPTERS]
    if a.mode == "ab":
        arms = ([("other_off", a.other_exe, [])] if a.other_exe else []) + [("off", EXE, []), ("on", EXE, on)]
        rates, walls = {name: [] for name, _, _ in arms}, {name: [] for name, _, _ in arms}
        demux(EXE, paths, meta, out, a.threads, [])   # warm-up: page cache, code objects
        for rep in range(a.reps):
            for name, exe, extra in arms:
                rate, wall, text = demux(exe, paths, meta, out, a.threads, extra)
                assert (text is not None) == bool(extra)
                rates[name].append(rate)
                walls[name].append(wall)
                print(f"  rep {rep} {name}: {rate:.2f} M templates/s steady, {wall:.2f} s wall", file=sys.stderr, flush=True)
        mid = {k: sorted(v)[len(v) // 2] for k, v in rates.items()}
        line = f"ab_adapter ab templates={a.templates} steady M templates/s  " + "  ".join(
            f"{k} {' '.join('%.2f' % x for x in v)} (spread {max(v) - min(v):.2f})" for k, v in rates.items())
        line += f"  on - off {mid['on'] - mid['off']:+.2f} ({100 * (mid['on'] - mid['off']) / mid['off']:+.1f} %)"
        if a.other_exe:
            line += f"  off - other_off {mid['off'] - mid['other_off']:+.2f} ({100 * (mid['off'] - mid['other_off']) / mid['other_off']:+.1f} %)"
        print(line, flush=True)
        print(f"ab_adapter ab templates={a.templates} wall s  " + "  ".join(
            f"{k} {' '.join('%.2f' % x for x in v)} (spread {max(v) - min(v):.2f})" for k, v in walls.items()), flush=True)
    else:
        prof = os.path.join(tmp, "prof")
        demux(EXE, paths, meta, out, a.threads, on, wrap=["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", prof, "-o", "a", "--"],
              env={"FQTK_CLEAN_EXIT": "1"})
        rows = [r for f in glob.glob(os.path.join(prof, "**", "*kernel_stats.csv"), recursive=True) for r in csv.DictReader(open(f))]
        by = {r["Name"].split("(")[0]: r for r in rows}
        k = next(r for n, r in by.items() if "k_adapter" in n)
        calls, avg_us, max_us = int(k["Calls"]), float(k["AverageNs"]) / 1e3, float(k["MaxNs"]) / 1e3
        items = 2 * min(CHUNK, a.templates)
        print(f"ab_adapter profile templates={a.templates} k_adapter calls={calls} avg {avg_us:.1f} us min {float(k['MinNs']) / 1e3:.1f} max {max_us:.1f}  "
              f"items per full chunk {items}: {items / max_us / 1e3:.2f} G items/s, x {LANE_OPS_PER_ITEM} lane-ops an item = "
              f"{items * LANE_OPS_PER_ITEM / max_us / 1e6:.1f} T lane-ops/s (a full chunk is the slowest call)", flush=True)
        for n, r in sorted(by.items(), key=lambda kv: -float(kv[1]["TotalDurationNs"]))[:8]:
            print(f"  {float(r['AverageNs']) / 1e3:9.1f} us x {r['Calls']:>5}  {n[:90]}", flush=True)
finally:
    shutil.rmtree(tmp, ignore_errors=True)
