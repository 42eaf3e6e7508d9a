#!/usr/bin/env python3
"""Developer tool: what `fqtk demux --quality-metrics` costs, on one box, at scope E's shape (cfg 3: R1 150T, I1 8B, I2 8B, R2 150T,
384 samples, plain text, the first 1 M templates repeated).

  ab       alternating runs of `fqtk demux`: [another build's binary with the flag off,] this build with the flag off, this build
           with the flag on -- the steady rate (fqtk's own clock, first chunk submitted -> last byte written) of every run, the
           spread of every arm and the differences between the arms;
  profile  one run with the flag on under `rocprofv3 --kernel-trace --stats` (FQTK_CLEAN_EXIT=1): k_quality's time per chunk, the
           bytes it must read per chunk -- the quality bytes in T spans, 4 B of result, 1 B of skip flag and a 20-byte record
           view per input with a T segment, per template -- and the GB/s that makes, to set beside tools/hbm_stream.hip's figure.

usage: python tools/ab_quality.py ab [--templates N] [--reps R] [--other-exe PATH/fqtk]
       python tools/ab_quality.py profile [--templates N]          (run on the GPU box; profiles/quality_ab.txt keeps its lines)"""
import argparse
import csv
import glob
import os
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import scope_bench  # noqa: E402

EXE = os.path.join(ROOT, "fqtk_amd", "bin", "fqtk")
CHUNK = 262144
BYTES_PER_TEMPLATE = 2 * 150 + 4 + 1 + 2 * 20


def demux(exe, paths, meta, out, threads, extra, wrap=(), env=None):
    cmd = [*wrap, exe, "demux", "-i", *paths, "-r", "150T", "8B", "8B", "150T", "-s", meta, "-o", out, "-t", str(threads), *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stderr[-2000:]
    steady = [float(ln.split("(")[1].split(" M templates/s")[0]) for ln in r.stderr.splitlines() if "GPU record pipeline:" in ln]
    quality = os.path.join(out, "demux-quality-metrics.txt")
    text = open(quality).read() if os.path.exists(quality) else None
    shutil.rmtree(out, ignore_errors=True)
    return steady[0], text


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
    if a.mode == "ab":
        arms = ([("other_off", a.other_exe, [])] if a.other_exe else []) + [("off", EXE, []), ("on", EXE, ["--quality-metrics"])]
        rates = {name: [] for name, _, _ in arms}
        demux(EXE, paths, meta, out, a.threads, [])   # warm-up: page cache, code objects
        for rep in range(a.reps):
            for name, exe, extra in arms:
                rate, text = demux(exe, paths, meta, out, a.threads, extra)
                assert (text is not None) == bool(extra)
                rates[name].append(rate)
        mid = {k: sorted(v)[len(v) // 2] for k, v in rates.items()}
        line = f"ab_quality ab templates={a.templates} steady M templates/s  " + "  ".join(
            f"{k} {' '.join('%.2f' % x for x in v)} (spread {max(v) - min(v):.2f})" for k, v in rates.items())
        line += f"  on - off {mid['on'] - mid['off']:+.2f} ({100 * (mid['on'] - mid['off']) / mid['off']:+.1f} %)"
        if a.other_exe:
            line += f"  off - other_off {mid['off'] - mid['other_off']:+.2f} ({100 * (mid['off'] - mid['other_off']) / mid['other_off']:+.1f} %)"
        print(line, flush=True)
    else:
        prof = os.path.join(tmp, "prof")
        demux(EXE, paths, meta, out, a.threads, ["--quality-metrics"], wrap=["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", prof, "-o", "q", "--"],
              env={"FQTK_CLEAN_EXIT": "1"})
        rows = [r for f in glob.glob(os.path.join(prof, "**", "*kernel_stats.csv"), recursive=True) for r in csv.DictReader(open(f))]
        by = {r["Name"].split("(")[0]: r for r in rows}
        q = next(r for n, r in by.items() if "k_quality" in n)
        calls, avg_us = int(q["Calls"]), float(q["AverageNs"]) / 1e3
        per_chunk = BYTES_PER_TEMPLATE * min(CHUNK, a.templates)
        print(f"ab_quality profile templates={a.templates} k_quality calls={calls} avg {avg_us:.1f} us min {float(q['MinNs']) / 1e3:.1f} max {float(q['MaxNs']) / 1e3:.1f}  "
              f"bytes per full chunk {per_chunk} ({BYTES_PER_TEMPLATE} B a template)  {per_chunk / avg_us / 1e3:.0f} GB/s", flush=True)
        for n, r in sorted(by.items(), key=lambda kv: -float(kv[1]["TotalDurationNs"]))[:8]:
            print(f"  {float(r['AverageNs']) / 1e3:9.1f} us x {r['Calls']:>5}  {n[:90]}", flush=True)
finally:
    shutil.rmtree(tmp, ignore_errors=True)
