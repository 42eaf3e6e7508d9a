#!/usr/bin/env python3
"""Developer tool: what the index-pair tally of the unmatched reads costs, kernel scope, on one box.
  1. with --parent DIR (a built checkout of the parent commit): the bench's kernel scope from that tree and from this one with the
     tally off, alternating, three rounds, each run a fresh process -- the flag-off cost next to the parent's own spread;
  2. cfg 3's table and batch size, the tally off and on alternating in one process over
       bench    the bench's own synthetic reads (len_a = L / 2),
       random   every read unmatched and uniformly random (every lane drains, nearly all of them into the last cell),
     four rounds per shape (the first is warm-up), three launches each timed with device events.  The results of the two arms
     are compared; the tally's sum is checked against counts[S].
usage: python tools/ab_pairs.py [--parent DIR] [reads]      (run on the GPU box; profiles/pairs_ab.txt keeps its lines)"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
argv = sys.argv[1:]
parent = None
if "--parent" in argv:
    parent = os.path.abspath(argv[argv.index("--parent") + 1])
    del argv[argv.index("--parent"):argv.index("--parent") + 2]

if parent:
    for rnd in range(3):
        for name, tree in (("parent", parent), ("this", ROOT)):
            r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "50", "--warmup", "10", "--cpu-seconds", "0", "--no-verify",
                                "--no-scopes"], cwd=tree, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                sys.exit(f"bench.py failed in {tree}:\n{r.stderr[-2000:]}")
            line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
            print(f"tree={name:6s} M_reads_s {line['value']} frac {line['roofline']['frac']} kernel_ms {line['roofline']['kernel_ms']}", flush=True)

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, ROOT)
from fqtk_amd import BarcodeMatcher, synth  # noqa: E402

cfg = synth.CONFIGS[3]
n = int(argv[0]) if argv else cfg.n_reads
w = synth.Workload(cfg)
st = torch.cuda.current_stream().cuda_stream
L, stride = cfg.barcode_len, cfg.stride


def reads(shape):
    d = torch.empty((n, stride), dtype=torch.uint8, device="cuda")
    if shape == "bench":
        for lo in range(0, n, 50_000_000):
            w.fill_device(lo, min(50_000_000, n - lo), d.data_ptr() + lo * stride, st)
    else:
        acgt = torch.from_numpy(np.frombuffer(b"ACGT", np.uint8).copy()).cuda()
        for lo in range(0, n, 50_000_000):
            d[lo:lo + 50_000_000] = acgt[torch.randint(0, 4, (min(50_000_000, n - lo), stride), device="cuda")]
    return d


for shape in ("bench", "random"):
    d = reads(shape)
    m = BarcodeMatcher(w.barcodes, cfg.max_mismatches, cfg.min_mismatch_delta)
    out = {k: torch.empty(n, dtype=torch.int32, device="cuda") for k in (0, 1)}
    ms = {0: [], 1: []}
    for rnd in range(4):
        for on in (0, 1):
            m.enable_pairs(L // 2) if on else m.disable_pairs()
            cnt = torch.zeros(cfg.n_samples + 1, dtype=torch.int64, device="cuda")
            m.assign_batch_device(d.data_ptr(), stride, n, out[on].data_ptr(), cnt.data_ptr(), stream=st)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(3):
                m.assign_batch_device(d.data_ptr(), stride, n, out[on].data_ptr(), cnt.data_ptr(), stream=st)
            e1.record()
            torch.cuda.synchronize()
            m.poll_error(st)
            if rnd:
                ms[on].append(e0.elapsed_time(e1) / 3)
            if on:
                mat, skipped = m.pairs()
                assert int(mat.sum()) + skipped == int(cnt[-1]), (shape, int(mat.sum()), skipped, int(cnt[-1]))
    assert torch.equal(out[0], out[1]), shape
    u_a, u_b = mat.shape[0] - 1, mat.shape[1] - 1
    off, on_ = min(ms[0]), min(ms[1])
    print(f"ab_pairs {shape} n={n} none={int(cnt[-1]) // 4} U_A={u_a} U_B={u_b} both={int(mat[:-1, :-1].sum()) // 4} neither={int(mat[-1, -1]) // 4}  "
          f"ms per batch off {' '.join('%.3f' % x for x in ms[0])}  on {' '.join('%.3f' % x for x in ms[1])}  "
          f"pairs +{on_ - off:.3f} ms = {100 * (on_ - off) / off:.0f} % of the match kernel  equal=True", flush=True)
    del d, out
