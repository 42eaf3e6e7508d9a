#!/usr/bin/env python3
"""Developer tool: the per-index assignment mode on cfg 3's table and batch, kernel scope, one box, arms alternating in one process:
     lds_memo     the default whole-barcode path (fqtk::lds_memo_kernel) on the same rows: the yardstick
     per_index    budgets 1,1, the two-memo LDS kernel (fqtk::per_index_kernel)
     scan         the same call with the per-index scan pinned
     whole_mm2    the whole-barcode rule at max_mismatches = 2, the nearest thing without this mode
   Five rounds (the first is warm-up), three launches each timed with device events; per arm the median and the spread.
usage: python tools/ab_per_index.py [reads]      (run on the GPU box)"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fqtk_amd import BarcodeMatcher, synth  # noqa: E402

cfg = synth.CONFIGS[3]
n = int(sys.argv[1]) if len(sys.argv) > 1 else cfg.n_reads
w = synth.Workload(cfg)
st = torch.cuda.current_stream().cuda_stream
L, stride = cfg.barcode_len, cfg.stride
d = torch.empty((n, stride), dtype=torch.uint8, device="cuda")
for lo in range(0, n, 50_000_000):
    w.fill_device(lo, min(50_000_000, n - lo), d.data_ptr() + lo * stride, st)
out = torch.empty(n, dtype=torch.int32, device="cuda")
cnt = torch.zeros(cfg.n_samples + 1, dtype=torch.int64, device="cuda")

m1 = BarcodeMatcher(w.barcodes, cfg.max_mismatches, cfg.min_mismatch_delta)
m1.set_per_index(L // 2, 1, cfg.min_mismatch_delta, 1, cfg.min_mismatch_delta)
assert m1.per_index_kind == m1.PER_INDEX_LDS, "the LDS form was not planned for cfg 3's table"
m2 = BarcodeMatcher(w.barcodes, 2, cfg.min_mismatch_delta)


def per_index(kind):
    def run():
        m1.per_index_kind = kind
        m1.assign_batch_per_index_device(d.data_ptr(), stride, n, out.data_ptr(), cnt.data_ptr(), stream=st)
    return run


arms = {"lds_memo": lambda: m1.assign_batch_device(d.data_ptr(), stride, n, out.data_ptr(), cnt.data_ptr(), stream=st),
        "per_index": per_index(m1.PER_INDEX_LDS), "scan": per_index(m1.PER_INDEX_SCAN),
        "whole_mm2": lambda: m2.assign_batch_device(d.data_ptr(), stride, n, out.data_ptr(), cnt.data_ptr(), stream=st)}
ms = {k: [] for k in arms}
some = {}
for rnd in range(5):
    for name, run in arms.items():
        cnt.zero_()
        run()
        torch.cuda.synchronize()
        some[name] = n - int(cnt[-1])
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(3):
            run()
        e1.record()
        torch.cuda.synchronize()
        if rnd:
            ms[name].append(e0.elapsed_time(e1) / 3)
print(f"ab_per_index n={n} S={cfg.n_samples} L={L} stride={stride} memo_kind(mm1)={m1.memo_kind} memo_kind(mm2)={m2.memo_kind}", flush=True)
base = sorted(ms["lds_memo"])[len(ms["lds_memo"]) // 2]
for name, v in ms.items():
    v = sorted(v)
    med = v[len(v) // 2]
    print(f"ab_per_index {name:10s} assigned {some[name]}  ms {' '.join('%.3f' % x for x in v)}  median {n / med / 1e6:.2f} G reads/s "
          f"= {n * (stride + 4) / med / 1e9 / 8 * 100:.1f} % of 8 TB/s on {stride + 4} B/read  x{base / med:.3f} of lds_memo", flush=True)
