#!/usr/bin/env python3
"""Developer tool: what the census of unmatched barcodes costs, kernel scope, on one box: cfg 3's table and batch size with
  bench    the bench's own synthetic reads,
  random   every read unmatched and uniformly random (distinct keys far beyond LDS and beyond the table: the overflow path),
  single   every read one and the same unmatched barcode (64 lanes, one key),
census off and on alternating in one process -- four rounds per shape (the first is warm-up), three launches each timed with
device events.  The results of the two arms are compared; the census' totals are checked against counts[S].
usage: python tools/ab_census.py [reads]      (run on the GPU box; profiles/census_ab.txt keeps its lines)"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fqtk_amd import BarcodeMatcher, synth

cfg = synth.CONFIGS[3]
n = int(sys.argv[1]) if len(sys.argv) > 1 else cfg.n_reads
w = synth.Workload(cfg)
st = torch.cuda.current_stream().cuda_stream
L, stride = cfg.barcode_len, cfg.stride


def reads(shape):
    d = torch.empty((n, stride), dtype=torch.uint8, device="cuda")
    if shape == "bench":
        for lo in range(0, n, 50_000_000):
            w.fill_device(lo, min(50_000_000, n - lo), d.data_ptr() + lo * stride, st)
    elif shape == "random":
        acgt = torch.from_numpy(np.frombuffer(b"ACGT", np.uint8).copy()).cuda()
        for lo in range(0, n, 50_000_000):
            d[lo:lo + 50_000_000] = acgt[torch.randint(0, 4, (min(50_000_000, n - lo), stride), device="cuda")]
    else:
        d[:] = ord("G")   # poly-G
    return d


for shape in ("bench", "random", "single"):
    d = reads(shape)
    m = BarcodeMatcher(w.barcodes, cfg.max_mismatches, cfg.min_mismatch_delta)
    out = {k: torch.empty(n, dtype=torch.int32, device="cuda") for k in (0, 1)}
    ms = {0: [], 1: []}
    for rnd in range(4):
        for on in (0, 1):
            m.enable_census() if on else m.disable_census()
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
                t = m.census_totals()
                assert t.keyed + t.unkeyed + t.overflow == int(cnt[-1]), (shape, t, int(cnt[-1]))
    assert torch.equal(out[0], out[1]), shape
    off, on_ = min(ms[0]), min(ms[1])
    print(f"ab_census {shape} n={n} none={int(cnt[-1]) // 4} distinct={t.distinct} overflow={t.overflow // 4}  "
          f"ms per batch off {' '.join('%.3f' % x for x in ms[0])}  on {' '.join('%.3f' % x for x in ms[1])}  "
          f"census +{on_ - off:.3f} ms = {100 * (on_ - off) / off:.0f} % of the match kernel  equal=True", flush=True)
    del d, out
