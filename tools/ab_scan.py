#!/usr/bin/env python3
"""Developer tool: same-box A/B of the two exhaustive-scan kernels (use_cache off), alternating in one process; tables and reads
as tools/bench_custom.py makes them.  Four rounds of valu, mfma per shape (the first is warm-up), three launches of 40 M reads
each timed with device events; the two arms' outputs are compared.
usage: python tools/ab_scan.py SxL[xMM] ...     (run on the GPU box; profiles/mfma_scan_ab.txt keeps its lines)"""
import sys, os
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fqtk_amd import BarcodeMatcher
shapes = [tuple(int(x) for x in a.split("x")) for a in sys.argv[1:]]
shapes = [(s[0], s[1], s[2] if len(s) > 2 else 1) for s in shapes]
n = 40_000_000
st = torch.cuda.current_stream().cuda_stream
for S, L, mm in shapes:
    assert S <= 4 ** L, "more samples than there are barcodes of this length"
    rng = np.random.default_rng(5)
    seen = set()
    while len(seen) < S:
        seen.add("".join(rng.choice(list("ACGT"), size=L)))
    bcs = sorted(seen)
    m0 = n // 100
    bc = np.stack([np.frombuffer(b.encode(), dtype=np.uint8) for b in bcs])[rng.integers(0, S, size=m0)]
    obs = bc.copy()
    flip = rng.random(obs.shape) < 0.015
    obs[flip] = np.frombuffer(b"ACGTN", dtype=np.uint8)[rng.integers(0, 5, int(flip.sum()))]
    rnd = rng.random(m0) < 0.1
    obs[rnd] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (int(rnd.sum()), L))]
    stride = (L + 3) // 4 * 4
    pad = np.zeros((m0, stride), dtype=np.uint8)
    pad[:, :L] = obs
    d = torch.from_numpy(np.tile(pad, (100, 1))).cuda()
    outs = {}
    m = BarcodeMatcher(bcs, mm, 2, use_cache=False)
    rates = {0: [], 1: []}
    for rnd_i in range(4):
        for kind in (0, 1):
            m.scan_kind = kind
            out = torch.empty(n, dtype=torch.int32, device="cuda")
            cnt = torch.zeros(S + 1, dtype=torch.int64, device="cuda")
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            m.assign_batch_device(d.data_ptr(), stride, n, out.data_ptr(), cnt.data_ptr(), stream=st)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(3):
                m.assign_batch_device(d.data_ptr(), stride, n, out.data_ptr(), cnt.data_ptr(), stream=st)
            e1.record()
            torch.cuda.synchronize()
            m.poll_error(st)
            if rnd_i:
                rates[kind].append(3 * n / (e0.elapsed_time(e1) * 1e-3) / 1e9)
            outs[kind] = out
        assert torch.equal(outs[0], outs[1]), (S, L, mm)
    print(f"ab_scan S={S} L={L} mm={mm} n={n}  valu G reads/s {' '.join('%.2f' % r for r in rates[0])}  mfma {' '.join('%.2f' % r for r in rates[1])}  equal=True", flush=True)
    del d
