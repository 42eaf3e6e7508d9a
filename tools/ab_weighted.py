#!/usr/bin/env python3
"""Developer tool: same-box A/B of the quality-weighted scan (fqtk::weighted_scan_kernel) against the unweighted MFMA scan of the same
matcher (use_cache off, scan_kind MFMA), alternating in one process; tables and reads as tools/ab_scan.py makes them, qualities
uniform in '!'..'K', the bench's batch of 400 M reads.  Four rounds of mfma, weighted per shape (the first is warm-up), three launches
each timed with device events.
usage: python tools/ab_weighted.py [SxL ...]     (run on the GPU box; profiles/weighted_scan_ab.txt keeps its lines)"""
import sys, os
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fqtk_amd import BarcodeMatcher
shapes = [tuple(int(x) for x in a.split("x")) for a in sys.argv[1:]] or [(384, 16), (96, 8), (385, 16)]
n = 400_000_000
st = torch.cuda.current_stream().cuda_stream
for S, L in shapes:
    rng = np.random.default_rng(5)
    seen = set()
    while len(seen) < S:
        seen.add("".join(rng.choice(list("ACGT"), size=L)))
    bcs = sorted(seen)
    m0 = n // 100
    obs = np.stack([np.frombuffer(b.encode(), dtype=np.uint8) for b in bcs])[rng.integers(0, S, size=m0)]
    flip = rng.random(obs.shape) < 0.015
    obs[flip] = np.frombuffer(b"ACGTN", dtype=np.uint8)[rng.integers(0, 5, int(flip.sum()))]
    rnd = rng.random(m0) < 0.1
    obs[rnd] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (int(rnd.sum()), L))]
    stride = (L + 3) // 4 * 4
    pad = np.zeros((m0, stride), dtype=np.uint8)
    pad[:, :L] = obs
    d = torch.from_numpy(pad).cuda().repeat(100, 1)
    q = torch.from_numpy(rng.integers(ord("!"), ord("K") + 1, size=pad.shape, dtype=np.uint8)).cuda().repeat(100, 1)
    m = BarcodeMatcher(bcs, 1, 2, use_cache=False)
    m.scan_kind = m.SCAN_MFMA
    m.set_weighted(60, 30)
    out = torch.empty(n, dtype=torch.int32, device="cuda")
    costs = torch.empty(n, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(S + 1, dtype=torch.int64, device="cuda")
    arms = {"mfma": lambda: m.assign_batch_device(d.data_ptr(), stride, n, out.data_ptr(), cnt.data_ptr(), stream=st),
            "weighted": lambda: m.assign_batch_weighted_device(d.data_ptr(), q.data_ptr(), stride, n, out.data_ptr(), costs.data_ptr(),
                                                               cnt.data_ptr(), st),
            "weighted_nocosts": lambda: m.assign_batch_weighted_device(d.data_ptr(), q.data_ptr(), stride, n, out.data_ptr(), 0,
                                                                       cnt.data_ptr(), st)}
    rates = {k: [] for k in arms}
    for rnd_i in range(4):
        for kind, run in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            run()
            torch.cuda.synchronize()
            e0.record()
            for _ in range(3):
                run()
            e1.record()
            torch.cuda.synchronize()
            if rnd_i:
                rates[kind].append(3 * n / (e0.elapsed_time(e1) * 1e-3) / 1e9)
    med = {k: float(np.median(v)) for k, v in rates.items()}
    print(f"ab_weighted S={S} L={L} n={n}  G reads/s  " + "  ".join(f"{k} {' '.join('%.2f' % r for r in v)}" for k, v in rates.items()) +
          f"  weighted/mfma {med['weighted'] / med['mfma']:.3f}  nocosts/mfma {med['weighted_nocosts'] / med['mfma']:.3f}", flush=True)
    del d, q
