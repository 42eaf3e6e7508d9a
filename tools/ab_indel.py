#!/usr/bin/env python3
"""Developer tool: what the indel rescue of the unmatched reads (fqtk::indel_rescue_kernel) costs, kernel scope, on one box.
  1. with --parent DIR (a built checkout of the parent commit): the bench's kernel scope from that tree and from this one with the
     rescue off, alternating, three rounds, each run a fresh process -- the flag-off cost next to the parent's own spread;
  2. cfg 3's table and the bench's own batch with 0 %, 2 % and 10 % of the reads carrying one indel (a base deleted and the row
     refilled at its end, or one inserted and the row cut), the rescue off and on (--indel-rescue 1,2) alternating in one process:
     four rounds per share (the first is warm-up), three launches each timed with device events.  The on-arm's counters are checked
     against the off-arm's counts[S]; the kernel's rate is the reads it examined over the time the batch grew by.
usage: python tools/ab_indel.py [--parent DIR] [reads]      (run on the GPU box; profiles/indel_rescue_ab.txt keeps its lines)"""
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
L, stride, S = cfg.barcode_len, cfg.stride, cfg.n_samples
CHUNK = 50_000_000


def reads(share):
    """The bench's batch; `share` of its rows then get one indel at a random place."""
    d = torch.empty((n, stride), dtype=torch.uint8, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(7)
    acgt = torch.from_numpy(np.frombuffer(b"ACGT", np.uint8).copy()).cuda()
    pos = torch.arange(L, device="cuda")[None]
    for lo in range(0, n, CHUNK):
        cur = min(CHUNK, n - lo)
        w.fill_device(lo, cur, d.data_ptr() + lo * stride, st)
        torch.cuda.synchronize()
        if not share:
            continue
        rows = torch.nonzero(torch.rand(cur, device="cuda", generator=gen) < share)[:, 0] + lo
        p = torch.randint(0, L, (len(rows), 1), device="cuda", generator=gen)
        deleted = torch.rand((len(rows), 1), device="cuda", generator=gen) < 0.5
        src = torch.where(deleted, pos + (pos >= p).long(), pos - (pos > p).long()).clamp_(0, L - 1)
        new = torch.gather(d[rows, :L], 1, src)
        fresh = acgt[torch.randint(0, 4, (len(rows), 1), device="cuda", generator=gen)]
        new = torch.where(torch.where(deleted, pos == L - 1, pos == p), fresh, new)   # the refill at the end / the inserted base
        d[rows, :L] = new
    return d


for share in (0.0, 0.02, 0.10):
    d = reads(share)
    m = BarcodeMatcher(w.barcodes, cfg.max_mismatches, cfg.min_mismatch_delta)
    out = torch.empty(n, dtype=torch.int32, device="cuda")
    ms, none = {0: [], 1: []}, 0
    for rnd in range(4):
        for on in (0, 1):
            m.enable_indel_rescue(1, 2) if on else m.disable_indel_rescue()
            cnt = torch.zeros(S + 1, dtype=torch.int64, device="cuda")
            m.assign_batch_device(d.data_ptr(), stride, n, out.data_ptr(), cnt.data_ptr(), stream=st)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(3):
                m.assign_batch_device(d.data_ptr(), stride, n, out.data_ptr(), cnt.data_ptr(), stream=st)
            e1.record()
            torch.cuda.synchronize()
            m.poll_error(st)
            if rnd:
                ms[on].append(e0.elapsed_time(e1) / 3)
            if not on:
                none = int(cnt[-1]) // 4
            else:
                rescued, skipped = m.indel_rescued()
                assert int(rescued.sum()) + skipped == 4 * none and int(rescued[:-1].sum()) == 4 * (none - int(cnt[-1]) // 4), (share, none)
    off, on_ = min(ms[0]), min(ms[1])
    examined, moved = int(rescued.sum()) // 4, int(rescued[:-1].sum()) // 4
    rate = examined / ((on_ - off) * 1e-3) / 1e9 if on_ > off else float("nan")
    print(f"ab_indel share={share:.2f} n={n} S={S} L={L} none={none} examined={examined} rescued={moved}  "
          f"ms per batch off {' '.join('%.3f' % x for x in ms[0])}  on {' '.join('%.3f' % x for x in ms[1])}  "
          f"rescue +{on_ - off:.3f} ms = {100 * (on_ - off) / off:.0f} % of the batch  {rate:.4f} G None reads/s", flush=True)
    del d, out
