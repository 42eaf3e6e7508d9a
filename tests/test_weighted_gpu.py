"""Quality-weighted assignment (fqtk::weighted_scan_kernel) against the rule of include/fqtk_match.h written out in numpy, int64:
exact equality of idx, both costs, the two saturated bytes and the counts, at the shapes where the kernel takes another path."""
import ctypes as C

import numpy as np
import pytest

from fqtk_amd import BarcodeMatcher, _lib
from oracle import oracle as O
from tests.test_mfma_scan_gpu import DT, make_reads, make_table

pytestmark = pytest.mark.gpu

NONE32 = 0xFFFFFFFF


def reference(barcodes, obs, qual, max_cost, delta):
    """(idx, best cost, next cost, counts); None rows are (0xFFFF, -1, -1)."""
    L = len(barcodes[0])
    tab = np.frombuffer("".join(barcodes).encode("latin-1"), dtype=np.uint8).reshape(len(barcodes), L)
    w = np.clip(qual[:, :L].astype(np.int64) - 33, 0, 93)
    mism = (O.ENC[obs[:, :L]][:, None, :] & ~O.ENC[tab][None]) != 0
    cost = (mism * w[:, None, :]).sum(-1)
    idx = cost.argmin(1)                                            # the lowest index on ties
    srt = np.sort(cost, axis=1)
    best, nxt = srt[:, 0], (srt[:, 1] if len(barcodes) > 1 else np.full(len(obs), 0xFFFF))
    none = (best > max_cost) | (nxt - best < delta)
    counts = np.bincount(np.where(none, len(barcodes), idx), minlength=len(barcodes) + 1).astype(np.uint64)
    return np.where(none, 0xFFFF, idx), np.where(none, -1, best), np.where(none, -1, nxt), counts


def check(barcodes, obs, qual, max_cost, delta, got=None):
    if got is None:
        got = BarcodeMatcher(barcodes, 1, 1, use_cache=False).assign_batch_weighted(obs, qual, max_cost, delta)
    out, costs, cnt = got
    idx, best, nxt, counts = reference(barcodes, obs, qual, max_cost, delta)
    none = idx == 0xFFFF
    assert np.array_equal(out["idx"], idx)
    assert np.array_equal(costs, np.where(none, NONE32, best | (nxt << 16)).astype(np.uint32))
    assert np.array_equal(out["best"], np.where(none, 255, np.minimum(best, 255)))
    assert np.array_equal(out["next"], np.where(none, 255, np.minimum(nxt, 255)))
    assert np.array_equal(cnt, counts)
    return none


# K steps change at L 12 | 13, the variant at 16 | 17; a tile (33) and a 128-sample group (129) with one row too many; S = 1; 1500 x 16
# does not fit one LDS staging; n = 3001 ends in a partial wave; 5 x 4 is the one-dword load path
@pytest.mark.parametrize("S,L,n", [(1, 1, 1), (5, 4, 59), (2, 8, 63), (33, 12, 65), (128, 13, 64), (129, 16, 3001), (385, 16, 3001), (385, 17, 65),
                                   (257, 32, 3001), (1500, 16, 1000)])
def test_structure_edges(S, L, n):
    rng = np.random.default_rng(1000 * S + L)
    barcodes = make_table(rng, S, L)
    obs = make_reads(rng, barcodes, n)
    qual = rng.integers(ord("!"), ord("K") + 1, size=obs.shape, dtype=np.uint8)
    _, best, nxt, _ = reference(barcodes, obs, qual, 93 * L, 0)      # loose bound, no delta: every read is Some
    delta = int(np.median(nxt - best))                               # both outcomes occur: about half the reads keep their costs
    none = check(barcodes, obs, qual, 93 * L, delta)
    assert n < 60 or (none.any() and not none.all())


@pytest.mark.parametrize("iupac", [0.0, 0.5])
@pytest.mark.parametrize("vary", ["base", "quality"])
def test_every_byte_value_at_every_position(iupac, vary):
    L = 16
    rng = np.random.default_rng(7)
    barcodes = make_table(rng, 5, L, iupac)
    tab = np.frombuffer("".join(barcodes).encode(), dtype=np.uint8).reshape(5, L)
    obs = tab[np.arange(L * 256) % 5].copy()
    obs[:, 3] = ord("N")
    obs[::3, 9] = ord("R")                                           # a flagged read in every third row
    qual = rng.integers(ord("!"), ord("K") + 1, size=obs.shape, dtype=np.uint8)
    (obs if vary == "base" else qual)[np.arange(L * 256), np.repeat(np.arange(L), 256)] = np.tile(np.arange(256, dtype=np.uint8), L)
    check(barcodes, obs, qual, 200, 5)


@pytest.mark.parametrize("q", [1, 40, 93])
def test_uniform_quality_is_the_reference_rule(q):
    rng = np.random.default_rng(q)
    barcodes = make_table(rng, 97, 16)
    obs = make_reads(rng, barcodes, 2000)
    qual = np.full(obs.shape, 33 + q, dtype=np.uint8)
    mm, delta = 2, 2
    out, costs, cnt = BarcodeMatcher(barcodes, 0, 0, use_cache=False).assign_batch_weighted(obs, qual, q * mm + q - 1, q * delta)
    idx, best, nxt, counts = O.RefLiteral(barcodes, mm, delta, False).assign_batch(obs)
    some = idx != 0xFFFF
    assert some.any() and not some.all()
    assert np.array_equal(out["idx"], idx) and np.array_equal(cnt, counts)
    assert np.array_equal(costs[some], q * (best[some].astype(np.uint32) | (nxt[some].astype(np.uint32) << 16)))
    assert (costs[~some] == NONE32).all()


@pytest.mark.parametrize("L", [8, 13])
def test_load_paths(L):
    import torch
    rng = np.random.default_rng(L)
    barcodes = make_table(rng, 40, L)
    n, stride, off = 300, L + 6, 3
    obs = rng.integers(0, 256, size=(n, stride), dtype=np.uint8)     # garbage in the pad bytes of both rows
    qual = rng.integers(0, 256, size=(n, stride), dtype=np.uint8)
    obs[:, :L] = make_reads(rng, barcodes, n)
    qual[:, :L] = rng.integers(ord("!"), ord("K") + 1, size=(n, L), dtype=np.uint8)
    check(barcodes, obs, qual, 93 * L, 12)                           # stride > L, aligned base
    dev = torch.device("cuda:0")
    d_obs = torch.zeros(off + n * stride + 16, dtype=torch.uint8, device=dev)       # the same rows at an unaligned base
    d_qual = torch.zeros(off + n * stride + 16, dtype=torch.uint8, device=dev)
    d_obs[off:off + n * stride] = torch.from_numpy(obs.reshape(-1)).to(dev)
    d_qual[off:off + n * stride] = torch.from_numpy(qual.reshape(-1)).to(dev)
    d_out = torch.empty(n, dtype=torch.int32, device=dev)
    d_costs = torch.empty(n, dtype=torch.int32, device=dev)
    d_counts = torch.zeros(len(barcodes) + 1, dtype=torch.int64, device=dev)
    m = BarcodeMatcher(barcodes, 1, 1, use_cache=False)
    m.set_weighted(93 * L, 12)
    m.assign_batch_weighted_device(d_obs.data_ptr() + off, d_qual.data_ptr() + off, stride, n, d_out.data_ptr(), d_costs.data_ptr(),
                                   d_counts.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    check(barcodes, obs, qual, 93 * L, 12, (d_out.cpu().numpy().view(DT), d_costs.cpu().numpy().view(np.uint32),
                                            d_counts.cpu().numpy().astype(np.uint64)))


def words(S, L):   # every L-letter word over ACGT, in index order
    d = (np.arange(S)[:, None] >> (2 * np.arange(L)[::-1])) & 3
    return [r.tobytes().decode() for r in np.frombuffer(b"ACGT", dtype=np.uint8)[d]]


@pytest.mark.parametrize("case", ["L=33", "S=16385", "before set_weighted", "NULL quality", "stride < L"])
def test_refusals_leave_the_matcher_usable(case):
    rng = np.random.default_rng(5)
    barcodes = words(16385, 8) if case == "S=16385" else make_table(rng, 20, 33 if case == "L=33" else 12)
    L = len(barcodes[0])
    m = BarcodeMatcher(barcodes, 2, 1, use_cache=False)
    obs = make_reads(rng, barcodes, 100)
    qual = np.full(obs.shape, ord("I"), dtype=np.uint8)
    before, before_counts = m.assign_batch(obs)
    out, costs = np.empty(100, dtype=DT), np.empty(100, dtype=np.uint32)
    call = lambda o, q, stride: m._lib.fqtk_matcher_assign_weighted_batch(m.handle, o, q, stride, 100, out.ctypes.data, costs.ctypes.data, None)
    if case in ("L=33", "S=16385"):
        assert m._lib.fqtk_matcher_set_weighted(m.handle, 100, 10) == _lib.FQTK_EINVAL and case[2:] in _lib.last_error()
        assert call(obs.ctypes.data, qual.ctypes.data, L) == _lib.FQTK_EINVAL
    elif case == "before set_weighted":
        assert call(obs.ctypes.data, qual.ctypes.data, L) == _lib.FQTK_EINVAL and "set_weighted" in _lib.last_error()
    else:
        m.set_weighted(100, 10)
        if case == "NULL quality":
            assert call(obs.ctypes.data, None, L) == _lib.FQTK_EINVAL and "qual" in _lib.last_error()
        else:
            assert call(obs.ctypes.data, qual.ctypes.data, L - 1) == _lib.FQTK_EINVAL and "stride" in _lib.last_error()
        with pytest.raises(ValueError):
            m.assign_batch_weighted_device(1, 0, L, 100, 1)
    after, after_counts = m.assign_batch(obs)
    assert np.array_equal(before, after) and np.array_equal(before_counts, after_counts)


def write_fastq(tmp, name, bases, quals):
    path = tmp / f"{name}.fastq"
    path.write_text("".join(f"@ex_{i}\n{b.tobytes().decode()}\n+\n{q.tobytes().decode()}\n" for i, (b, q) in enumerate(zip(bases, quals))))
    return path


@pytest.mark.parametrize("extra", [[], ["--devices", "0,0", "--chunk-reads", "1000"]])
def test_cli_quality_weighted(tmp_path, extra):
    from tests import hostlib as H
    rng = np.random.default_rng(11)
    barcodes = make_table(rng, 24, 16, 0.0)
    n = 3000
    obs = make_reads(rng, barcodes, n)
    qual = rng.integers(ord("#"), ord("K") + 1, size=obs.shape, dtype=np.uint8)
    idx, _, _, counts = reference(barcodes, obs, qual, 60, 30)
    assert counts[-1] and (counts[:-1] > 0).all()
    tmpl = np.full((n, 8), ord("A"), dtype=np.uint8)
    files = [write_fastq(tmp_path, "i1", obs[:, :8], qual[:, :8]), write_fastq(tmp_path, "i2", obs[:, 8:], qual[:, 8:]),
             write_fastq(tmp_path, "r1", tmpl, np.full_like(tmpl, ord(";")))]
    out = tmp_path / "out"
    r = H.run_demux(files, ["8B", "8B", "+T"], H.metadata_file(tmp_path, barcodes), out, extra=extra + ["--quality-weighted", "60,30"])
    assert r.returncode == 0, r.stderr
    assert "--max-mismatches and --min-mismatch-delta are ignored" in r.stderr
    rows = [l.split("\t") for l in open(out / "demux-metrics.txt").read().splitlines()[1:]]
    assert [int(row[2]) for row in rows] == [int(c) for c in counts]
    for s in range(24):
        assert [h.split()[0] for h, _, _ in H.read_fastq(out / f"Sample{s:04}.R1.fq.gz")] == [f"ex_{i}" for i in np.nonzero(idx == s)[0]]
    assert len(H.read_fastq(out / "unmatched.R1.fq.gz")) == counts[-1]


@pytest.mark.parametrize("rs,extra,sentence", [(["8B", "8B", "+T"], ["--host-output"], "the host routers carry no quality rows"),
                                               (["8B", "+B", "+T"], [], "variable length"),
                                               (["8B", "8B", "+T"], ["--quality-metrics"], "saturated cost")])
def test_cli_quality_weighted_usage_errors(tmp_path, rs, extra, sentence):
    from tests import hostlib as H
    files = [H.fastq_file(tmp_path, k, "ex", ["ACGTACGT"] * 4) for k in ("i1", "i2", "r1")]
    r = H.run_demux(files, rs, H.metadata_file(tmp_path, ["ACGTACGTACGTACGT", "TTTTACGTACGTAAAA"]), tmp_path / "out",
                    extra=extra + ["--quality-weighted", "60,30"])
    assert r.returncode == 1 and sentence in r.stderr
