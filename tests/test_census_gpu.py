"""The census of unmatched barcodes (fqtk_matcher_census_*, `fqtk demux --top-unmatched`) against plain Python: the reads
oracle.RefLiteral assigns None, keyed by the reference's encode() / spelled by its decode(), counted with a Counter.  Integer
code: every comparison is exact."""
import os
from collections import Counter

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from fqtk_amd import BarcodeMatcher  # noqa: E402
from oracle.oracle import RefLiteral  # noqa: E402

ENC = {"A": 1, "C": 2, "G": 4, "T": 8, "U": 8, "M": 3, "R": 5, "W": 9, "S": 6, "Y": 10, "K": 12, "V": 7, "H": 11, "D": 13, "B": 14, "N": 15}
DEC = {v: k for k, v in ENC.items() if k != "U"}


def key_of(row: bytes):
    """The reported barcode of a read of exactly L bases, or None when a byte encodes to 0 (mod.rs:26-61, :68)."""
    e = [15 if c in "Nn." else ENC.get(c.upper(), 0) for c in row.decode("latin-1")]
    return None if 0 in e else "".join(DEC[x] for x in e)


def expected(bcs, obs, lens=None, mm=1, delta=2):
    """(Counter of the keyed None reads, number of unkeyed None reads, number of None reads)."""
    L = len(bcs[0])
    # (without lens the matcher takes every read as its first L bases; the oracle takes the whole row)
    idx = RefLiteral(bcs, mm, delta).assign_batch(obs if lens is not None else obs[:, :L], lens)[0]
    keyed, unkeyed = Counter(), 0
    for i in np.flatnonzero(idx == 0xFFFF):
        k = key_of(obs[i, :L].tobytes()) if obs.shape[1] >= L and (lens is None or lens[i] == L) else None
        if k is None:
            unkeyed += 1
        else:
            keyed[k] += 1
    return keyed, unkeyed, int((idx == 0xFFFF).sum())


def ordered(counter):
    return sorted(counter.items(), key=lambda kv: (-kv[1], kv[0]))


def draw(rng, L, n, S=5):
    """A table and n reads over it: table rows with substitutions, a small pool of foreign barcodes, all-N, lower case and '.',
    IUPAC codes, junk bytes."""
    S = min(S, 4 ** L)
    bcs = sorted({"".join(rng.choice(list("ACGT"), L)) for _ in range(40)})[:S]
    tab = np.array([list(b.encode()) for b in bcs], dtype=np.uint8)
    pool = rng.choice(np.frombuffer(b"ACGT", np.uint8), (7, L))
    obs = np.where((rng.random(n) < 0.5)[:, None], tab[rng.integers(0, len(bcs), n)], pool[rng.integers(0, 7, n)])
    for frac, alphabet in ((0.04, b"ACGTN"), (0.01, b"acgtn."), (0.01, b"MRWSYKVHDBU"), (0.003, b"X@\x00\xff")):
        hit = rng.random(obs.shape) < frac
        obs[hit] = np.frombuffer(alphabet, np.uint8)[rng.integers(0, len(alphabet), int(hit.sum()))]
    obs[rng.random(n) < 0.02] = ord("N")
    return bcs, np.ascontiguousarray(obs)


def check(m, keyed, unkeyed, n_none):
    t = m.census_totals()
    assert m.census_top(len(keyed) + 3) == ordered(keyed)
    assert t == (len(keyed), sum(keyed.values()), unkeyed, 0)
    assert t.keyed + t.unkeyed + t.overflow == n_none


@pytest.mark.parametrize("use_cache", [True, False])
@pytest.mark.parametrize("L", [1, 8, 16, 17, 32])
def test_parity_at_the_edges_of_the_key(L, use_cache):
    rng = np.random.default_rng(L)
    bcs, obs = draw(rng, L, 3000)
    pad = np.full((3000, L + 3), ord("G"), np.uint8)   # stride > L, rows at odd addresses
    pad[:, :L] = obs
    m = BarcodeMatcher(bcs, 1, 2, use_cache=use_cache)
    m.enable_census()
    for o in (obs, pad):
        m.reset_census()
        keyed, unkeyed, n_none = expected(bcs, o)
        _, counts = m.assign_batch(o)
        assert n_none == int(counts[-1]) and unkeyed > 0 and len(keyed) > 1
        check(m, keyed, unkeyed, n_none)
    # obs_len: shorter reads, and longer ones the no-call prefilter rejects (every base beyond L, and two more, are N)
    lens = np.full(3000, L, np.uint32)
    lens[::7] = L - 1
    lens[3::11] = L + 3
    pad[3::11, max(L - 2, 0):] = ord("N")
    m.reset_census()
    keyed, unkeyed, n_none = expected(bcs, pad, lens)
    _, counts = m.assign_batch(pad, lens)
    assert n_none == int(counts[-1])
    check(m, keyed, unkeyed, n_none)


def test_order_and_cut():
    """Ties at the cut: the barcode decides."""
    bcs = ["ACGTACGT", "TTTTAAAA"]
    foreign = {"GGGGGGGG": 5, "CCCCCCCC": 3, "CACACACA": 3, "AGAGAGAG": 3, "NNNNNNNN": 3, "GTGTGTGT": 1}
    rows = [b for b, c in foreign.items() for _ in range(c)] + bcs * 4
    obs = np.array([list(r.encode()) for r in rows], dtype=np.uint8)
    m = BarcodeMatcher(bcs, 1, 2)
    m.enable_census()
    m.assign_batch(obs)
    full = ordered(Counter(foreign))
    assert [b for b, _ in full[:5]] == ["GGGGGGGG", "AGAGAGAG", "CACACACA", "CCCCCCCC", "NNNNNNNN"]
    for k in range(0, 8):
        assert m.census_top(k) == full[:k]


def test_skew():
    bcs = ["ACGTACGTAC", "TTTTAAAACC"]
    obs = np.tile(np.frombuffer(b"GGGGGGGGGG", np.uint8), (70001, 1))
    obs[[5, 69000]] = np.frombuffer(b"CCCCCCCCCA", np.uint8)
    m = BarcodeMatcher(bcs, 1, 2)
    m.enable_census()
    m.assign_batch(obs)
    assert m.census_top(10) == [("GGGGGGGGGG", 69999), ("CCCCCCCCCA", 2)]
    assert m.census_totals() == (2, 70001, 0, 0)


def test_overflow():
    rng = np.random.default_rng(4)
    bcs = ["ACGTACGTACGT", "TTTTAAAACCCC"]
    obs = rng.choice(np.frombuffer(b"ACGT", np.uint8), (2000, 12))[rng.integers(0, 2000, 6000)]
    keyed, unkeyed, n_none = expected(bcs, obs)
    assert len(keyed) > 1500
    m = BarcodeMatcher(bcs, 1, 2)
    m.enable_census(64)
    m.assign_batch(obs)
    t, rows = m.census_totals(), m.census_top(1000)
    assert t.overflow > 0 and t.distinct <= 64 and t.distinct == len(rows) == len({b for b, _ in rows})
    assert all(keyed[b] == c for b, c in rows)
    assert t.keyed == sum(c for _, c in rows) and t.keyed + t.unkeyed + t.overflow == n_none


def test_accumulation_and_lifetime():
    import torch
    rng = np.random.default_rng(9)
    bcs, obs = draw(rng, 16, 5000)
    parts = np.array_split(obs, 5)
    m = BarcodeMatcher(bcs, 1, 2)
    plain, plain_counts = m.assign_batch(obs)
    with pytest.raises(ValueError, match="not enabled"):
        m.census_top(1)
    m.enable_census()
    for p in parts[:2]:
        m.assign_batch(p)
    outs = [np.empty(len(p), dtype=np.uint32) for p in parts[2:4]]
    for slot, (p, o) in enumerate(zip(parts[2:4], outs)):
        assert m._lib.fqtk_matcher_enqueue(m.handle, slot, p.ctypes.data, 16, None, len(p), o.ctypes.data) == 0
    for slot in (0, 1):
        assert m._lib.fqtk_matcher_wait(m.handle, slot) == 0
    d = torch.from_numpy(parts[4]).cuda()
    out = torch.empty(len(parts[4]), dtype=torch.int32, device="cuda")
    m.assign_batch_device(d.data_ptr(), 16, len(parts[4]), out.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    check(m, *expected(bcs, obs))
    with_census, with_counts = m.assign_batch(obs)   # the census changes no result
    assert np.array_equal(plain, with_census) and np.array_equal(plain_counts, with_counts)
    m.reset_census()
    assert m.census_totals() == (0, 0, 0, 0) and m.census_top(5) == []
    m.disable_census()
    m.assign_batch(obs)
    m.enable_census()
    assert m.census_totals() == (0, 0, 0, 0)
    with pytest.raises(ValueError, match="32"):
        BarcodeMatcher(["A" * 33, "C" * 33], 1, 2).enable_census()


@pytest.mark.parametrize("path", ["device", "host"])
def test_cli_top_unmatched(tmp_path, path):
    from tests import hostlib as H
    bcs = ["AAAAAAAACCCCCCCC", "GGGGGGGGTTTTTTTT"]
    foreign = {"ACACACACGTGTGTGT": 4, "NNNNNNNNNNNNNNNN": 3, "CCCCCCCCAAAAAAAA": 3, "TTTTTTTTGGGGGGGG": 2, "AGAGAGAGAGAGAGAG": 1,
               "GAGAGAGAGAGAGAGA": 1}
    reads = [b for b, c in foreign.items() for _ in range(c)] + bcs * 3
    i1 = H.fastq_file(tmp_path, "i1", "ex", [r[:8] for r in reads])
    i2 = H.fastq_file(tmp_path, "i2", "ex", [r[8:] for r in reads])
    r1 = H.fastq_file(tmp_path, "r1", "ex", ["ACGTACGT"] * len(reads))
    meta = H.metadata_file(tmp_path, bcs)
    extra = ["--host-output"] if path == "host" else []
    want = "barcode\ttemplates\n" + "".join(f"{b}\t{c}\n" for b, c in ordered(Counter(foreign))[:5])
    for name, more in (("one", []), ("two", ["--devices", "0,0", "--chunk-reads", "4"])):
        out = tmp_path / name
        r = H.run_demux([i1, i2, r1], ["8B", "8B", "+T"], meta, out, extra=extra + more + ["--top-unmatched", "5"])
        assert r.returncode == 0, r.stderr
        assert open(out / "unmatched-barcodes.txt").read() == want
    r = H.run_demux([i1, i2, r1], ["8B", "8B", "+T"], meta, tmp_path / "off", extra=extra)
    assert r.returncode == 0 and not os.path.exists(tmp_path / "off" / "unmatched-barcodes.txt")
