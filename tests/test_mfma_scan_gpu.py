"""The exhaustive scan on the matrix cores (fqtk::mfma_scan_kernel) against the literal oracle and against the VALU scan
of the same matcher: exact equality of (idx, best, next), the counts and any length error, at the shapes where the kernel
takes another path -- K-step and tile edges, a table past one LDS staging, flagged (two- and three-bit) read codes, the
14 index bits of the accumulator key."""
import numpy as np
import pytest

from fqtk_amd import BarcodeMatch, BarcodeMatcher, FqtkLengthError
from oracle import oracle as O

pytestmark = pytest.mark.gpu

CODES = np.frombuffer(b"ACGTMRWSYKVHDBN", dtype=np.uint8)
DT = np.dtype([("idx", "<u2"), ("best", "u1"), ("next", "u1")])


def make_table(rng, S, L, iupac=0.1):
    t = rng.choice(CODES[:4], size=(S, L))
    amb = rng.random((S, L)) < iupac
    t[amb] = rng.choice(CODES, size=int(amb.sum()))
    return [r.tobytes().decode() for r in t]


def make_reads(rng, barcodes, n):
    """Rows of the table with substitutions and N; a two- or three-bit code of the table becomes a base in the read, so the
    reads are one-hot / N and the accumulators decide them (test_every_byte_value_at_every_position has the flagged codes)."""
    tab = np.frombuffer("".join(barcodes).encode(), dtype=np.uint8).reshape(len(barcodes), -1)
    obs = tab[rng.integers(len(barcodes), size=n)].copy()
    sub = (rng.random(obs.shape) < 0.08) | ~np.isin(obs, np.frombuffer(b"ACGTN", dtype=np.uint8))
    obs[sub] = rng.choice(np.frombuffer(b"ACGTN", dtype=np.uint8), size=int(sub.sum()))
    return obs


def mfma_matcher(barcodes, mm, delta):
    m = BarcodeMatcher(barcodes, mm, delta, use_cache=False)
    m.scan_kind = m.SCAN_MFMA
    assert m.scan_kind == m.SCAN_MFMA
    return m


def check(barcodes, mm, delta, obs, lens=None):
    m = mfma_matcher(barcodes, mm, delta)
    got, cnt = m.assign_batch(obs, lens)
    i, b, nx, c = O.RefLiteral(barcodes, mm, delta, False).assign_batch(obs, lens)
    assert np.array_equal(got["idx"], i) and np.array_equal(got["best"], b) and np.array_equal(got["next"], nx)
    assert np.array_equal(cnt, c)
    m.scan_kind = m.SCAN_VALU
    assert m.scan_kind == m.SCAN_VALU
    got2, cnt2 = m.assign_batch(obs, lens)
    assert np.array_equal(got, got2) and np.array_equal(cnt, cnt2)


# (S, L, n): 5 channels per base + 2 index channels in 32-wide K steps -> L = 12 | 13, 24 | 25 change the step count, 16 | 17
# and 32 | 33 the kernel variant, 64 | 65 and 96 | 97 its plane words; 1500 x 16, 385 x 80 and 385 x 128 do not fit one LDS staging
@pytest.mark.parametrize("S,L,n", [(1, 1, 1), (2, 8, 63), (31, 12, 64), (32, 13, 65), (33, 16, 3001), (385, 25, 3001),
                                   (385, 26, 65), (33, 32, 3001), (32, 33, 64), (385, 64, 3001), (385, 128, 1000),
                                   (2, 128, 63), (1500, 16, 3001), (64, 24, 1), (385, 17, 65), (385, 80, 1000), (33, 65, 65),
                                   (33, 97, 65)])
def test_tile_edges(S, L, n):
    rng = np.random.default_rng(1000 * S + L)
    barcodes = make_table(rng, S, L)
    check(barcodes, L // 2 + 1, 1, make_reads(rng, barcodes, n))   # the bound is loose: most reads are Some, and show their counts


@pytest.mark.parametrize("L", [16, 33])
@pytest.mark.parametrize("iupac", [0.0, 0.5])
def test_every_byte_value_at_every_position(L, iupac):
    rng = np.random.default_rng(L)
    barcodes = make_table(rng, 5, L, iupac)
    tab = np.frombuffer("".join(barcodes).encode(), dtype=np.uint8).reshape(5, L)
    obs = tab[np.arange(L * 256) % 5].copy()
    obs[np.arange(L * 256), np.repeat(np.arange(L), 256)] = np.tile(np.arange(256, dtype=np.uint8), L)
    check(barcodes, 2, 1, obs)


@pytest.mark.parametrize("mm,delta", [(0, 0), (255, 0), (1, 2), (255, 255), (0, 1)])
def test_decision_edges(mm, delta):
    reads = np.frombuffer(b"ACGTNNNNACGAACGRTTTTACNN....nnnn", dtype=np.uint8).reshape(-1, 4)
    check(["NNNN"], mm, delta, reads)                                # S = 1: next is 255
    check(["ACGN", "ACGT", "ACGR", "NNNN", "TTTT"], mm, delta, reads)   # ties: lowest index wins, next == best


def test_assign_known_answers(kat):
    for c in kat["assign"]["cases"]:
        m = mfma_matcher(c["barcodes"], c["max_mismatches"], c["min_mismatch_delta"])
        expected = None if c["expect"] is None else BarcodeMatch(*c["expect"])
        assert m.assign(c["read"].encode()) == expected, c["name"]


def test_lengths():
    import torch
    rng = np.random.default_rng(4)
    barcodes = make_table(rng, 40, 13)
    n, L, stride, off = 200, 13, 19, 3
    obs = np.full((n, stride), ord("N"), dtype=np.uint8)             # what follows the barcode is no-calls
    obs[:, :L] = make_reads(rng, barcodes, n)
    lens = np.full(n, L, dtype=np.uint32)
    lens[::7] = rng.integers(0, L, size=len(lens[::7]))              # shorter: None
    lens[3::11] = stride                                             # longer, 6 no-calls > 2 + max_ns: the prefilter's None
    check(barcodes, 2, 1, obs, lens)
    # a longer read the prefilter lets through: the lowest index is reported, every other result is written
    bad = [57, 120]
    obs[bad] = ord("A")
    lens[bad] = L + 2
    exp_lens = lens.copy()
    exp_lens[bad] = 0                                                # its own result is None
    i, b, nx, c = O.RefLiteral(barcodes, 2, 1, False).assign_batch(obs, exp_lens)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    raw = torch.zeros(off + n * stride + 16, dtype=torch.uint8, device=dev)      # stride > L, unaligned base
    raw[off:off + n * stride] = torch.from_numpy(obs.reshape(-1)).to(dev)
    d_lens = torch.from_numpy(lens.astype(np.int32)).to(dev)
    d_out = torch.empty(n, dtype=torch.int32, device=dev)
    d_counts = torch.zeros(len(barcodes) + 1, dtype=torch.int64, device=dev)
    m = mfma_matcher(barcodes, 2, 1)
    m.assign_batch_device(raw.data_ptr() + off, stride, n, d_out.data_ptr(), d_counts.data_ptr(), d_lens.data_ptr(), stream)
    with pytest.raises(FqtkLengthError, match=r"\[read index 57 of its batch\]"):
        m.poll_error(stream)
    got = d_out.cpu().numpy().view(DT)
    assert np.array_equal(got["idx"], i) and np.array_equal(got["best"], b) and np.array_equal(got["next"], nx)
    assert np.array_equal(d_counts.cpu().numpy().astype(np.uint64), c)


def test_sample_count_bound():
    def words(S, L):   # every L-letter word over ACGT, in index order
        d = (np.arange(S)[:, None] >> (2 * np.arange(L)[::-1])) & 3
        return [r.tobytes().decode() for r in CODES[:4][d]]
    barcodes = words(16384, 7)                                       # the largest eligible table
    pick = [0, 127, 128, 8191, 8192, 16382, 16383]
    obs = np.frombuffer("".join(barcodes[s] for s in pick).encode(), dtype=np.uint8).reshape(-1, 7)
    check(barcodes, 0, 1, obs)
    m = mfma_matcher(barcodes, 0, 1)
    assert list(m.assign_batch(obs)[0]["idx"]) == pick
    barcodes = words(16385, 8)                                       # one above: the VALU scan serves
    obs = np.frombuffer("".join(barcodes[s] for s in (0, 16383, 16384)).encode(), dtype=np.uint8).reshape(-1, 8)
    m = BarcodeMatcher(barcodes, 0, 1, use_cache=False)
    with pytest.raises(ValueError, match="16384"):
        m.scan_kind = m.SCAN_MFMA
    assert m.scan_kind == m.SCAN_VALU
    assert list(m.assign_batch(obs)[0]["idx"]) == [0, 16383, 16384]
