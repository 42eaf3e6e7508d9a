"""The index-pair tally of the unmatched reads (fqtk_matcher_pairs_*, `fqtk demux --index-pairs`) against the CPU oracle:
oracle.RefLiteral over the whole rows finds the None reads, RefLiteral over each index's distinct strings and the reads'
column slices assigns the two indexes, np.add.at makes the matrix.  Integer code: every comparison is exact."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from fqtk_amd import BarcodeMatcher  # noqa: E402
from oracle.oracle import RefLiteral  # noqa: E402

NONE = 0xFFFF


def table(seed, len_a, len_b, n_a, n_b, comb, iupac=False):
    """(barcodes, A, B): n_a x n_b combinatorial minus the last pair, or n_a == n_b unique-dual (n_a == 1: one A for every B)."""
    rng = np.random.default_rng(seed)

    def distinct(n, length):
        out = {}
        while len(out) < n:
            out["".join(rng.choice(list("ACGT"), length))] = None
        return list(out)
    A, B = distinct(n_a, len_a), distinct(n_b, len_b)
    if iupac:
        A[0], B[1] = A[0][:3] + "N" + A[0][4:], B[1][:2] + "R" + B[1][3:]
    bcs = [a + b for a in A for b in B][:-1] if comb else [A[i % n_a] + b for i, b in enumerate(B)]
    return bcs, A, B


def draw(seed, A, B, n):
    """Index 1 and index 2 each at random from the run's own lists (hopped pairs), 15 % of reads random, 4 % of bytes from ACGTNn.RX."""
    rng = np.random.default_rng(seed)
    rows = lambda lst: np.array([list(s.encode()) for s in lst], dtype=np.uint8)  # noqa: E731
    obs = np.concatenate([rows(A)[rng.integers(0, len(A), n)], rows(B)[rng.integers(0, len(B), n)]], axis=1)
    rnd = rng.random(n) < 0.15
    obs[rnd] = rng.choice(np.frombuffer(b"ACGT", np.uint8), (int(rnd.sum()), obs.shape[1]))
    hit = rng.random(obs.shape) < 0.04
    obs[hit] = np.frombuffer(b"ACGTNn.RX", np.uint8)[rng.integers(0, 9, int(hit.sum()))]
    return np.ascontiguousarray(obs)


def expected(bcs, A, B, obs, lens=None, mi=1, di=2):
    """(matrix, skipped, number of None reads); the whole-barcode matcher is always 1 / 2."""
    L, len_a = len(bcs[0]), len(A[0])
    idx = RefLiteral(bcs, 1, 2).assign_batch(obs if lens is not None else obs[:, :L], lens)[0]
    none = idx == NONE
    tallied = none & (obs.shape[1] >= L) & (True if lens is None else lens == L)
    mat = np.zeros((len(A) + 1, len(B) + 1), dtype=np.uint64)
    if tallied.any():
        rows = obs[tallied]
        a = RefLiteral(A, mi, di).assign_batch(rows[:, :len_a])[0].astype(np.int64)
        b = RefLiteral(B, mi, di).assign_batch(rows[:, len_a:L])[0].astype(np.int64)
        np.add.at(mat, (np.where(a == NONE, len(A), a), np.where(b == NONE, len(B), b)), 1)
    return mat, int(none.sum() - tallied.sum()), int(none.sum())


def reaches_every_region(mat):
    return mat[:-1, :-1].any() and (mat[-1, :-1].any() or mat[:-1, -1].any())


# (len_a, len_b, U_A, U_B, combinatorial, per-index max_mismatches, per-index min_mismatch_delta)
SHAPES = {"8+8 4x3": (8, 8, 4, 3, True, 1, 2), "8+8 96 dual": (8, 8, 96, 96, False, 1, 2), "16+16 5 dual": (16, 16, 5, 5, False, 1, 2),
          "6+8 one A": (6, 8, 1, 5, False, 1, 2), "1+7 4x3": (1, 7, 4, 3, True, 0, 1), "7+1 4x3": (7, 1, 4, 3, True, 0, 1)}


@functools.lru_cache(maxsize=None)
def shape_case(name, use_cache):
    """The shape's table, its 3000 reads and ONE matcher with the tally on (creating a matcher builds its memo)."""
    len_a, len_b, n_a, n_b, comb, mi, di = SHAPES[name]
    bcs, A, B = table(len_a * 100 + n_b, len_a, len_b, n_a, n_b, comb)
    obs = draw(len_a, A, B, 3000)
    assert reaches_every_region(expected(bcs, A, B, obs, None, mi, di)[0]), "change the draw"
    m = BarcodeMatcher(bcs, 1, 2, use_cache=use_cache)
    m.enable_pairs(len_a, mi, di)
    return bcs, A, B, obs, m


@pytest.mark.parametrize("use_cache", [True, False])
@pytest.mark.parametrize("n", [1, 63, 64, 3000])
@pytest.mark.parametrize("name", list(SHAPES))
def test_parity(name, n, use_cache):
    bcs, A, B, obs, m = shape_case(name, use_cache)
    mi, di = SHAPES[name][5:]
    assert m.pair_indexes() == (A, B)
    m.reset_pairs()
    mat, skipped, n_none = expected(bcs, A, B, obs[:n], None, mi, di)
    _, counts = m.assign_batch(obs[:n])
    got, got_skipped = m.pairs()
    assert got.dtype == np.uint64 and np.array_equal(got, mat) and got_skipped == skipped == 0
    assert int(got.sum()) + got_skipped == n_none == int(counts[-1])


def test_stride_and_lengths():
    """Rows at stride L + 3 (odd addresses); then obs_len with shorter reads and longer ones the no-call prefilter rejects."""
    bcs, A, B = table(1, 8, 8, 4, 3, True)
    L, n = 16, 3000
    pad = np.full((n, L + 3), ord("G"), np.uint8)
    pad[:, :L] = draw(2, A, B, n)
    lens = np.full(n, L, np.uint32)
    lens[::7] = L - 1
    lens[3::11] = L + 3
    m = BarcodeMatcher(bcs, 1, 2)
    m.enable_pairs(8)
    for ln in (None, lens):
        if ln is not None:
            pad[3::11, L - 2:] = ord("N")
        m.reset_pairs()
        mat, skipped, n_none = expected(bcs, A, B, pad, ln)
        _, counts = m.assign_batch(pad, ln)
        got, got_skipped = m.pairs()
        assert reaches_every_region(mat) and (ln is None or skipped > 0)
        assert np.array_equal(got, mat) and got_skipped == skipped
        assert int(got.sum()) + got_skipped == n_none == int(counts[-1])


@pytest.mark.parametrize("kind", ["all None", "no None", "N and IUPAC in the sample indexes"])
def test_extremes(kind):
    bcs, A, B = table(3, 8, 8, 4, 3, True, iupac=kind.startswith("N"))
    if kind == "all None":   # reads of a foreign table
        obs = draw(5, *table(4, 8, 8, 4, 3, True)[1:], 3000)
    elif kind == "no None":
        obs = np.array([list(b.encode()) for b in bcs] * 30, dtype=np.uint8)
    else:
        obs = draw(6, A, B, 3000)
    mat, skipped, n_none = expected(bcs, A, B, obs)
    assert {"all None": n_none == 3000, "no None": n_none == 0}.get(kind, reaches_every_region(mat))
    m = BarcodeMatcher(bcs, 1, 2)
    m.enable_pairs(8)
    m.assign_batch(obs)
    got, got_skipped = m.pairs()
    assert np.array_equal(got, mat) and got_skipped == skipped == 0 and int(got.sum()) == n_none


def test_accumulation_and_lifetime():
    bcs, A, B, obs, _ = shape_case("8+8 4x3", True)
    mat, skipped, _ = expected(bcs, A, B, obs)
    fresh = BarcodeMatcher(bcs, 1, 2)
    plain, plain_counts = fresh.assign_batch(obs)
    fresh.enable_census()
    fresh.assign_batch(obs)
    m = BarcodeMatcher(bcs, 1, 2)
    with pytest.raises(ValueError, match="not enabled"):
        m.pairs()
    m.enable_pairs(8)
    m.enable_census()
    for part in np.array_split(obs, 2):   # two batches accumulate; the census runs beside the tally
        m.assign_batch(part)
    got, got_skipped = m.pairs()
    assert np.array_equal(got, mat) and got_skipped == skipped
    assert m.census_totals() == fresh.census_totals() and m.census_top(50) == fresh.census_top(50)
    m.reset_pairs()
    got, got_skipped = m.pairs()
    assert not got.any() and got_skipped == 0 and got.shape == (5, 4)
    m.disable_pairs()
    m.disable_census()
    after, after_counts = m.assign_batch(obs)
    assert np.array_equal(after, plain) and np.array_equal(after_counts, plain_counts)
    with pytest.raises(ValueError, match="len_a"):
        m.enable_pairs(0)
    with pytest.raises(ValueError, match="len_a"):
        m.enable_pairs(16)
    with pytest.raises(ValueError, match="32 bases"):
        BarcodeMatcher(["A" * 33, "C" * 33], 1, 2).enable_pairs(16)
    big = table(7, 8, 8, 4097, 4097, False)[0]   # 4098^2 cells > 2^24
    with pytest.raises(ValueError, match="2\\^24"):
        BarcodeMatcher(big, 1, 2, use_cache=False).enable_pairs(8)


@pytest.mark.parametrize("path", ["device", "host", "devices"])
def test_cli_index_pairs(tmp_path, path):
    from tests import hostlib as H
    bcs, A, B = table(8, 8, 8, 4, 3, True)
    obs = draw(9, A, B, 4000)
    mat, skipped, _ = expected(bcs, A, B, obs)
    assert reaches_every_region(mat)
    names = (A + ["*"], B + ["*"])
    ids = {b: f"Sample{i:04}" for i, b in enumerate(bcs)}
    cells = sorted((-int(mat[a, b]), names[0][a], names[1][b]) for a, b in zip(*np.nonzero(mat)))
    want = "index_1\tindex_2\ttemplates\tsample_id\n" + "".join(f"{a}\t{b}\t{-c}\t{ids.get(a + b, '-')}\n" for c, a, b in cells)
    want += f"*\t*\t{skipped}\tskipped\n"
    reads = [r.tobytes().decode() for r in obs]
    i1 = H.fastq_file(tmp_path, "i1", "ex", [r[:8] for r in reads])
    i2 = H.fastq_file(tmp_path, "i2", "ex", [r[8:] for r in reads])
    r1 = H.fastq_file(tmp_path, "r1", "ex", ["ACGTACGT"] * len(reads))
    meta = H.metadata_file(tmp_path, bcs)
    extra = {"device": [], "host": ["--host-output"], "devices": ["--devices", "0,0", "--chunk-reads", "1000"]}[path]
    r = H.run_demux([i1, i2, r1], ["8B", "8B", "+T"], meta, tmp_path / "out", extra=extra + ["--index-pairs"])
    assert r.returncode == 0, r.stderr
    assert open(tmp_path / "out" / "index-pairs.txt").read() == want
    r = H.run_demux([i1, r1], ["8B", "+T"], meta, tmp_path / "single", extra=extra + ["--index-pairs"])
    assert r.returncode != 0 and "exactly two sample-barcode (B) segments of fixed length" in r.stderr
