"""Per-index mismatch budgets (fqtk::per_index_kernel and the per-index scan) against the rule of include/fqtk_match.h written
out in numpy: exact equality of idx, best, next and the counts, at the splits, budgets and table shapes where the kernels take
another path."""
import numpy as np
import pytest

from fqtk_amd import BarcodeMatcher, _lib
from oracle import oracle as O

pytestmark = pytest.mark.gpu

DT = np.dtype([("idx", "<u2"), ("best", "u1"), ("next", "u1")])
BUDGETS = [((0, 1), (1, 1)), ((1, 1), (1, 1)), ((1, 1), (2, 2)), ((2, 1), (1, 1))]   # (mm_a, mm_b), (delta_a, delta_b)


def rows_of(strings):
    return np.frombuffer("".join(strings).encode("latin-1"), dtype=np.uint8).reshape(len(strings), -1)


def reference(barcodes, len_a, mm, delta, obs):
    """(idx, best, next, counts) of the rule; None rows are (0xFFFF, 255, 255)."""
    L, n = len(barcodes[0]), len(obs)
    ok, entry, best, nxt, lists = np.ones(n, bool), [], [], [], []
    for w, (lo, hi) in enumerate([(0, len_a), (len_a, L)]):
        lst = list(dict.fromkeys(b[lo:hi] for b in barcodes))                       # distinct, in order of first appearance
        cnt = ((O.ENC[obs[:, lo:hi]][:, None, :] & ~O.ENC[rows_of(lst)][None]) != 0).sum(-1)
        srt = np.sort(cnt, axis=1)
        b, x = srt[:, 0], (srt[:, 1] if len(lst) > 1 else np.full(n, 255))
        ok &= (b <= mm[w]) & (x - b >= delta[w])
        entry.append(cnt.argmin(1)), best.append(b), nxt.append(x), lists.append(lst)
    sample = {}
    for s, b in enumerate(barcodes):
        sample.setdefault((lists[0].index(b[:len_a]), lists[1].index(b[len_a:])), s)
    idx = np.array([sample.get((a, b), 0xFFFF) if k else 0xFFFF for a, b, k in zip(entry[0], entry[1], ok)])
    none = idx == 0xFFFF
    counts = np.bincount(np.where(none, len(barcodes), idx), minlength=len(barcodes) + 1).astype(np.uint64)
    nx = np.minimum(255, np.minimum(nxt[0] + best[1], best[0] + nxt[1]))
    return idx, np.where(none, 255, best[0] + best[1]), np.where(none, 255, nx), counts


def make_table(rng, kind, len_a, len_b):
    def distinct(k, length):
        out = set()
        while len(out) < k:
            out.add("".join(rng.choice(list("ACGT"), length)))
        return sorted(out)
    if kind == "combinatorial":                                                     # 3 x 4 indexes, 10 of the 12 pairs are samples
        a, b = distinct(3, len_a), distinct(4, len_b)
        return [x + y for x in a for y in b][1:11]
    if kind == "single":                                                            # index 1 has one value: next_a = 255
        a = distinct(1, len_a)[0]
        return [a + y for y in distinct(7, len_b)]
    a, b = distinct(24, len_a), distinct(24, len_b)
    table = [x + y for x, y in zip(a, b)]                                           # unique dual index
    if kind == "iupac":
        table[5] = "R" + table[5][1:]
    return table


def make_reads(rng, barcodes, len_a, n):
    L = len(barcodes[0])
    tab = rows_of(barcodes)
    obs = tab[rng.integers(0, len(barcodes), n)].copy()
    obs[n // 2:, :len_a] = tab[rng.integers(0, len(barcodes), n - n // 2), :len_a]  # pairs that may be no sample's
    subs = np.frombuffer(b"ACGTNacgtn.", dtype=np.uint8)
    for lo, hi in [(0, len_a), (len_a, L)]:                                         # 0-2 substitutions per index
        k = rng.integers(0, 3, n)
        for j in range(2):
            hit = np.nonzero(k > j)[0]
            obs[hit, rng.integers(lo, hi, len(hit))] = rng.choice(subs, len(hit))
    edge = np.array([0, len_a - 1, len_a, L - 1])
    for j, byte in enumerate([ord("R"), ord("y"), 0x00, 0xFF, ord("U")]):           # odd bytes at the first and last base of each index
        hit = np.arange(10 + j, n, 37)
        obs[hit, edge[(hit // 37) % 4]] = byte
    obs[::53] = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), (len(obs[::53]), L))
    return obs


def check(got, want):
    out, cnt = got
    assert np.array_equal(out["idx"], want[0])
    assert np.array_equal(out["best"], want[1]) and np.array_equal(out["next"], want[2])
    assert np.array_equal(cnt, want[3]) and cnt.sum() == len(out)


@pytest.mark.parametrize("split", [(8, 8), (6, 8), (10, 10), (16, 16)])
@pytest.mark.parametrize("kind", ["combinatorial", "unique", "iupac", "single"])
def test_the_rule_on_both_paths(kind, split):
    len_a, L = split[0], sum(split)
    rng = np.random.default_rng(100 * len_a + L + len(kind))
    barcodes = make_table(rng, kind, *split)
    obs = make_reads(rng, barcodes, len_a, 4097)
    padded = np.concatenate([obs, rng.integers(0, 256, (len(obs), 3), dtype=np.uint8)], axis=1)   # stride = L + 3
    m = BarcodeMatcher(barcodes, 1, 1)
    assigned = 0
    for mm, delta in BUDGETS:
        m.set_per_index(len_a, mm[0], delta[0], mm[1], delta[1])
        m.per_index_kind = m.PER_INDEX_LDS
        assert m.per_index_kind == (m.PER_INDEX_LDS if kind != "iupac" and max(mm) <= 1 else m.PER_INDEX_SCAN)
        want = reference(barcodes, len_a, mm, delta, obs)
        assigned += int((want[0] != 0xFFFF).sum())
        check(m.assign_batch_per_index(obs), want)
        check(m.assign_batch_per_index(padded), want)
        for n in (1, 63):                                                           # a partial wave, a partial tile
            check(m.assign_batch_per_index(obs[:n]), reference(barcodes, len_a, mm, delta, obs[:n]))
        m.per_index_kind = m.PER_INDEX_SCAN                                         # the scan path, pinned: the same output
        check(m.assign_batch_per_index(obs), want)
    assert 4 * 4097 // 10 < assigned < 4 * 4097


def test_one_mismatch_in_each_index_is_assigned_only_by_the_new_call():
    rng = np.random.default_rng(3)
    barcodes = make_table(rng, "unique", 8, 8)
    obs = rows_of(barcodes).copy()
    obs[:, 2] = np.where(obs[:, 2] == ord("A"), ord("C"), ord("A"))
    obs[:, 13] = np.where(obs[:, 13] == ord("G"), ord("T"), ord("G"))
    m = BarcodeMatcher(barcodes, 1, 1)
    before = m.assign_batch(obs)
    assert (before[0]["idx"] == 0xFFFF).all()                                       # two mismatches over the whole barcode
    m.set_per_index(8, 1, 1, 1, 1)
    out, cnt = m.assign_batch_per_index(obs)
    assert np.array_equal(out["idx"], np.arange(24)) and (out["best"] == 2).all()
    check((out, cnt), reference(barcodes, 8, (1, 1), (1, 1), obs))
    after = m.assign_batch(obs)                                                     # the old entry point is untouched
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])


def test_device_entry_point_and_the_tallies_behind_a_batch():
    import torch
    rng = np.random.default_rng(4)
    barcodes = make_table(rng, "combinatorial", 8, 8)
    obs = make_reads(rng, barcodes, 8, 4097)
    m = BarcodeMatcher(barcodes, 1, 1)
    m.set_per_index(8, 1, 1, 1, 1)
    m.enable_census(1 << 14)
    m.enable_pairs(8, 1, 1)
    host = m.assign_batch_per_index(obs)
    none = int(host[1][-1])
    assert 0 < none < len(obs)
    t = m.census_totals()
    mat, skipped = m.pairs()
    assert t.keyed + t.unkeyed + t.overflow == none and int(mat.sum()) + skipped == none
    dev = torch.device("cuda:0")
    d_obs = torch.from_numpy(obs.reshape(-1)).to(dev)
    d_out = torch.empty(len(obs), dtype=torch.int32, device=dev)
    d_counts = torch.zeros(len(barcodes) + 1, dtype=torch.int64, device=dev)
    m.assign_batch_per_index_device(d_obs.data_ptr(), 16, len(obs), d_out.data_ptr(), d_counts.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(d_out.cpu().numpy().view(DT), host[0]) and np.array_equal(d_counts.cpu().numpy().astype(np.uint64), host[1])
    t = m.census_totals()
    assert t.keyed + t.unkeyed + t.overflow == 2 * none


@pytest.mark.parametrize("case", ["before set_per_index", "len_a = 0", "len_a = L", "index of 17 bases", "stride < L"])
def test_argument_errors(case):
    rng = np.random.default_rng(5)
    L = 24 if case == "index of 17 bases" else 16
    barcodes = make_table(rng, "unique", L // 2, L // 2)
    m = BarcodeMatcher(barcodes, 1, 1)
    obs = rows_of(barcodes).copy()
    out = np.empty(len(obs), dtype=DT)
    call = lambda stride: m._lib.fqtk_matcher_assign_per_index_batch(m.handle, obs.ctypes.data, stride, len(obs), out.ctypes.data, None)
    setup = lambda len_a: m._lib.fqtk_matcher_set_per_index(m.handle, len_a, 1, 1, 1, 1)
    if case == "before set_per_index":
        assert call(L) == _lib.FQTK_EINVAL and "set_per_index" in _lib.last_error()
    elif case == "stride < L":
        assert setup(8) == _lib.FQTK_OK
        assert call(L - 1) == _lib.FQTK_EINVAL and "stride" in _lib.last_error()
    else:
        len_a = {"len_a = 0": 0, "len_a = L": L, "index of 17 bases": 17}[case]
        assert setup(len_a) == _lib.FQTK_EINVAL and ("16 bases" if len_a == 17 else "len_a") in _lib.last_error()
        assert m.per_index_kind == m.PER_INDEX_OFF and call(L) == _lib.FQTK_EINVAL


def test_cli_per_index_mismatches(tmp_path):
    from tests import hostlib as H
    rng = np.random.default_rng(11)
    barcodes = make_table(rng, "unique", 8, 8)
    obs = make_reads(rng, barcodes, 8, 211)
    obs[~np.isin(obs, np.frombuffer(b"ACGTN", dtype=np.uint8))] = ord("N")          # what a FASTQ line can carry
    idx, _, _, counts = reference(barcodes, 8, (1, 1), (2, 2), obs)
    whole = BarcodeMatcher(barcodes, 1, 2).assign_batch(obs)[0]["idx"]
    assert counts[-1] and ((idx != 0xFFFF) & (whole == 0xFFFF)).any()               # templates only the per-index rule assigns
    fastq = lambda name, rows: H.fastq_file(tmp_path, name, "ex", [r.tobytes().decode() for r in rows])
    files = [fastq("i1", obs[:, :8]), fastq("i2", obs[:, 8:]), fastq("r1", np.full((len(obs), 8), ord("A"), dtype=np.uint8))]
    out = tmp_path / "out"
    r = H.run_demux(files, ["8B", "8B", "+T"], H.metadata_file(tmp_path, barcodes), out,
                    extra=["--per-index-mismatches", "1,1", "--max-mismatches", "0", "--quality-metrics", "--index-pairs", "--top-unmatched", "5"])
    assert r.returncode == 0, r.stderr
    assert "--max-mismatches is ignored" in r.stderr
    rows = [line.split("\t") for line in open(out / "demux-metrics.txt").read().splitlines()[1:]]
    assert [int(row[2]) for row in rows] == [int(c) for c in counts]
    for s in range(len(barcodes)):
        assert [h.split()[0] for h, _, _ in H.read_fastq(out / f"Sample{s:04}.R1.fq.gz")] == [f"ex_{i}" for i in np.nonzero(idx == s)[0]]
    assert len(H.read_fastq(out / "unmatched.R1.fq.gz")) == counts[-1]


@pytest.mark.parametrize("rs,extra,sentence", [
    (["8B", "8B", "+T"], ["--quality-weighted", "60,30"], "invalid use of '--per-index-mismatches' with '--quality-weighted'"),
    (["8B", "8B", "+T"], ["--indel-rescue", "1,2"], "invalid use of '--per-index-mismatches' with '--indel-rescue'"),
    (["8B", "8B", "+T"], ["--host-output"], "the host routers match whole barcodes"),
    (["16B", "+T", "+T"], [], "exactly two sample-barcode (B) segments of fixed length"),
    (["8B", "+B", "+T"], [], "one of them of variable length"),
    (["8B", "8B", "+T"], ["--per-index-mismatches", "1"], "expected M1,M2")])
def test_cli_per_index_usage_errors(tmp_path, rs, extra, sentence):
    from tests import hostlib as H
    files = [H.fastq_file(tmp_path, k, "ex", ["ACGTACGTACGTACGT"] * 4) for k in ("i1", "i2", "r1")]
    r = H.run_demux(files, rs, H.metadata_file(tmp_path, ["ACGTACGTACGTACGT", "TTTTACGTACGTAAAA"]), tmp_path / "out",
                    extra=["--per-index-mismatches", "1,1"] + extra)
    assert r.returncode == 1 and sentence in r.stderr
