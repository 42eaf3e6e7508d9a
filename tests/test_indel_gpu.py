"""The indel rescue (fqtk::indel_rescue_kernel, fqtk_matcher_indel_*, `fqtk demux --indel-rescue`) against the rule of include/fqtk_match.h in two
stages: oracle.RefLiteral for the matcher's own rule, then the sequence-Levenshtein DP in numpy, int64, for the reads it leaves None.  All exact."""
import functools

import numpy as np
import pytest

from fqtk_amd import BarcodeMatcher
from oracle import oracle as O
from tests.test_mfma_scan_gpu import DT, make_reads, make_table
from tests.test_weighted_gpu import words

pytestmark = pytest.mark.gpu

NONE = 0xFFFF
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def seqlev(r, s):
    """r [n, L], s [S, L] enc() codes -> [n, S] min over the last row and the last column of the edit-distance matrix."""
    (n, L), S = r.shape, len(s)
    row = [np.full((n, S), j, dtype=np.int64) for j in range(L + 1)]
    last_col = [row[L]]
    for i in range(1, L + 1):
        new = [np.full((n, S), i, dtype=np.int64)]
        for j in range(1, L + 1):
            mis = (r[:, None, i - 1] & ~s[None, :, j - 1] & 15) != 0
            new.append(np.minimum(np.minimum(row[j - 1] + mis, row[j] + 1), new[j - 1] + 1))
        row = new
        last_col.append(row[L])
    return np.minimum(np.min(row, axis=0), np.min(last_col, axis=0))


def with_edits(rng, obs, L, rows):
    """The given rows get one or two edits: a base deleted and the row refilled at its end, or one inserted and the row cut to L."""
    obs = obs.copy()
    for i in rows:
        row = obs[i, :L].tolist()
        for _ in range(int(rng.integers(1, 3))):
            p = int(rng.integers(0, L))
            if rng.random() < 0.5:
                del row[p]
                row.append(int(rng.choice(ACGT)))
            else:
                row.insert(p, int(rng.choice(ACGT)))
                row.pop()
        obs[i, :L] = row
    return obs


def first_stage(barcodes, mm, delta, obs, lens=None):
    """The matcher's own result as int64 arrays, the rows the rescue examines, and their distances to every sample."""
    L = len(barcodes[0])
    idx, best, nxt, counts = [a.astype(np.int64) for a in O.RefLiteral(barcodes, mm, delta, False).assign_batch(obs if lens is not None else obs[:, :L], lens)]
    none = idx == NONE
    rows = np.nonzero(none & (obs.shape[1] >= L) & (True if lens is None else lens == L))[0]
    tab = np.frombuffer("".join(barcodes).encode("latin-1"), dtype=np.uint8).reshape(len(barcodes), L)
    dist = seqlev(O.ENC[obs[rows, :L]], O.ENC[tab]) if len(rows) else np.zeros((0, len(barcodes)), dtype=np.int64)
    return (idx, best, nxt, counts), rows, dist, int(none.sum()) - len(rows)


def second_stage(first, rows, dist, max_edits, med):
    """(idx, best, next, counts, rescued[S + 1]) after the rescue; `rescued` as the bool per examined row comes last."""
    idx, best, nxt, counts = [a.copy() for a in first]
    S, sat = dist.shape[1], max_edits + max(med, 1)                   # (a delta of 0 saturates one above max_edits: no decision moves)
    d = np.minimum(dist, sat)
    srt = np.sort(d, axis=1)
    b, s = srt[:, 0], d.argmin(1)                                    # the lowest index on ties
    n2 = srt[:, 1] if S > 1 else np.full(len(rows), sat)
    ok = (b <= max_edits) & (n2 - b >= med)
    idx[rows[ok]], best[rows[ok]], nxt[rows[ok]] = s[ok], 0x80 | b[ok], n2[ok]
    rescued = np.bincount(np.where(ok, s, S), minlength=S + 1)
    counts += np.append(rescued[:S], -int(ok.sum()))                 # + at s, the sum - at S
    return idx, best, nxt, counts, rescued, ok


def check(m, want, got, skipped):
    (out, cnt), (idx, best, nxt, counts, rescued) = got, want[:5]
    assert np.array_equal(out["idx"], idx) and np.array_equal(out["best"], best) and np.array_equal(out["next"], nxt)
    assert cnt is None or np.array_equal(cnt.astype(np.int64), counts)
    got_rescued, got_skipped = m.indel_rescued()
    assert got_rescued.dtype == np.uint64 and np.array_equal(got_rescued.astype(np.int64), rescued) and got_skipped == skipped


@functools.lru_cache(maxsize=None)
def structure_case(S, L, n, kind):
    """(barcodes, mm, delta, max_edits, obs): `words` = the first S L-letter words (every neighbour is a sample: mm 0), reads from all of them; `exact` = rows of
    an A/C/G/T table; `edited` = make_reads, a third of the rows edited; `dense` = exact but 600 edited rows in tile 0 and 100 in tile 512 (256 CUs: the same workgroup)."""
    rng = np.random.default_rng(1000 * S + L)
    by_words = kind == "words" or L == 1
    barcodes = words(S, L) if by_words else make_table(rng, S, L, 0.1 if kind == "edited" else 0.0)
    mm, delta = (0, 1) if by_words else (1, 2)
    tab = np.frombuffer("".join(barcodes).encode(), dtype=np.uint8).reshape(S, L)
    if kind == "words":
        obs = np.frombuffer("".join(words(4 ** L, L)).encode(), dtype=np.uint8).reshape(-1, L)[rng.integers(4 ** L, size=n)]
    elif kind == "edited":
        obs = with_edits(rng, make_reads(rng, barcodes, n), L, np.nonzero(rng.random(n) < 0.33)[0])
    else:
        obs = tab[rng.integers(S, size=n)]
        if kind == "dense":
            obs = with_edits(rng, obs, L, np.concatenate([rng.choice(2048, 600, replace=False), 512 * 2048 + rng.choice(2048, 100, replace=False)]))
    return barcodes, mm, delta, min(L - 1, 1 if L < 16 else 2), np.ascontiguousarray(obs)


# L: the top bit of the word (1, 32), the carry (17, 31), each instantiation's last column (8, 16, 32); S: next = sat (1), a sample group and
# one over (4, 5), 8192 bins in LDS and one more.  lo <= examined <= hi: none; under 64 (only the last partial drain); over 2200 (several
# chunks a wave); two tiles of one workgroup with 600 and 100 edited rows (a full drain, the remainder carried, the last round)
@pytest.mark.parametrize("S,L,n,kind,lo,hi", [
    (5, 8, 200, "exact", 0, 0), (4, 1, 300, "edited", 1, 63), (1, 8, 150, "edited", 1, 63), (4, 16, 70, "edited", 1, 63),
    (5, 17, 100, "edited", 1, 63), (5, 8, 9000, "edited", 2200, 9000), (4, 31, 9000, "edited", 2200, 9000), (5, 32, 9000, "edited", 2200, 9000),
    (5, 16, 513 * 2048 + 77, "dense", 600, 700), (8191, 8, 400, "words", 60, 400), (8192, 8, 400, "words", 60, 400)])
def test_structure_edges(S, L, n, kind, lo, hi):
    barcodes, mm, delta, max_edits, obs = structure_case(S, L, n, kind)
    first, rows, dist, skipped = first_stage(barcodes, mm, delta, obs)
    srt = np.sort(dist, axis=1)                                      # min_edit_delta = the median of next - best over the examined reads
    med = max(int(np.median(srt[:, 1] - srt[:, 0])) if S > 1 and len(rows) else 1, 1 - max_edits)
    want = second_stage(first, rows, dist, max_edits, med)
    assert lo <= len(rows) <= hi and (len(rows) < 60 or (want[5].any() and not want[5].all()))
    m = BarcodeMatcher(barcodes, mm, delta, use_cache=False)
    m.enable_indel_rescue(max_edits, med)
    check(m, want, m.assign_batch(obs), skipped)


@pytest.mark.parametrize("iupac", [0.0, 0.5])
def test_every_byte_value_at_every_position(iupac):
    L, rng = 16, np.random.default_rng(11)
    barcodes = make_table(rng, 5, L, iupac)
    tab = np.frombuffer("".join(barcodes).encode(), dtype=np.uint8).reshape(5, L)
    obs = tab[np.arange(L * 256) % 5].copy()
    obs[~np.isin(obs, ACGT)] = ord("C")
    obs[:, 1:L - 1] = obs[:, 2:]                                     # base 1 deleted: the first stage leaves these None
    obs[np.arange(L * 256), np.repeat(np.arange(L), 256)] = np.tile(np.arange(256, dtype=np.uint8), L)
    first, rows, dist, skipped = first_stage(barcodes, 1, 2, obs)
    want = second_stage(first, rows, dist, 1, 2)
    assert len(rows) > (L * 256) // 2 and want[5].any() and not want[5].all()
    m = BarcodeMatcher(barcodes, 1, 2)
    m.enable_indel_rescue(1, 2)
    check(m, want, m.assign_batch(obs), skipped)


@pytest.mark.parametrize("use_cache", [True, False])
def test_load_paths(use_cache):
    """stride > L with garbage in the pad bytes; the same rows at an unaligned device base; obs_len with None reads shorter than L."""
    import torch
    L, n, off, rng = 13, 3000, 3, np.random.default_rng(13)
    barcodes = make_table(rng, 40, L)
    obs = rng.integers(0, 256, size=(n, L + 6), dtype=np.uint8)
    obs[:, :L] = with_edits(rng, make_reads(rng, barcodes, n), L, np.arange(0, n, 3))
    m = BarcodeMatcher(barcodes, 1, 2, use_cache=use_cache)
    m.enable_indel_rescue(1, 2)
    first, rows, dist, skipped = first_stage(barcodes, 1, 2, obs)
    want = second_stage(first, rows, dist, 1, 2)
    assert want[5].any() and not want[5].all() and skipped == 0
    check(m, want, m.assign_batch(obs), 0)
    dev = torch.device("cuda:0")
    d_obs = torch.zeros(off + obs.size + 16, dtype=torch.uint8, device=dev)
    d_obs[off:off + obs.size] = torch.from_numpy(obs.reshape(-1)).to(dev)
    d_out = torch.empty(n, dtype=torch.int32, device=dev)
    d_counts = torch.zeros(len(barcodes) + 1, dtype=torch.int64, device=dev)
    m.reset_indel_rescue()
    m.assign_batch_device(d_obs.data_ptr() + off, obs.shape[1], n, d_out.data_ptr(), d_counts=d_counts.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    check(m, want, (d_out.cpu().numpy().view(DT), d_counts.cpu().numpy()), 0)
    lens = np.where(np.arange(n) % 5 == 0, L - 2, L).astype(np.uint32)
    first, rows, dist, skipped = first_stage(barcodes, 1, 2, obs, lens)
    assert skipped == n // 5 and (first[0][::5] == NONE).all()
    m.reset_indel_rescue()
    check(m, second_stage(first, rows, dist, 1, 2), m.assign_batch(obs, lens), skipped)


def test_composition_and_off_means_off():
    """Census and pair tally count the reads that remain None; after disable the batch is the plain one and the counters stay."""
    barcodes, mm, delta, max_edits, obs = structure_case(4, 16, 120, "edited")
    obs = np.tile(obs, (20, 1))
    first, rows, dist, skipped = first_stage(barcodes, mm, delta, obs)
    want = second_stage(first, rows, dist, 2, 2)
    remain = int((want[0] == NONE).sum())
    assert 0 < remain < int((first[0] == NONE).sum())
    m = BarcodeMatcher(barcodes, mm, delta)
    with pytest.raises(ValueError, match="not enabled"):
        m.indel_rescued()
    m.enable_indel_rescue(2, 2)
    m.enable_census()
    m.enable_pairs(8)
    check(m, want, m.assign_batch(obs), skipped)
    t, (mat, pair_skipped) = m.census_totals(), m.pairs()
    assert t.keyed + t.unkeyed + t.overflow == remain == int(mat.sum()) + pair_skipped
    for switch_off in (m.disable_census, m.disable_pairs, m.disable_indel_rescue):
        switch_off()
    out, cnt = m.assign_batch(obs)
    assert np.array_equal(out["idx"], first[0]) and np.array_equal(out["best"], first[1]) and np.array_equal(cnt.astype(np.int64), first[3])
    assert np.array_equal(m.indel_rescued()[0].astype(np.int64), want[4])


@pytest.mark.parametrize("L,max_edits,med,bound", [(33, 1, 2, "at most 32 bases"), (16, 9, 8, "<= 16"), (16, 0, 0, "1 <="), (16, 16, 0, "max_edits < 16")])
def test_refusals_leave_the_matcher_usable(L, max_edits, med, bound):
    rng = np.random.default_rng(L)
    barcodes = make_table(rng, 20, L)
    m = BarcodeMatcher(barcodes, 2, 1, use_cache=False)
    obs = make_reads(rng, barcodes, 100)
    before, before_counts = m.assign_batch(obs)
    with pytest.raises(ValueError, match=bound):
        m.enable_indel_rescue(max_edits, med)
    after, after_counts = m.assign_batch(obs)
    assert np.array_equal(before, after) and np.array_equal(before_counts, after_counts)


@pytest.mark.parametrize("extra", [[], ["--devices", "0,0", "--chunk-reads", "1000"]], ids=["one device", "two matchers"])
def test_cli_indel_rescue(tmp_path, extra):
    from tests import hostlib as H
    rng = np.random.default_rng(24)
    barcodes = make_table(rng, 24, 16, 0.0)
    tab = np.frombuffer("".join(barcodes).encode(), dtype=np.uint8).reshape(24, 16)
    obs = with_edits(rng, tab[rng.integers(24, size=3000)], 16, np.arange(0, 3000, 4))
    first, rows, dist, _ = first_stage(barcodes, 1, 2, obs)
    idx, _, _, counts, rescued, ok = second_stage(first, rows, dist, 1, 2)
    assert ok.any() and not ok.all()
    reads = [r.tobytes().decode() for r in obs]
    files = [H.fastq_file(tmp_path, k, "ex", v) for k, v in (("i1", [r[:8] for r in reads]), ("i2", [r[8:] for r in reads]), ("r1", ["ACGTACGT"] * 3000))]
    out = tmp_path / "out"
    r = H.run_demux(files, ["8B", "8B", "+T"], H.metadata_file(tmp_path, barcodes), out, extra=extra + ["--indel-rescue", "1,2"])
    assert r.returncode == 0, r.stderr
    names = [f"Sample{s:04}" for s in range(24)] + ["unmatched"]
    for s, name in enumerate(names):
        want = [f"ex_{i} 1:N:0:{reads[i][:8]}+{reads[i][8:]}" for i in np.nonzero(idx == (s if s < 24 else NONE))[0]]
        assert [rec[0] for rec in H.read_fastq(out / f"{name}.R1.fq.gz")] == want
    assert [int(line.split("\t")[2]) for line in open(out / "demux-metrics.txt").read().splitlines()[1:]] == counts.tolist()
    lines = [line.split("\t") for line in open(out / "indel-rescue.txt").read().splitlines()]
    assert lines[0] == ["sample_id", "barcode", "rescued_templates"] and [f[0] for f in lines[1:]] == names + ["skipped"]
    assert [int(f[2]) for f in lines[1:]] == rescued.tolist() + [0]


@pytest.mark.parametrize("args,structures,sentence", [
    (["--indel-rescue", "1,2", "--quality-weighted", "60,20"], ["8B", "8B", "+T"], "invalid use of '--indel-rescue' with '--quality-weighted'"),
    (["--indel-rescue", "1,2"], ["8B", "+B", "+T"], "a sample-barcode segment of variable length ('+B') is not taken"),
    (["--indel-rescue", "1,2"], ["20B", "20B", "+T"], "sample barcodes of at most 32 bases"),
    (["--indel-rescue", "1"], ["8B", "8B", "+T"], "expected MAXEDITS,DELTA")])
def test_cli_usage_errors(tmp_path, args, structures, sentence):
    from tests import hostlib as H
    meta = H.metadata_file(tmp_path, [c * (40 if structures[0] == "20B" else 16) for c in "AC"])
    r = H.run_demux([tmp_path / "absent1.fq", tmp_path / "absent2.fq", tmp_path / "absent3.fq"], structures, meta, tmp_path / "out", extra=args)
    assert r.returncode != 0 and sentence in r.stderr and "doesn't exist" not in r.stderr
