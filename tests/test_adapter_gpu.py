"""3' adapter read-through scan on the device (fqtk_demuxer_adapter_*, csrc/adapter_kernels.hip.h) against the rule of
include/fqtk_demux.h stated literally -- a loop over p and j on the very templates a case generates; exact integers."""
import os

import numpy as np
import pytest

from fqtk_amd import BarcodeMatcher, _lib
from fqtk_amd.demux import Demuxer, parse_read_structure
from oracle import oracle as O
from tests import hostlib as H
from tests.test_demuxer_gpu import BARCODES8, _bgzf_of, _span, make_templates
from tests.test_quality_gpu import ten_mers, texts_latin1

pytestmark = pytest.mark.gpu

TRUSEQ = ["AGATCGGAAGAGCACACGTCTGAACTCCAGTCA", "AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGT"]   # 33 bases each
A32 = "CTGTCTCTTATACACATCTCCGAGCCCACGAG"
A64 = (A32 + TRUSEQ[1])[:64]


def expected_adapters(barcodes, mm, delta, structures, templates, adapters, min_overlap, pct, short):
    segs = [parse_read_structure(r) for r in structures]
    S, L = len(barcodes), len(barcodes[0])
    min_len = [sum(l if l >= 0 else 1 for _, l, _ in ss) for ss in segs]
    kept = [t for t in templates if all(len(t[i][1]) >= min_len[i] for i in range(len(segs)))]
    bcs = ["".join(t[i][1][slice(*_span(s, len(t[i][1])))] for i, ss in enumerate(segs) for s in ss if s[2] == "B") for t in kept]
    obs = np.frombuffer("".join(b.ljust(L, "\0") for b in bcs).encode(), np.uint8).reshape(len(kept), L)
    idx = O.RefLiteral(barcodes, mm, delta, True).assign_batch(obs)[0]
    scanned = [i for i, ss in enumerate(segs) if any(s[2] == "T" for s in ss)]
    want = np.zeros((S + 1, 5 * len(scanned)), dtype=np.uint64)
    for t, b, i_s in zip(kept, bcs, idx):
        row = want[int(i_s) if len(b) == L and i_s != 0xFFFF else S]
        for j, i in enumerate(scanned):
            A = adapters[min(j, len(adapters) - 1)].upper().encode()
            R = t[i][1][slice(*_span([s for s in segs[i] if s[2] == "T"][-1], len(t[i][1])))].encode("latin-1")
            n, m = len(R), len(A)
            if n > 512:
                row[5 * j + 4] += 1
                continue
            row[5 * j] += 1
            for p in range(n):
                ov = min(m, n - p)
                mis = sum((R[p + k] & 0xDF) != A[k] for k in range(ov))
                if ov >= min_overlap and mis <= ov * pct // 100:
                    row[5 * j + 1:5 * j + 4] += np.array([1, n - p, p < short], dtype=np.uint64)
                    break
    return want


def mutated(a, k):
    """`a` with k of its bases replaced by another base, spread over its length."""
    a = list(a)
    for q in range(k):
        pos = q * len(a) // k
        a[pos] = "ACGT"[("ACGT".index(a[pos]) + 1) % 4]
    return "".join(a)


def placement_spans(rng, A, min_overlap, pct):
    """Spans for one +T input: 'N' never matches, so every hit is one that is planted here."""
    m, e = len(A), len(A) * pct // 100
    N = lambda k: "N" * k
    spans = []
    for n in list(range(1, m + 3)) + [31, 32, 33, 63, 64, 65, 95, 96, 97, 511, 512, 513]:   # random, and the adapter from the middle on
        r = "".join(rng.choice(list("ACGT"), n))
        spans += [r, (r[:n // 2] + A + r)[:n]]
    spans += [A + N(10), N(40) + A[:min_overlap], N(40) + A[:min_overlap - 1],           # p = 0, p = n - min_overlap, one behind it
              N(20) + mutated(A, e) + N(5), N(20) + mutated(A, e + 1) + N(5),             # the full length at its budget and one over
              N(3) + A + N(10) + A, N(20) + A + N(max(6, 50 - m)) + A,                     # two hits; in different 32-offset words
              N(70) + mutated(A, e + 1) + N(30) + A, N(500 - m) + A, (N(512 - min_overlap) + A)[:512]]
    part = max(ov for ov in range(min_overlap, m + 1) if ov * pct // 100 == max(e - 1, 0))   # a partial overlap with one mismatch less allowed
    spans += [N(20) + mutated(A[:part], ov_e) for ov_e in (max(e - 1, 0), max(e - 1, 0) + 1)]
    for byte in ("N", ".", "R", "\xc1", "\xe1"):                                             # one mismatch each, never a match
        spans += [N(7) + A[:m // 2] + byte + A[m // 2 + 1:] + N(3), N(7) + mutated(A, e)[:m - 1] + byte]
    spans.append(N(9) + A.lower() + N(4))
    return spans


def planted(rng, templates, structures, adapters, every=3):
    """The adapter from a random place of the scanned span on, in every third template; headers of 1..17 bytes."""
    segs = [parse_read_structure(r) for r in structures]
    scanned = [i for i, ss in enumerate(segs) if any(s[2] == "T" for s in ss)]
    for k, t in enumerate(templates):
        for j, i in enumerate(scanned):
            head, bases, quals = t[i]
            lo, hi = _span([s for s in segs[i] if s[2] == "T"][-1], len(bases))
            if k % every == 0 and hi > lo:
                p = int(rng.integers(lo, hi))
                tail = adapters[min(j, len(adapters) - 1)] + "".join(rng.choice(list("ACGT"), hi - lo))
                bases = bases[:p] + tail[:hi - p] + bases[hi:]
            t[i] = (head, bases, quals)
        for i in range(len(structures)):
            t[i] = ("h" * (1 + k % 17),) + t[i][1:]
    return templates


RULE = (5, 10, 30)
CASES = {   # structures, barcodes, adapters, (min_overlap, max_error_pct, short_insert), options
    "place_m5": (["8B+T"], BARCODES8, ["GATCG"], (3, 20, 2), {"place": True}),
    "place_m13_one_base": (["8B+T"], BARCODES8, ["A" * 13], RULE, {"place": True}),
    "place_m32": (["8B+T"], BARCODES8, [A32], RULE, {"place": True}),
    "place_m33": (["8B+T"], BARCODES8, TRUSEQ[:1], RULE, {"place": True}),
    "place_m64": (["8B+T"], BARCODES8, [A64], (8, 10, 40), {"place": True}),
    "8B20T": (["8B20T"], BARCODES8, TRUSEQ[:1], RULE, {"crlf": True}),
    "8B+T": (["8B+T"], BARCODES8, TRUSEQ[:1], RULE, {}),
    "two_T_two_B": (["+T", "+T", "4B", "4B"], BARCODES8, TRUSEQ, RULE, {"short_every": 7}),
    "every_kind": (["3M2S3B10T5C", "5B+T"], BARCODES8, ["GATCG", "A" * 13], (3, 20, 2), {"crlf": True, "short_every": 5}),
    "last_T": (["10T3M+T"], BARCODES8, TRUSEQ[:1], RULE, {}),
    "no_T": (["8B"], BARCODES8, TRUSEQ[:1], RULE, {}),
    "direct_to_hbm": (["10B+T"], ten_mers(_lib.FQTK_DEMUX_QUALITY_LDS_COUNTERS // 5 + 1), TRUSEQ[:1], RULE, {}),
    "fed_bgzf": (["8B", "+T", "6M+T"], BARCODES8, TRUSEQ, RULE, {"member": 700}),
    # one workgroup, 16 items a round: 4200 templates in one chunk are 263 rounds, past the flush of the LDS table after 255
    "flush_between_rounds": (["8B+T"], BARCODES8, ["A" * 13], RULE, {"n": 4200, "chunk": 4200, "grid": 1}),
}


@pytest.mark.parametrize("case", list(CASES))
def test_adapter_rows_equal_the_rule(case, monkeypatch):
    structures, barcodes, adapters, rule, opt = CASES[case]
    rng = np.random.default_rng(sorted(CASES).index(case))
    if opt.get("place"):
        spans = placement_spans(rng, adapters[0], rule[0], rule[1])
        templates = [[("h" * (1 + t % 17), (BARCODES8[t % 8] if t % 5 else "CATGCATG") + s, "I" * (8 + len(s)))] for t, s in enumerate(spans)]
    else:
        templates = planted(rng, make_templates(rng, opt.get("n", 700), barcodes, structures, header_kind=1, short_every=opt.get("short_every", 0)),
                            structures, adapters)
    n_in, chunk = len(structures), opt.get("chunk", 256)
    monkeypatch.setenv("FQTK_ADAPTER_GRID", str(opt.get("grid", 0)))
    m = BarcodeMatcher(barcodes, 1, 2, device=0)
    d = Demuxer(m, structures, "TB" if case != "last_T" else "T", skip_too_few_bases="short_every" in opt, max_chunk_templates=chunk)
    d.enable_adapters(adapters, *rule)
    want = expected_adapters(barcodes, 1, 2, structures, templates, adapters, *rule)
    assert (want.size > _lib.FQTK_DEMUX_QUALITY_LDS_COUNTERS) == (case == "direct_to_hbm")
    sizes = [min(chunk, len(templates) - lo) for lo in range(0, len(templates), chunk)]
    if "member" in opt:   # BGZF members of 700 bytes of text: windows with lead != 0 and first_line != 0
        monkeypatch.setenv("FQTK_FED_ARENA_MIN", "60000")
        for i, text in enumerate(texts_latin1(templates, 0, len(templates), n_in)):
            d.feed(i, _bgzf_of(text, opt["member"], rng), last=True)
        for k, n in enumerate(sizes):
            d.submit_fed(k % 3, n)
            d.collect_fed(k % 3)
        d.flush()
    else:
        d.run([(texts_latin1(templates, lo, lo + n, n_in, opt.get("crlf", False)), n) for lo, n in zip(range(0, len(templates), chunk), sizes)])
    got = d.adapters()
    assert got.dtype == np.uint64 and got.shape == want.shape and np.array_equal(got, want)
    for j in range(want.shape[1] // 5):
        assert np.array_equal(got[:, 5 * j] + got[:, 5 * j + 4], d.counts())
    if case != "no_T":
        assert want[:, 1].sum() > 0 and want[-1].sum() > 0   # (hits exist, and the unmatched row is in use)


def test_adapter_enable_says_which_parameter_is_out_of_range():
    m = BarcodeMatcher(BARCODES8, 1, 2, device=0)
    for args, word in [(([],), "n_adapters"), ((TRUSEQ,), "n_adapters"), ((["ACGNT"],), "plain ACGT"), ((["ACG"],), "length"), ((["A" * 65],), "length"),
                       ((["ACGTA"], 0), "min_overlap"), ((["ACGTA"], 6), "length"), ((TRUSEQ[:1], 5, 31), "max_error_pct"), (([A64], 5, 13), "7 mismatches")]:
        with pytest.raises(Exception, match=word):
            Demuxer(m, ["8B+T"], "T").enable_adapters(*args)
    d = Demuxer(m, ["8B+T"], "T", max_chunk_templates=8)
    with pytest.raises(Exception, match="not enabled"):
        d.adapters()
    d.run([(texts_latin1(make_templates(np.random.default_rng(0), 8, BARCODES8, ["8B+T"]), 0, 8, 1), 8)])
    with pytest.raises(Exception, match="before the first chunk"):
        d.enable_adapters(["acgta"])
    ok = Demuxer(m, ["8B+T", "+T"], "T")
    ok.enable_adapters(["acgta"], 5, 30, 0)   # lower case is taken; one adapter serves both inputs
    assert ok.adapters().shape == (9, 10)


def test_cli_adapter_metrics_one_and_two_devices_and_what_it_refuses(tmp_path):
    structures = ["8B+T", "+T"]
    rng = np.random.default_rng(5)
    templates = planted(rng, make_templates(rng, 300, BARCODES8, structures), structures, TRUSEQ)
    paths = []
    for i, text in enumerate(texts_latin1(templates, 0, len(templates), 2)):
        paths.append(tmp_path / f"in{i}.fq")
        paths[-1].write_bytes(text)
    meta = H.metadata_file(tmp_path, BARCODES8)
    want = expected_adapters(BARCODES8, 1, 2, structures, templates, TRUSEQ, 6, 10, 12)
    text = "sample_id\tbarcode\tread\tscanned\twith_adapter\tfrac_with_adapter\tadapter_bases\tshort_inserts\tfrac_short_inserts\ttoo_long\n"
    for s, (sid, bc) in enumerate([(f"Sample{k:04}", b) for k, b in enumerate(BARCODES8)] + [("unmatched", ".")]):
        for j in range(2):
            sc, wa, ab, si, tl = (int(x) for x in want[s, 5 * j:5 * j + 5])
            text += "\t".join([sid, bc, f"R{j + 1}", str(sc), str(wa), "%.4f" % (wa / sc if sc else 0), str(ab), str(si), "%.4f" % (si / sc if sc else 0), str(tl)]) + "\n"
    flags = ["--chunk-reads", "100", "--adapter-metrics", ",".join(TRUSEQ), "--adapter-rule", "6,10,12"]
    for name, more in (("plain", []), ("two", ["--devices", "0,0"])):
        r = H.run_demux(paths, structures, meta, tmp_path / name, extra=flags + more)
        assert r.returncode == 0, r.stderr
        assert (tmp_path / name / "adapter-metrics.txt").read_text() == text, name
    r = H.run_demux(paths, structures, meta, tmp_path / "host", extra=flags + ["--host-output"])
    assert r.returncode != 0 and "invalid use of '--adapter-metrics' with '--host-output'" in r.stderr
    r = H.run_demux(paths, structures, meta, tmp_path / "off", extra=["--chunk-reads", "100"])
    assert r.returncode == 0, r.stderr
    assert sorted(os.listdir(tmp_path / "off")) == sorted(f for f in os.listdir(tmp_path / "plain") if f != "adapter-metrics.txt")
    for f in os.listdir(tmp_path / "off"):
        assert (tmp_path / "off" / f).read_bytes() == (tmp_path / "plain" / f).read_bytes(), f
