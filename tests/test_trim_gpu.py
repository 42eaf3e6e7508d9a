"""3' quality and adapter trimming on the device (fqtk_demuxer_trim_*, csrc/trim_kernels.hip.h) against the rule of
include/fqtk_demux.h stated literally -- loops over i, p and j on the very templates a case generates; the files are
expected_files on the trimmed templates, byte for byte, and the counters are exact integers."""
import gzip
import os

import numpy as np
import pytest

from fqtk_amd import BarcodeMatcher, _lib
from fqtk_amd.demux import BGZF_EOF, Demuxer, parse_read_structure
from oracle import oracle as O
from tests import hostlib as H
from tests.test_adapter_gpu import A64, TRUSEQ, expected_adapters, planted
from tests.test_demuxer_gpu import BARCODES8, _bgzf_of, _span, expected_files, make_templates
from tests.test_quality_gpu import expected_quality, ten_mers, texts_latin1

pytestmark = pytest.mark.gpu

HI, LO = "\x7f", "!"   # above every cutoff + 33 (at most 126); Phred 0


def rule(R, Q, A, min_overlap, pct, cutoff, min_length):
    n = n_q = len(R)
    s = best = 0
    for i in range(n - 1, -1, -1) if cutoff else ():
        s += cutoff + 33 - Q[i]
        if s < 0:
            break
        if s > best:
            best, n_q = s, i
    cut = n_q
    for p in range(n_q) if A else ():
        ov = min(len(A), n_q - p)
        if ov >= min_overlap and sum((R[p + j] & 0xDF) != A[j] for j in range(ov)) <= ov * pct // 100:
            cut = p
            break
    return n_q, cut, max(cut, min(min_length, n))


def expected_trim(barcodes, structures, templates, adapters, min_overlap, pct, cutoff, min_length):
    """(the templates as they are written, the counter table)"""
    segs = [parse_read_structure(r) for r in structures]
    S, L = len(barcodes), len(barcodes[0])
    min_len = [sum(l if l >= 0 else 1 for _, l, _ in ss) for ss in segs]
    live = [k for k, t in enumerate(templates) if all(len(t[i][1]) >= min_len[i] for i in range(len(segs)))]
    bcs = ["".join(templates[k][i][1][slice(*_span(s, len(templates[k][i][1])))] for i, ss in enumerate(segs) for s in ss if s[2] == "B") for k in live]
    obs = np.frombuffer("".join(b.ljust(L, "\0") for b in bcs).encode(), np.uint8).reshape(len(live), L)
    idx = O.RefLiteral(barcodes, 1, 2, True).assign_batch(obs)[0]
    tin = [i for i, ss in enumerate(segs) if any(s[2] == "T" for s in ss)]
    want, out = np.zeros((S + 1, 8 * len(tin)), dtype=np.uint64), [list(t) for t in templates]
    for k, b, i_s in zip(live, bcs, idx):
        row = want[int(i_s) if len(b) == L and i_s != 0xFFFF else S]
        for j, i in enumerate(tin):
            head, bases, quals = templates[k][i]
            lo, hi = _span([s for s in segs[i] if s[2] == "T"][-1], len(bases))
            if hi - lo > 512:
                row[8 * j + 7] += 1
                continue
            A = adapters[min(j, len(adapters) - 1)].upper().encode() if adapters else b""
            n_q, cut, kept = rule(bases[lo:hi].encode("latin-1"), quals[lo:hi].encode("latin-1"), A, min_overlap, pct, cutoff, min_length)
            row[8 * j:8 * j + 7] += np.array([1, n_q < hi - lo, hi - lo - n_q, cut < n_q, n_q - cut, kept > cut, kept], dtype=np.uint64)
            out[k][i] = (head, bases[:lo + kept], quals[:lo + kept]) if kept != hi - lo else templates[k][i]
    return out, want


def run_and_check(monkeypatch, structures, barcodes, templates, trim_args, opt={}, types="T"):
    """The templates through a trimming demuxer: files and counters against the rule; returns (demuxer, trimmed templates, table)."""
    n_in, chunk = len(structures), opt.get("chunk", 256)
    monkeypatch.setenv("FQTK_TRIM_GRID", str(opt.get("grid", 0)))
    d = Demuxer(BarcodeMatcher(barcodes, 1, 2, device=0), structures, types, skip_too_few_bases="short_every" in opt, max_chunk_templates=chunk)
    d.enable_trim(*trim_args)
    for name, args in opt.get("also", []):
        getattr(d, name)(*args)
    sizes = [min(chunk, len(templates) - lo) for lo in range(0, len(templates), chunk)]
    if "member" in opt:   # BGZF members of 700 bytes of text: windows with lead != 0 and first_line != 0
        monkeypatch.setenv("FQTK_FED_ARENA_MIN", "60000")
        files = [bytearray() for _ in range(d.n_files)]
        for i, text in enumerate(texts_latin1(templates, 0, len(templates), n_in)):
            d.feed(i, _bgzf_of(text, opt["member"], np.random.default_rng(i)), last=True)
        for k, n in enumerate(sizes):
            d.submit_fed(k % 3, n)
            for c, x in enumerate(d.collect_fed(k % 3)[0]):
                files[c] += x
        files = [bytes(f + x) + BGZF_EOF for f, x in zip(files, d.flush())]
    else:
        files = d.run([(texts_latin1(templates, lo, lo + n, n_in, opt.get("crlf", False)), n) for lo, n in zip(range(0, len(templates), chunk), sizes)])
    trimmed, want = expected_trim(barcodes, structures, templates, *trim_args)
    for c, w in enumerate(expected_files(barcodes, 1, 2, structures, types, trimmed, "short_every" in opt)[0]):
        assert gzip.decompress(files[c]) == w.decode().encode("latin-1"), f"file column {c}"   # (expected_files encodes UTF-8)
    got = d.trim()
    assert got.dtype == np.uint64 and got.shape == want.shape and np.array_equal(got, want)
    for j in range(want.shape[1] // 8):
        assert np.array_equal(got[:, 8 * j] + got[:, 8 * j + 7], d.counts())
    assert want[-1].sum() > 0 and (not trim_args[3] or want[:, 1::8].sum() > 0) and (not trim_args[0] or want[:, 3::8].sum() > 0)   # (no case is empty)
    return d, trimmed, want


def one_input(spans):   # 8B+T, three of every (bases, quals), headers of 1..17 bytes, every fifth template unmatched
    return [[("h" * (1 + t % 17), (BARCODES8[t % 8] if t % 5 else "CATGCATG") + r, "I" * 8 + q)] for t, (r, q) in enumerate(spans * 3)]


@pytest.mark.parametrize("min_length", [1, 20])
@pytest.mark.parametrize("cutoff", [2, 20, 40, 93])
def test_quality_cut_at_every_length_alignment_and_lane_boundary(cutoff, min_length, monkeypatch):
    rng, c33, lines = np.random.default_rng(cutoff), cutoff + 33, []
    for n in list(range(1, 36)) + [63, 64, 65, 95, 96, 97, 511, 512, 513]:
        lines += [HI * n, LO * n, "".join("\x00 \x7f\xff"[k] for k in rng.integers(0, 4, n))]
        lines += [HI * (n - 3) + chr(c33 - 1) + chr(c33 + 1) + chr(c33 - 1)] * (n >= 3)   # s = 1, 0, 1: the right one of the two maxima is n_q
        lines += [HI * (n - 16) + LO * 5 + "\xff" * 8 + LO * 3] * (n >= 16)                # s < 0 inside the \xff run: the low bytes left of it stay
    lines += [HI * (n - k) + LO * k for k in range(1, 41) for n in (64, 97, 512)]           # cuts across the lanes' 32-byte boundaries
    templates = one_input([("".join(rng.choice(list("ACGT"), len(q))), q) for q in lines])
    want = run_and_check(monkeypatch, ["8B+T"], BARCODES8, templates, ((), 5, 10, cutoff, min_length), {"chunk": len(templates)})[2]
    assert want[:, 5].sum() > 0 and want[:, 7].sum() > 0   # floored (the all-low lines), too long (513)


@pytest.mark.parametrize("case, adapters, min_overlap, pct, cutoff, min_length", [
    ("m5", ["GATCG"], 3, 20, 20, 1), ("m33", TRUSEQ[:1], 5, 10, 20, 1), ("m33_floor", TRUSEQ[:1], 5, 10, 20, 25), ("m64_floor", [A64], 8, 10, 20, 25),
    ("adapter_only", TRUSEQ[:1], 5, 10, 0, 1), ("quality_only", (), 5, 10, 20, 1)])
def test_adapter_cut_behind_the_quality_cut(case, adapters, min_overlap, pct, cutoff, min_length, monkeypatch):
    A, mo, N = (adapters or TRUSEQ)[0], min_overlap, lambda k: "N" * k   # ('N' never matches: every hit is one planted here)
    m = len(A)
    spans = [(N(40) + A + N(5), HI * 40 + LO * (m + 5)),                # the adapter lies in the quality-trimmed tail: no hit
             (N(40) + A + N(3), HI * (40 + mo) + LO * (m + 3 - mo)),    # it straddles n_q and min_overlap bases survive: a hit at 40
             (N(40) + A + N(3), HI * (39 + mo) + LO * (m + 4 - mo)),    # one base less survives: no hit
             (N(30) + A + N(10), HI * (32 + m) + LO * 8),               # in front of a low tail: both counters move
             (A + N(10), HI * (m + 10))]                                # p = 0: the floor decides
    want = run_and_check(monkeypatch, ["8B+T"], BARCODES8, one_input(spans), (adapters, mo, pct, cutoff, min_length))[2]
    assert not adapters or want[:, 5].sum() > 0


CASES = {   # structures, barcodes, output types, options
    "two_T_two_B": (["+T", "+T", "4B", "4B"], BARCODES8, "TB", {"short_every": 7, "crlf": True}),
    "last_T": (["10T3M+T"], BARCODES8, "T", {}),
    "fed_bgzf": (["8B", "+T", "6M+T"], BARCODES8, "TBM", {"member": 700}),
    "direct_to_hbm": (["10B+T"], ten_mers(_lib.FQTK_DEMUX_QUALITY_LDS_COUNTERS // 8 + 1), "T", {}),
    # one workgroup, 16 items a round: 4200 templates in one chunk are 263 rounds, past the flush of the LDS table after 255
    "flush_between_rounds": (["8B+T"], BARCODES8, "T", {"n": 4200, "chunk": 4200, "grid": 1}),
    "with_both_reports": (["8B+T", "+T"], BARCODES8, "T", {"also": [("enable_adapters", (TRUSEQ, 5, 10, 30)), ("enable_quality", ())]}),
}


@pytest.mark.parametrize("case", list(CASES))
def test_trimmed_files_and_counters_through_the_pipeline(case, monkeypatch):
    structures, barcodes, types, opt = CASES[case]
    rng = np.random.default_rng(sorted(CASES).index(case))
    templates = planted(rng, make_templates(rng, opt.get("n", 700), barcodes, structures, header_kind=1, short_every=opt.get("short_every", 0)), structures, TRUSEQ)
    for k, t in enumerate(templates):   # a '#' (Phred 2) tail of 0..11 bytes on every other template; make_templates' own lines end in '#' now and then
        for i in range(len(structures)):
            tail = min(int(rng.integers(0, 12)) * (k % 2), len(t[i][2]))
            t[i] = (t[i][0], t[i][1], t[i][2][:len(t[i][2]) - tail] + "#" * tail)
    adapters = TRUSEQ[:sum("T" in r for r in structures)]   # (at most one adapter per trimmed input)
    d, trimmed, want = run_and_check(monkeypatch, structures, barcodes, templates, (adapters, 5, 10, 20, 3), opt, types)
    assert (want.size > _lib.FQTK_DEMUX_QUALITY_LDS_COUNTERS) == (case == "direct_to_hbm")
    if "also" in opt:   # the adapter metrics see the reads as they came in, the quality tally the bytes the files got
        assert np.array_equal(d.adapters(), expected_adapters(barcodes, 1, 2, structures, templates, TRUSEQ, 5, 10, 30))
        assert np.array_equal(d.quality(), expected_quality(barcodes, 1, 2, structures, trimmed))


def test_trim_enable_says_which_parameter_is_out_of_range():
    m = BarcodeMatcher(BARCODES8, 1, 2, device=0)
    for structures, types, kw, word in [(["100T8B"], "T", {"quality_cutoff": 20}, "input 0"), (["8B"], "B", {"quality_cutoff": 20}, "no read structure"),
                                        (["8B+T"], "T", {"quality_cutoff": 94}, "quality_cutoff"), (["8B+T"], "T", {"quality_cutoff": 20, "min_length": 0}, "min_length"),
                                        (["8B+T"], "T", {}, "n_adapters is 0 and quality_cutoff is 0"), (["8B+T"], "T", {"adapters": ["ACGNT"]}, "plain ACGT")]:
        with pytest.raises(Exception, match=word):
            Demuxer(m, structures, types).enable_trim(**kw)
    d = Demuxer(m, ["8B+T"], "T", max_chunk_templates=8)
    with pytest.raises(Exception, match="not enabled"):
        d.trim()
    d.run([(texts_latin1(make_templates(np.random.default_rng(0), 8, BARCODES8, ["8B+T"]), 0, 8, 1), 8)])
    with pytest.raises(Exception, match="before the first chunk"):
        d.enable_trim(quality_cutoff=20)
    ok = Demuxer(m, ["8B+T", "10T3M+T"], "T")
    ok.enable_trim(["acgta"], quality_cutoff=93)   # lower case is taken; one adapter serves both inputs
    with pytest.raises(Exception, match="enabled once"):
        ok.enable_trim(quality_cutoff=20)
    assert ok.trim().shape == (9, 16)


def test_cli_trims_on_one_and_two_devices_and_what_it_refuses(tmp_path):
    structures = ["8B+T", "+T"]
    rng = np.random.default_rng(5)
    templates = planted(rng, make_templates(rng, 300, BARCODES8, structures), structures, TRUSEQ)
    templates = [[(h, b, q[:len(q) - len(q) // 3 * (k % 2)] + "#" * (len(q) // 3 * (k % 2))) for h, b, q in t] for k, t in enumerate(templates)]
    paths = []
    for i, text in enumerate(texts_latin1(templates, 0, len(templates), 2)):
        paths.append(tmp_path / f"in{i}.fq")
        paths[-1].write_bytes(text)
    meta = H.metadata_file(tmp_path, BARCODES8)
    trimmed, want = expected_trim(BARCODES8, structures, templates, TRUSEQ, 6, 10, 20, 12)
    assert want[:, 1].sum() > 0 and want[:, 3].sum() > 0 and want[:, 5].sum() > 0 and want[-1].sum() > 0
    files = expected_files(BARCODES8, 1, 2, structures, "T", trimmed)[0]
    names = [f"Sample{k:04}" for k in range(8)] + ["unmatched"]
    text = "sample_id\tbarcode\tread\tscanned\tquality_trimmed\tfrac_quality_trimmed\tquality_bases\tadapter_trimmed\tfrac_adapter_trimmed\tadapter_bases\tfloored\tkept_bases\ttoo_long\n"
    for s, (sid, bc) in enumerate(zip(names, BARCODES8 + ["."])):
        for j in range(2):
            c = [int(x) for x in want[s, 8 * j:8 * j + 8]]
            text += "\t".join([sid, bc, f"R{j + 1}", str(c[0]), str(c[1]), "%.4f" % (c[1] / c[0] if c[0] else 0), str(c[2]), str(c[3]), "%.4f" % (c[3] / c[0] if c[0] else 0)] +
                              [str(x) for x in c[4:]]) + "\n"
    flags = ["--chunk-reads", "100", "--trim-adapters", ",".join(TRUSEQ), "--trim-quality", "20", "--trim-rule", "6,10", "--trim-min-length", "12"]
    for name, more in (("plain", []), ("two", ["--devices", "0,0"])):
        r = H.run_demux(paths, structures, meta, tmp_path / name, extra=flags + more)
        assert r.returncode == 0, r.stderr
        assert (tmp_path / name / "trim-metrics.txt").read_text() == text, name
        for s, sid in enumerate(names):
            for j in range(2):
                assert gzip.decompress((tmp_path / name / f"{sid}.R{j + 1}.fq.gz").read_bytes()) == files[2 * s + j], (name, sid, j)
    r = H.run_demux(paths, structures, meta, tmp_path / "host", extra=flags + ["--host-output"])
    assert r.returncode != 0 and "invalid use of '--trim-adapters' with '--host-output'" in r.stderr
    # no flag: the files of a run whose trimming finds nothing (no quality byte of these inputs is below Phred 1)
    for name, more in (("off", []), ("nothing", ["--trim-quality", "1"])):
        r = H.run_demux(paths, structures, meta, tmp_path / name, extra=["--chunk-reads", "100"] + more)
        assert r.returncode == 0, r.stderr
    assert sorted(os.listdir(tmp_path / "off")) == sorted(f for f in os.listdir(tmp_path / "nothing") if f != "trim-metrics.txt")
    for f in os.listdir(tmp_path / "off"):
        assert (tmp_path / "off" / f).read_bytes() == (tmp_path / "nothing" / f).read_bytes(), f
