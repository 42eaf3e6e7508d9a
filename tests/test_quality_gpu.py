"""Per-sample yield and quality metrics tallied on the device (fqtk_demuxer_quality_*, csrc/quality_kernels.hip.h) against a
few lines of numpy over the very templates a case generates -- the definition in include/fqtk_demux.h, exact integers."""
import numpy as np
import pytest

from fqtk_amd import BarcodeMatcher, _lib
from fqtk_amd.demux import Demuxer, parse_read_structure
from oracle import oracle as O
from tests import hostlib as H
from tests.test_demuxer_gpu import BARCODES8, _bgzf_of, _span, make_templates

pytestmark = pytest.mark.gpu

QUALS = [chr(c) for c in (33, 52, 53, 62, 63, 126, 127, 128, 255)]   # both sides of both thresholds, and high bytes


def expected_quality(barcodes, mm, delta, structures, templates):
    segs = [parse_read_structure(r) for r in structures]
    S, L = len(barcodes), len(barcodes[0])
    min_len = [sum(l if l >= 0 else 1 for _, l, _ in ss) for ss in segs]
    kept = [t for t in templates if all(len(t[i][1]) >= min_len[i] for i in range(len(segs)))]
    bcs = ["".join(t[i][1][slice(*_span(s, len(t[i][1])))] for i, ss in enumerate(segs) for s in ss if s[2] == "B") for t in kept]
    obs = np.frombuffer("".join(b.ljust(L, "\0") for b in bcs).encode(), np.uint8).reshape(len(kept), L)
    idx, best, _, _ = O.RefLiteral(barcodes, mm, delta, True).assign_batch(obs)
    want = np.zeros((S + 1, 3 + 4 * len(segs)), dtype=np.uint64)
    for t, b, i_s, bst in zip(kept, bcs, idx, best):
        hit = len(b) == L and i_s != 0xFFFF      # (a shorter barcode is unmatched)
        row = want[int(i_s) if hit else S]
        row[:3] += np.array([1, hit and bst == 0, hit and bst == 1], dtype=np.uint64)
        for i, ss in enumerate(segs):
            for s in (s for s in ss if s[2] == "T"):
                q = np.frombuffer(t[i][2][slice(*_span(s, len(t[i][1])))].encode("latin-1"), np.uint8).astype(np.uint64)
                row[3 + 4 * i:7 + 4 * i] += np.array([q.size, (q >= 53).sum(), (q >= 63).sum(), q.sum()], dtype=np.uint64)
    return want


def texts_latin1(templates, lo, hi, n_inputs, crlf=False):   # (texts_of encodes UTF-8: not for bytes >= 0x80)
    nl = "\r\n" if crlf else "\n"
    return [("".join(f"@{t[i][0]}{nl}{t[i][1]}{nl}+{nl}{t[i][2]}{nl}" for t in templates[lo:hi])).encode("latin-1") for i in range(n_inputs)]


def ten_mers(n):
    return ["".join("ACGT"[(k * 7919 % 4 ** 10) >> (2 * j) & 3] for j in range(10)) for k in range(n)]


def geometry_templates(rng):
    """One +T input: read lengths 1..40 and around one pass of 256 bytes, headers that put the quality lines at every offset mod 16."""
    out = []
    for t, rl in enumerate(list(range(1, 41)) * 16 + [255, 256, 257, 600] * 15):
        head = "h" * (1 + t % 17)
        out.append([(head, BARCODES8[t % 8], "I" * 8), (head, "".join(rng.choice(list("ACGT"), rl)), "".join(rng.choice(QUALS, rl)))])
    return out


CASES = {   # structures, barcodes, max_mismatches, options
    "8B20T": (["8B20T"], BARCODES8, 1, {}),
    "8B+T": (["8B+T"], BARCODES8, 1, {}),
    "two_T_two_B": (["+T", "+T", "4B", "4B"], BARCODES8, 1, {}),
    "every_kind": (["3M2S3B10T5C", "5B+T"], BARCODES8, 1, {}),
    "no_T": (["8B"], BARCODES8, 1, {}),
    "geometry": (["8B", "+T"], BARCODES8, 1, {"geometry": True}),
    "crlf_skip": (["8B12T", "6T"], BARCODES8, 1, {"crlf": True, "short_every": 5}),
    "direct_to_hbm": (["10B+T"], ten_mers(_lib.FQTK_DEMUX_QUALITY_LDS_COUNTERS // 7 + 1), 1, {}),
    "fed_bgzf": (["8B", "+T", "6M+T"], BARCODES8, 1, {"member": 700}),
    "best_0_1_2": (["8B+T"], BARCODES8, 2, {"mutate": True}),
    # one workgroup, 16 items a round: 4200 templates in one chunk are 263 rounds, past the flush of the LDS table after 255
    "flush_between_rounds": (["8B+T"], BARCODES8, 1, {"n": 4200, "chunk": 4200, "grid": 1}),
}


@pytest.mark.parametrize("case", list(CASES))
def test_quality_rows_equal_the_definition(case, monkeypatch):
    structures, barcodes, mm, opt = CASES[case]
    rng = np.random.default_rng(sorted(CASES).index(case))
    if opt.get("geometry"):
        templates = geometry_templates(rng)
    else:
        templates = make_templates(rng, opt.get("n", 700), barcodes, structures, header_kind=1, short_every=opt.get("short_every", 0))
        for k, t in enumerate(templates):
            if opt.get("mutate") and k % 3 == 0:      # a second mismatch on top of make_templates' own
                t[0] = (t[0][0], "CGTAA"["ACGTN".index(t[0][1][0])] + t[0][1][1:], t[0][2])
            for i in range(len(structures)):
                t[i] = (t[i][0], t[i][1], "".join(rng.choice(QUALS, len(t[i][1]))))
    n_in, chunk = len(structures), opt.get("chunk", 256)
    monkeypatch.setenv("FQTK_QUALITY_GRID", str(opt.get("grid", 0)))
    m = BarcodeMatcher(barcodes, mm, 2, device=0)
    d = Demuxer(m, structures, "TB", skip_too_few_bases="short_every" in opt, max_chunk_templates=chunk)
    assert ((m.n_samples + 1) * (3 + 4 * n_in) > _lib.FQTK_DEMUX_QUALITY_LDS_COUNTERS) == (case == "direct_to_hbm")
    d.enable_quality()
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
    want = expected_quality(barcodes, mm, 2, structures, templates)
    got = d.quality()
    assert got.dtype == np.uint64 and np.array_equal(got, want)
    assert np.array_equal(got[:, 0], d.counts())
    if opt.get("mutate"):
        matched = want[:-1]
        assert matched[:, 1].sum() > 0 and matched[:, 2].sum() > 0 and matched[:, 0].sum() > (matched[:, 1] + matched[:, 2]).sum()
    late = Demuxer(m, structures, "TB", skip_too_few_bases=True, max_chunk_templates=8)
    late.run([(texts_latin1(templates, 0, 8, n_in), 8)])
    with pytest.raises(Exception, match="before the first chunk"):
        late.enable_quality()


def test_cli_quality_metrics_device_host_and_two_devices(tmp_path, monkeypatch):
    structures = ["8B+T", "+T"]
    rng = np.random.default_rng(11)
    templates = make_templates(rng, 300, BARCODES8, structures)
    paths = []
    for i, text in enumerate(texts_latin1(templates, 0, len(templates), 2)):
        paths.append(tmp_path / f"in{i}.fq")
        paths[-1].write_bytes(text)
    meta = H.metadata_file(tmp_path, BARCODES8)
    want = expected_quality(BARCODES8, 1, 2, structures, templates)
    text = "sample_id\tbarcode\tread\ttemplates\tperfect_matches\tone_mismatch_matches\tbases\tq20_bases\tq30_bases\tfrac_q30\tmean_quality\n"
    for s, (sid, bc) in enumerate([(f"Sample{k:04}", b) for k, b in enumerate(BARCODES8)] + [("unmatched", ".")]):
        for i in range(2):
            b, q20, q30, qs = (int(x) for x in want[s, 3 + 4 * i:7 + 4 * i])
            text += "\t".join([sid, bc, f"R{i + 1}"] + [str(int(x)) for x in want[s, :3]] + [str(b), str(q20), str(q30),
                              "%.4f" % (q30 / b if b else 0), "%.4f" % (qs / b - 33 if b else 0)]) + "\n"
    for name, env, more in (("plain", None, []), ("host", "1", []), ("two", None, ["--devices", "0,0"])):
        monkeypatch.setenv("FQTK_HOST_OUTPUT", env) if env else monkeypatch.delenv("FQTK_HOST_OUTPUT", raising=False)
        r = H.run_demux(paths, structures, meta, tmp_path / name, extra=["--chunk-reads", "100", "--quality-metrics"] + more)
        assert r.returncode == 0, r.stderr
        assert (tmp_path / name / "demux-quality-metrics.txt").read_text() == text, name
    r = H.run_demux(paths, structures, meta, tmp_path / "off", extra=["--chunk-reads", "100"])
    assert r.returncode == 0 and not (tmp_path / "off" / "demux-quality-metrics.txt").exists()
