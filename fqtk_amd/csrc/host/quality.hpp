// quality.hpp -- demux-quality-metrics.txt (`fqtk demux --quality-metrics`): per-sample yield and quality, one row per
// (sample, input that has a template segment).  The counters are those of include/fqtk_demux.h (fqtk_demuxer_quality): the
// device tallies them (csrc/quality_kernels.hip.h); with --host-output the router threads, which walk every record anyway,
// tally the same sums with add_template below.  The file has no counterpart in the reference: its text is this project's own.
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "read_structure.hpp"

namespace fqtk_host {

// [n_samples + 1][3 + 4 * n_inputs]: templates, perfect_matches, one_mismatch_matches, then per input bases, q20_bases,
// q30_bases, qual_byte_sum
struct QualityTable {
    size_t n_inputs = 0, row_words = 0;
    std::vector<uint64_t> v;
    void init(size_t n_samples, size_t inputs) {
        n_inputs = inputs;
        row_words = 3 + 4 * inputs;
        v.assign((n_samples + 1) * row_words, 0);
    }
    uint64_t *row(size_t s) { return v.data() + s * row_words; }
    const uint64_t *row(size_t s) const { return v.data() + s * row_words; }
    void add(const QualityTable &o) { for (size_t k = 0; k < v.size(); ++k) v[k] += o.v[k]; }
};

// One template that is not dropped: `row` is its sample's, matched / best are the matcher's verdict, qual[i] / seq_len[i] the
// quality line of input i.
inline void add_template(uint64_t *row, bool matched, unsigned best, const std::vector<ReadStructure> &rs, const char *const *qual, const uint32_t *seq_len) {
    row[0] += 1;
    row[1] += matched && best == 0;
    row[2] += matched && best == 1;
    for (size_t i = 0; i < rs.size(); ++i) {
        uint64_t *c = row + 3 + 4 * i;
        for (const ReadSegment &seg : rs[i].segments) {
            if (seg.kind != SegType::Template) continue;
            size_t lo, hi;
            segment_span(seg, seq_len[i], &lo, &hi);
            const unsigned char *q = reinterpret_cast<const unsigned char *>(qual[i]);
            uint64_t q20 = 0, q30 = 0, sum = 0;
            for (size_t k = lo; k < hi; ++k) { q20 += q[k] >= 53; q30 += q[k] >= 63; sum += q[k]; }
            c[0] += hi - lo; c[1] += q20; c[2] += q30; c[3] += sum;
        }
    }
}

// ids / barcodes: n_samples + 1 of them, unmatched (barcode ".") last.  Reads are numbered R1, R2, .. over the inputs that
// have a template segment, as the T output files are by segment.
inline std::string quality_tsv(const QualityTable &t, const std::vector<ReadStructure> &rs, const std::vector<std::string> &ids, const std::vector<std::string> &barcodes) {
    std::string out = "sample_id\tbarcode\tread\ttemplates\tperfect_matches\tone_mismatch_matches\tbases\tq20_bases\tq30_bases\tfrac_q30\tmean_quality\n";
    char buf[256];
    for (size_t s = 0; s < ids.size(); ++s) {
        const uint64_t *r = t.row(s);
        size_t read = 0;
        for (size_t i = 0; i < rs.size(); ++i) {
            if (rs[i].count(SegType::Template) == 0) continue;
            const uint64_t *c = r + 3 + 4 * i;
            const double frac = c[0] ? (double)c[2] / (double)c[0] : 0.0, mean = c[0] ? (double)c[3] / (double)c[0] - 33.0 : 0.0;
            std::snprintf(buf, sizeof buf, "\tR%zu\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%.4f\t%.4f\n", ++read, (unsigned long long)r[0], (unsigned long long)r[1],
                          (unsigned long long)r[2], (unsigned long long)c[0], (unsigned long long)c[1], (unsigned long long)c[2], frac, mean);
            out += ids[s] + "\t" + barcodes[s] + buf;
        }
    }
    return out;
}

}  // namespace fqtk_host
