// trim.hpp -- trim-metrics.txt (`fqtk demux --trim-adapters / --trim-quality`): what 3' quality and adapter trimming did per sample
// and trimmed read, one row per (sample, input that has a template segment).  The counters are those of include/fqtk_demux.h
// (fqtk_demuxer_trim): the device trims the records and tallies them (csrc/trim_kernels.hip.h); the host routers of --host-output hold
// no such step and the flags are refused there.  The file has no counterpart in the reference: its text is this project's own.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

namespace fqtk_host {

// [n_samples + 1][8 * trimmed inputs]: per trimmed input scanned, quality_trimmed, quality_bases, adapter_trimmed, adapter_bases,
// floored, kept_bases, too_long
struct TrimTable {
    size_t n_trimmed = 0, row_words = 0;
    std::vector<uint64_t> v;
    void init(size_t n_samples, size_t trimmed_inputs) {
        n_trimmed = trimmed_inputs;
        row_words = 8 * trimmed_inputs;
        v.assign((n_samples + 1) * row_words, 0);
    }
    const uint64_t *row(size_t s) const { return v.data() + s * row_words; }
};

// "MINOVERLAP,ERRPCT" -> the adapter rule of the trimming (the values' ranges are the library's to check)
inline bool parse_trim_rule(const std::string &v, unsigned long rule[2]) {
    const size_t q = v.find(',');
    if (q == std::string::npos || q == 0 || q + 1 == v.size()) return false;
    const std::string tok[2] = {v.substr(0, q), v.substr(q + 1)};
    for (int k = 0; k < 2; ++k) {
        char *end = nullptr;
        if (tok[k][0] < '0' || tok[k][0] > '9') return false;
        rule[k] = std::strtoul(tok[k].c_str(), &end, 10);
        if (*end != '\0' || rule[k] > 0xFFFFFFFFul) return false;
    }
    return true;
}

// ids / barcodes: n_samples + 1 of them, unmatched (barcode ".") last.  Reads are numbered R1, R2, .. over the trimmed inputs, as
// adapter-metrics.txt numbers them.
inline std::string trim_tsv(const TrimTable &t, const std::vector<std::string> &ids, const std::vector<std::string> &barcodes) {
    std::string out = "sample_id\tbarcode\tread\tscanned\tquality_trimmed\tfrac_quality_trimmed\tquality_bases\tadapter_trimmed\tfrac_adapter_trimmed\t"
                      "adapter_bases\tfloored\tkept_bases\ttoo_long\n";
    char buf[384];
    for (size_t s = 0; s < ids.size(); ++s)
        for (size_t j = 0; j < t.n_trimmed; ++j) {
            const uint64_t *c = t.row(s) + 8 * j;
            const double fq = c[0] ? (double)c[1] / (double)c[0] : 0.0, fa = c[0] ? (double)c[3] / (double)c[0] : 0.0;
            std::snprintf(buf, sizeof buf, "\tR%zu\t%llu\t%llu\t%.4f\t%llu\t%llu\t%.4f\t%llu\t%llu\t%llu\t%llu\n", j + 1, (unsigned long long)c[0], (unsigned long long)c[1], fq,
                          (unsigned long long)c[2], (unsigned long long)c[3], fa, (unsigned long long)c[4], (unsigned long long)c[5], (unsigned long long)c[6],
                          (unsigned long long)c[7]);
            out += ids[s] + "\t" + barcodes[s] + buf;
        }
    return out;
}

}  // namespace fqtk_host
