// adapters.hpp -- adapter-metrics.txt (`fqtk demux --adapter-metrics`): 3' adapter read-through per sample and scanned read, one
// row per (sample, input that has a template segment).  The counters are those of include/fqtk_demux.h (fqtk_demuxer_adapter):
// the device tallies them (csrc/adapter_kernels.hip.h) from text that is in HBM anyway; the host routers of --host-output have no
// such text and the flag is refused there.  The file has no counterpart in the reference: its text is this project's own.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "read_structure.hpp"

namespace fqtk_host {

// [n_samples + 1][5 * scanned inputs]: per scanned input scanned, with_adapter, adapter_bases, short_inserts, too_long
struct AdapterTable {
    size_t n_scanned = 0, row_words = 0;
    std::vector<uint64_t> v;
    void init(size_t n_samples, size_t scanned_inputs) {
        n_scanned = scanned_inputs;
        row_words = 5 * scanned_inputs;
        v.assign((n_samples + 1) * row_words, 0);
    }
    const uint64_t *row(size_t s) const { return v.data() + s * row_words; }
};

inline size_t scanned_inputs(const std::vector<ReadStructure> &rs) {
    size_t n = 0;
    for (const ReadStructure &r : rs) n += r.count(SegType::Template) != 0;
    return n;
}

// "SEQ1[,SEQ2..]" -> the adapters; "MINOVERLAP,ERRPCT,SHORT" -> the rule.  false: not of that form (the values' ranges are the
// library's to check: fqtk_demuxer_adapter_enable says which parameter).
inline bool parse_adapter_list(const std::string &v, std::vector<std::string> *out) {
    size_t p = 0;
    while (p <= v.size()) {
        const size_t q = v.find(',', p);
        const std::string tok = v.substr(p, q == std::string::npos ? std::string::npos : q - p);
        if (tok.empty()) return false;
        out->push_back(tok);
        if (q == std::string::npos) break;
        p = q + 1;
    }
    return !out->empty();
}
inline bool parse_adapter_rule(const std::string &v, unsigned long rule[3]) {
    size_t p = 0;
    for (int k = 0; k < 3; ++k) {
        const size_t q = k < 2 ? v.find(',', p) : v.size();
        if (q == std::string::npos || q == p) return false;
        char *end = nullptr;
        const std::string tok = v.substr(p, q - p);
        if (tok[0] < '0' || tok[0] > '9') return false;
        rule[k] = std::strtoul(tok.c_str(), &end, 10);
        if (*end != '\0' || rule[k] > 0xFFFFFFFFul) return false;
        p = q + 1;
    }
    return true;
}

// ids / barcodes: n_samples + 1 of them, unmatched (barcode ".") last.  Reads are numbered R1, R2, .. over the scanned inputs, as
// demux-quality-metrics.txt numbers them.
inline std::string adapter_tsv(const AdapterTable &t, const std::vector<std::string> &ids, const std::vector<std::string> &barcodes) {
    std::string out = "sample_id\tbarcode\tread\tscanned\twith_adapter\tfrac_with_adapter\tadapter_bases\tshort_inserts\tfrac_short_inserts\ttoo_long\n";
    char buf[256];
    for (size_t s = 0; s < ids.size(); ++s)
        for (size_t j = 0; j < t.n_scanned; ++j) {
            const uint64_t *c = t.row(s) + 5 * j;
            const double with = c[0] ? (double)c[1] / (double)c[0] : 0.0, shrt = c[0] ? (double)c[3] / (double)c[0] : 0.0;
            std::snprintf(buf, sizeof buf, "\tR%zu\t%llu\t%llu\t%.4f\t%llu\t%llu\t%.4f\t%llu\n", j + 1, (unsigned long long)c[0], (unsigned long long)c[1], with,
                          (unsigned long long)c[2], (unsigned long long)c[3], shrt, (unsigned long long)c[4]);
            out += ids[s] + "\t" + barcodes[s] + buf;
        }
    return out;
}

}  // namespace fqtk_host
