// quality_kernels.hip.h -- per-sample yield and quality tally of a chunk (include/fqtk_demux.h, fqtk_demuxer_quality_*;
// DESIGN.md section 5.1d): a reduction, keyed by sample, over the quality bytes that lie in the template (T) segments of every
// input's read structure.  Everything it reads is in HBM already: the inputs' text, the record views k_records wrote, the
// matcher's results, skip[].
//
// THE TALLY (exact integer arithmetic).  For a template t that is not dropped, s = its sample (None -> n_samples):
//   row s:  templates += 1, perfect += (matched with 0 mismatches), one_mismatch += (matched with 1)
//   row s, input i, over the bytes q of i's quality line inside a T segment's span (fmt::segment_span at qual_off, the span
//   k_format writes; a trailing '\r' is not part of seq_len):  bases += 1, q20 += (q >= 53), q30 += (q >= 63), sum += q
//   -- unsigned compares on the raw Phred+33 byte, no byte value is special.
// A row is 3 + 4 * n_inputs counters: [templates, perfect, one_mismatch, (bases, q20, q30, sum) per input].
//
// WORK SPLIT.  An ITEM is one (template, input that has a T segment) pair; a GROUP of 16 lanes -- one DPP row -- owns an item, a
// workgroup of 256 lanes is 16 groups, and the grid strides over the items in ROUNDS (every group of the grid one item per
// round, so a workgroup's groups all make the same number of rounds).  A quality line starts at an arbitrary byte; the group
// reads it as ALIGNED 16-byte loads, 256 bytes of line per pass, from the 16-byte boundary at or below the first T byte on.
// Per lane and pass a 16-bit mask says which of its bytes lie in a T span -- the OR of one range per T segment of the input,
// so several segments cost no further load, and the bytes before the line, behind it and between segments are masked off,
// not branched on; a lane whose mask is empty does not load.  Loads go through tile_bytes (demux_kernels.hip.h): nothing
// outside [lead, len) of the input's text is touched.  Per dword: the mask nibble is spread to a byte mask, q >= 53 and
// q >= 63 are SWAR compares (exact for bytes >= 0x80, as newline_mask is) + popcount, the byte sum is v_sad_u8 against 0.
// The four per-lane sums are reduced over the row with four DPP moves each, and lanes 0..6 of the group add one counter each.
//
// TWO LEVELS.  Level 2 is the demuxer's table of 64-bit counters in HBM, kept across chunks.  Level 1 is a table of 32-bit
// counters in the workgroup's LDS, indexed as level 2 is, used when (n_samples + 1) * row words <= kQualLdsCounters; it is
// flushed with 64-bit global atomics (non-zero counters only).  A larger table: the groups add to level 2 directly.
//
// NO LEVEL-1 COUNTER CAN WRAP.  A group adds to LDS only for a line of at most kQualLineBytes = 4096 bytes of passes (16
// passes; a longer line's sums go to level 2 directly, every 16 passes), a byte adds at most 255 to a counter, and the
// workgroup flushes and clears its table every kQualFlushRounds = 255 rounds: between two flushes a counter receives at most
// 255 rounds x 16 groups x 4096 bytes x 255 = 4 261 478 400 < 2^32.  (A chunk of 262 144 templates x 2 inputs on 256 CUs is 16
// rounds: one flush, at the end.)  A lane's own sums between two reductions cover 16 passes x 16 bytes x 255 < 2^17.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "demux_kernels.hip.h"

namespace fqtk {
namespace demux {

constexpr uint32_t kQualBlock = 256;                 // 16 groups of 16 lanes
constexpr uint32_t kQualGroups = kQualBlock / 16u;
constexpr uint32_t kQualLdsCounters = FQTK_DEMUX_QUALITY_LDS_COUNTERS;   // level 1: 32 KiB of LDS at most
constexpr uint32_t kQualPasses = 16;                 // passes between two reductions of a group
constexpr uint32_t kQualLineBytes = kQualPasses * 256u;
constexpr uint32_t kQualFlushRounds = 255;
constexpr uint32_t kQualMaxSegs = 32;                // T segments over all inputs
static_assert((uint64_t)kQualFlushRounds * kQualGroups * kQualLineBytes * 255u < (1ull << 32), "a level-1 counter cannot wrap between two flushes");

struct QualConfig {
    uint32_t n_inputs, n_samples, row_words;
    uint32_t n_qin;                               // inputs that have a T segment
    uint32_t items;                               // items per template: max(n_qin, 1) -- item 0 also counts the template
    uint8_t qin[FQTK_DEMUX_MAX_INPUTS];           // which inputs those are
    uint8_t seg0[FQTK_DEMUX_MAX_INPUTS + 1];      // T segments of qin[j]: tseg[seg0[j] .. seg0[j + 1])
    uint32_t t_off[kQualMaxSegs];
    int32_t t_len[kQualMaxSegs];
};

// 0x80 in every byte of x that is >= T (1 <= T <= 128), exact for every byte value: the low seven bits are compared by an add
// that cannot carry out of its byte, a byte with its top bit set is >= T anyway
template <uint32_t T>
__device__ __forceinline__ uint32_t bytes_ge(uint32_t x) {
    return (((x & 0x7F7F7F7Fu) + (0x80u - T) * 0x01010101u) | x) & 0x80808080u;
}
// bits 0..3 -> 0xFF in bytes 0..3
__device__ __forceinline__ uint32_t nibble_bytes(uint32_t n) { return ((n * 0x00204081u) & 0x01010101u) * 0xFFu; }

// sum over the 16 lanes of a DPP row, in every lane of it
__device__ __forceinline__ uint32_t row_sum(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, true);    // quad_perm [1,0,3,2]
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, true);    // quad_perm [2,3,0,1]
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, true);   // row_half_mirror
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, true);   // row_mirror
    return v;
}

// what a group knows of its item before it touches the line
struct QualItem { uint32_t live, s, best, seq_len, qual_off, j; };

__device__ __forceinline__ QualItem load_item(const TextSet &T, const QualConfig &Q, uint32_t n, const uint32_t *res, const uint8_t *skip, uint64_t w, uint64_t n_items) {
    QualItem it;
    it.live = 0; it.s = 0; it.best = 255; it.seq_len = 0; it.qual_off = 0; it.j = 0;
    if (w >= n_items) return it;
    const uint32_t t = (uint32_t)(w / Q.items);
    it.j = (uint32_t)(w - (uint64_t)t * Q.items);
    if (t >= n || skip[t]) return it;
    const uint32_t r = res[t], idx = r & 0xFFFFu;
    it.live = 1;
    it.s = idx == FQTK_NO_MATCH ? Q.n_samples : idx;
    it.best = idx == FQTK_NO_MATCH ? 255u : (r >> 16) & 0xFFu;
    if (Q.n_qin) {
        const RecView *rv = T.rec[Q.qin[it.j]] + t;
        it.seq_len = rv->seq_len;
        it.qual_off = rv->qual_off;
    }
    return it;
}

__global__ __launch_bounds__(kQualBlock) void k_quality(TextSet T, QualConfig Q, uint32_t n, const uint32_t *res, const uint8_t *skip,
                                                        unsigned long long *table, uint32_t n_counters, uint32_t use_lds, const ChunkStatus *st) {
    if (no_records(st)) return;
    extern __shared__ uint32_t q_lds[];   // level 1: n_counters words (use_lds)
    const uint32_t tid = threadIdx.x, lane = tid & 15u, group = tid >> 4;
    if (use_lds) {
        for (uint32_t c = tid; c < n_counters; c += kQualBlock) q_lds[c] = 0u;
        __syncthreads();
    }
    const uint64_t n_items = (uint64_t)n * Q.items, per_round = (uint64_t)gridDim.x * kQualGroups;
    const uint32_t rounds = (uint32_t)((n_items + per_round - 1) / per_round);
    uint64_t w = (uint64_t)blockIdx.x * kQualGroups + group;
    QualItem next = load_item(T, Q, n, res, skip, w, n_items);
    for (uint32_t round = 0; round < rounds; ++round) {
        const QualItem it = next;
        w += per_round;
        if (round + 1u < rounds) next = load_item(T, Q, n, res, skip, w, n_items);   // (the next item's views are on their way while this one's line is read)
        if (it.live) {
            // the T spans of this line, relative to its first byte
            uint32_t lo_min = 0xFFFFFFFFu, hi_max = 0;
            const uint32_t k0 = Q.n_qin ? Q.seg0[it.j] : 0u, k1 = Q.n_qin ? Q.seg0[it.j + 1u] : 0u;
            for (uint32_t k = k0; k < k1; ++k) {
                uint32_t lo, hi;
                fmt::segment_span(Q.t_off[k], Q.t_len[k], it.seq_len, &lo, &hi);
                if (hi > lo) { lo_min = lo < lo_min ? lo : lo_min; hi_max = hi > hi_max ? hi : hi_max; }
            }
            const uint32_t in = Q.n_qin ? Q.qin[it.j] : 0u;
            const uint8_t *text = T.text[in];
            const uint32_t len = T.len[in], lead = T.lead[in];
            // aligned start of the passes, and where they end (offsets in the text; an empty span makes no pass)
            const uint32_t a0 = hi_max ? (it.qual_off + lo_min) & ~15u : 0u;
            const uint32_t end = hi_max ? it.qual_off + hi_max : 0u;
            const bool direct = !use_lds || (end - a0) > kQualLineBytes;
            unsigned long long *row2 = table + (size_t)it.s * Q.row_words;
            uint32_t *row1 = q_lds + it.s * Q.row_words;
            const uint32_t col = 3u + 4u * in;
            bool head = it.j == 0u;   // the template's own three counters go with the item's first reduction
            uint32_t a = a0;
            do {
                uint32_t bases = 0, q20 = 0, q30 = 0, sum = 0;
                for (uint32_t p = 0; p < kQualPasses && a < end; ++p, a += 256u) {
                    const uint32_t off = a + lane * 16u;
                    const int32_t rel = (int32_t)(off - it.qual_off);   // of the lane's first byte in the line (negative in front of it)
                    uint32_t m16 = 0;
                    for (uint32_t k = k0; k < k1; ++k) {
                        uint32_t lo, hi;
                        fmt::segment_span(Q.t_off[k], Q.t_len[k], it.seq_len, &lo, &hi);
                        int32_t b0 = (int32_t)lo - rel, b1 = (int32_t)hi - rel;
                        b0 = b0 < 0 ? 0 : (b0 > 16 ? 16 : b0);
                        b1 = b1 < 0 ? 0 : (b1 > 16 ? 16 : b1);
                        m16 |= ((1u << b1) - 1u) & ~((1u << b0) - 1u);
                    }
                    uint4 v = make_uint4(0, 0, 0, 0);
                    if (m16) v = tile_bytes(text, len, off / kLineTile, (off % kLineTile) / 16u, lead);
                    const uint32_t d[4] = {v.x & nibble_bytes(m16 & 15u), v.y & nibble_bytes((m16 >> 4) & 15u), v.z & nibble_bytes((m16 >> 8) & 15u),
                                           v.w & nibble_bytes(m16 >> 12)};
                    bases += (uint32_t)__popc(m16);
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        q20 += (uint32_t)__popc(bytes_ge<53>(d[q]));
                        q30 += (uint32_t)__popc(bytes_ge<63>(d[q]));
                        sum = __builtin_amdgcn_sad_u8(d[q], 0u, sum);
                    }
                }
                bases = row_sum(bases);
                q20 = row_sum(q20);
                q30 = row_sum(q30);
                sum = row_sum(sum);
                // lane 0..3: the input's four counters; lane 4..6: the template's
                uint32_t add = lane == 0u ? bases : lane == 1u ? q20 : lane == 2u ? q30 : lane == 3u ? sum : 0u;
                uint32_t c = col + lane;
                if (head && lane >= 4u && lane < 7u) {
                    c = lane - 4u;
                    add = lane == 4u ? 1u : (lane == 5u ? (it.best == 0u ? 1u : 0u) : (it.best == 1u ? 1u : 0u));
                }
                head = false;
                if (add && lane < 7u) {
                    if (direct) atomicAdd(row2 + c, (unsigned long long)add);
                    else atomicAdd(row1 + c, add);
                }
            } while (a < end);
        }
        if (use_lds && (round + 1u) % kQualFlushRounds == 0u && round + 1u < rounds) {   // (uniform over the workgroup)
            __syncthreads();
            for (uint32_t c = tid; c < n_counters; c += kQualBlock) {
                const uint32_t v = q_lds[c];
                if (v) { atomicAdd(table + c, (unsigned long long)v); q_lds[c] = 0u; }
            }
            __syncthreads();
        }
    }
    if (use_lds) {
        __syncthreads();
        for (uint32_t c = tid; c < n_counters; c += kQualBlock) {
            const uint32_t v = q_lds[c];
            if (v) atomicAdd(table + c, (unsigned long long)v);
        }
    }
}

}  // namespace demux
}  // namespace fqtk
