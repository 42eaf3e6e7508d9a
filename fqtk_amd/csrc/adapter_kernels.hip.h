// adapter_kernels.hip.h -- 3' adapter read-through scan of a chunk's template reads (include/fqtk_demux.h, fqtk_demuxer_adapter_*;
// DESIGN.md section 5.1i): per (sample, scanned input) how many reads run into the adapter, how many bases that costs, how many
// inserts are shorter than `short_insert`.  Everything it reads is in HBM already: the inputs' text, the record views k_records
// wrote, the matcher's results, skip[].
//
// THE RULE (exact integers).  A SCANNED INPUT is an input whose read structure has a T segment; the j-th one uses adapter
// A_min(j, k-1) (upper-case ACGT, m bases, min_overlap <= m <= 64) and its scanned span is its LAST T segment's
// (fmt::segment_span on seq_len: the bytes k_format writes; a trailing '\r' is not part of them).  For a template that is not
// dropped, s = its sample (None -> n_samples), R[0..n) the span's sequence bytes:
//   n > 512: too_long += 1, the read is not scanned.  Otherwise scanned += 1, and for an offset p in [0, n)
//     ov = min(m, n - p),  mis(p) = #{ j < ov : (R[p+j] & 0xDF) != A[j] }   (N, '.', IUPAC codes, junk never match; lower case does)
//     p is a HIT iff ov >= min_overlap and mis(p) <= floor(ov * max_error_pct / 100)
//   the trim position is the SMALLEST hit p; if there is one: with_adapter += 1, adapter_bases += n - p, short_inserts += (p < short_insert).
// A row is 5 counters per scanned input: [scanned, with_adapter, adapter_bases, short_inserts, too_long].
//
// WORK SPLIT.  An ITEM is one (template, scanned input) pair; a GROUP of 16 lanes -- one DPP row -- owns an item, a workgroup of
// 256 lanes is 16 groups, the grid strides over the items in ROUNDS (as k_quality does).  Items are numbered input-major over the
// templates padded to a multiple of 4, so the four groups of a wavefront always scan the same input: the adapter is
// WAVE-UNIFORM, its masks and thresholds live in SGPRs and the loops over its bases are scalar loops.
//
// LOAD AND ENCODE.  The span starts at an arbitrary byte; the group reads it as ALIGNED 16-byte loads through tile_bytes (nothing
// outside [lead, len) of the text is touched), 256 bytes a pass, at most 3 passes (512 bases + 15 bytes in front of them).  Per
// pass a lane turns its 16 bytes into four 16-bit one-hot fragments (is-A, is-C, is-G, is-T: a SWAR zero-byte test of
// (byte & 0xDF) ^ base, exact for every byte value as newline_mask is, the four 0x80 flags of a dword gathered into a nibble by one
// multiply) and stores them as halfwords into the group's slice of LDS -- four bit-planes of 24 dwords in ALIGNED coordinates
// (384 B an item, 6 KiB a workgroup).  No two lanes write one halfword, so there is no atomic and no shuffle; the shift to
// "bit 0 is R[0]" is a funnel shift on the way back: lane w reads dwords w..w+3 of a plane and three v_alignbit_b32 by
// (start & 15) give words w, w+1, w+2 of the plane in READ coordinates, ANDed with the words of V = bits [0, n): bits at and
// beyond n are zero.  12 VGPRs of planes + 3 of V cover every shift j <= 63 of the lane's 32 offsets.
//
// SCAN, bit-parallel over offsets.  Lane w owns offsets 32w .. 32w+31.  For each base b the adapter is a 64-bit mask of the
// positions j with A[j] == b; the loop runs over b and over the set bits j of the mask (scalar find-first-set).  Per step ONE
// funnel shift of plane b gives the 32 bits "R[p+j] == A[j]", one of V gives "p + j < n", and V_j & ~eq is added into a
// BIT-SLICED SATURATING COUNTER (3 planes + a sticky overflow plane; carry-save: 7 logic ops for 32 offsets).  The low and the
// high 32 positions of a mask are two loops, so which two words a shift takes is decided by the code, not by a select.
// No per-offset loop and no per-base select exists.
//
// DECISION.  allowed(ov) = floor(ov * pct / 100) does not decrease with ov and ov does not increase with p, so for every
// threshold t in 0..e_max the host precomputes ov_t = the smallest ov >= min_overlap with allowed(ov) >= t, and
//   hit = OR_t ( count == t  &  p <= n - ov_t )
// -- (count == t) from the sliced counter, the range as a mask of the lane's 32 offsets.  e_max <= 7 is what the enable call
// checks, so an overflowed counter is never a hit.  The smallest hit is the DPP row minimum of 32w + ctz(hit).
//
// TALLY.  Lanes 0..4 of the group add one counter each.  Two levels as in quality_kernels.hip.h: 32-bit counters in the
// workgroup's LDS when (n_samples + 1) * row words <= kQualLdsCounters, flushed (non-zero counters only) with 64-bit global
// atomics every kAdapterFlushRounds rounds and at the end; a larger table goes to HBM directly.
// NO LEVEL-1 COUNTER CAN WRAP: an item adds at most kAdapterMaxSpan = 512 to a counter (adapter_bases = n - p <= n), so between
// two flushes a counter receives at most 255 rounds x 16 groups x 512 = 2 088 960 < 2^32.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "demux_kernels.hip.h"
#include "quality_kernels.hip.h"

namespace fqtk {
namespace demux {

constexpr uint32_t kAdapterBlock = 256;               // 16 groups of 16 lanes
constexpr uint32_t kAdapterGroups = kAdapterBlock / 16u;
constexpr uint32_t kAdapterMaxSpan = 512;             // bases of a scanned span; a longer one is counted too_long
constexpr uint32_t kAdapterMaxLen = 64;               // bases of an adapter
constexpr uint32_t kAdapterMaxErrors = 7;             // floor(m * pct / 100): the sliced counter holds 0..7 and "more"
constexpr uint32_t kAdapterRowWords = 5;              // counters per scanned input
constexpr uint32_t kAdapterPasses = 3;                // 256-byte passes over a span: 512 bases + 15 bytes of misalignment
constexpr uint32_t kAdapterPlaneWords = kAdapterPasses * 8u;          // a bit-plane in aligned coordinates: 16 bits a lane and pass
constexpr uint32_t kAdapterGroupWords = 4u * kAdapterPlaneWords;      // LDS words of a group
constexpr uint32_t kAdapterFlushRounds = 255;
static_assert(kAdapterMaxSpan + 15u <= kAdapterPasses * 256u, "three passes cover the longest span wherever it starts");
static_assert(kAdapterMaxSpan == 16u * 32u, "a lane owns 32 offsets, a group 512");
static_assert(15u + 3u < kAdapterPlaneWords, "lane 15 reads dwords 15..18 of a plane");
static_assert((uint64_t)kAdapterFlushRounds * kAdapterGroups * kAdapterMaxSpan < (1ull << 32), "a level-1 counter cannot wrap between two flushes");

struct AdapterConfig {
    uint32_t n_samples, row_words;                // row_words = 5 * n_ain
    uint32_t n_ain;                               // scanned inputs
    uint32_t short_insert;
    uint8_t ain[FQTK_DEMUX_MAX_INPUTS];           // which inputs those are
    uint32_t t_off[FQTK_DEMUX_MAX_INPUTS];        // their last T segment
    int32_t t_len[FQTK_DEMUX_MAX_INPUTS];
    uint32_t base_lo[FQTK_DEMUX_MAX_INPUTS][4];   // positions 0..31 / 32..63 of the adapter that hold A, C, G, T
    uint32_t base_hi[FQTK_DEMUX_MAX_INPUTS][4];
    uint8_t e_max[FQTK_DEMUX_MAX_INPUTS];         // floor(m * pct / 100)
    uint8_t ov[FQTK_DEMUX_MAX_INPUTS][kAdapterMaxErrors + 1u];   // ov_t: the smallest overlap that allows t mismatches (t <= e_max)
};

// 0x80 in every byte of x that is zero (exact for every byte value: no carry leaves a byte)
__device__ __forceinline__ uint32_t zero_bytes(uint32_t x) { return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu); }
// bits 7, 15, 23, 31 -> bits 0..3 (the partial products land on distinct bits: nothing carries)
__device__ __forceinline__ uint32_t flags_nibble(uint32_t f) { return (((f >> 7) * 0x00204081u) >> 21) & 15u; }
// which of the 16 bytes of v are base `c` (upper case) in either case: bit k = byte k
__device__ __forceinline__ uint32_t base_fragment(const uint4 &v, uint32_t c) {
    const uint32_t k = c * 0x01010101u;
    return flags_nibble(zero_bytes((v.x & 0xDFDFDFDFu) ^ k)) | (flags_nibble(zero_bytes((v.y & 0xDFDFDFDFu) ^ k)) << 4) |
           (flags_nibble(zero_bytes((v.z & 0xDFDFDFDFu) ^ k)) << 8) | (flags_nibble(zero_bytes((v.w & 0xDFDFDFDFu) ^ k)) << 12);
}
// bits [0, lim) of a word, lim any integer
__device__ __forceinline__ uint32_t low_bits(int32_t lim) { return lim <= 0 ? 0u : (lim >= 32 ? 0xFFFFFFFFu : (1u << lim) - 1u); }

// minimum over the 16 lanes of a DPP row, in every lane of it
__device__ __forceinline__ uint32_t row_min(uint32_t v) {
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, 0xB1, 0xF, 0xF, false));    // quad_perm [1,0,3,2]
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, 0x4E, 0xF, 0xF, false));    // quad_perm [2,3,0,1]
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, 0x141, 0xF, 0xF, false));   // row_half_mirror
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, 0x140, 0xF, 0xF, false));   // row_mirror
    return v;
}

// the sliced counter of a lane's 32 offsets: c0..c2 the count's bits, ovf = "8 or more" (sticky)
struct SlicedCount { uint32_t c0, c1, c2, ovf; };
__device__ __forceinline__ void sliced_add(SlicedCount &c, uint32_t x) {
    uint32_t t = c.c0 & x;
    c.c0 ^= x;
    x = t;
    t = c.c1 & x;
    c.c1 ^= x;
    x = t;
    t = c.c2 & x;
    c.c2 ^= x;
    c.ovf |= t;
}

struct AdapterItem { uint32_t live, s, start, n; };   // start: offset of R[0] in the input's text

// items are input-major over the templates padded to a multiple of 4: item w is template w % n_pad of scanned input w / n_pad
__device__ __forceinline__ AdapterItem adapter_item(const TextSet &T, const AdapterConfig &A, uint32_t n, uint32_t n_pad, uint32_t j, const uint32_t *res,
                                                    const uint8_t *skip, uint32_t w, uint32_t n_items) {
    AdapterItem it;
    it.live = 0; it.s = 0; it.start = 0; it.n = 0;
    if (w >= n_items) return it;
    const uint32_t t = w - j * n_pad;
    if (t >= n || skip[t]) return it;
    const uint32_t idx = res[t] & 0xFFFFu;
    const RecView *rv = T.rec[A.ain[j]] + t;
    uint32_t lo, hi;
    fmt::segment_span(A.t_off[j], A.t_len[j], rv->seq_len, &lo, &hi);
    it.live = 1;
    it.s = idx == FQTK_NO_MATCH ? A.n_samples : idx;
    it.start = rv->seq_off + lo;
    it.n = hi - lo;
    return it;
}

// The scan of one item by its group of 16 lanes (k_adapter; k_trim of trim_kernels.hip.h on a span that ends at its quality cut): the smallest hit
// p of R[0..n_span), R[0] at byte `start` of scanned input j's text, 1 <= n_span <= kAdapterMaxSpan, in every lane of the group; 0xFFFFFFFF: no hit.
// `planes`: the group's kAdapterGroupWords of LDS.  j is wave-uniform.
__device__ __forceinline__ uint32_t adapter_scan(const TextSet &T, const AdapterConfig &A, uint32_t j, uint32_t *planes, uint32_t lane, uint32_t start, uint32_t n_span) {
    const uint32_t in = A.ain[j];
    const uint8_t *text = T.text[in];
    const uint32_t len = T.len[in], lead = T.lead[in];
    const uint32_t a0 = start & ~15u, sh = start & 15u, end = start + n_span;
    // ---- load and encode: halfword (pass * 16 + lane) of every plane, aligned coordinates
    __builtin_amdgcn_wave_barrier();   // (the round before has read its planes)
    typedef uint16_t __attribute__((may_alias)) half_t;   // (halfword stores into planes that are read back as dwords)
    half_t *half = reinterpret_cast<half_t *>(planes);
#pragma unroll
    for (uint32_t p = 0; p < kAdapterPasses; ++p) {
        if (a0 + p * 256u >= end) break;   // (the group as one; what an earlier item left in the halfwords of such a pass lies at and beyond n: V masks it)
        const uint32_t off = a0 + p * 256u + lane * 16u;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (off < end) v = tile_bytes(text, len, off / kLineTile, (off % kLineTile) / 16u, lead);
        const uint32_t h = p * 16u + lane;
        half[0u * 2u * kAdapterPlaneWords + h] = (uint16_t)base_fragment(v, 'A');
        half[1u * 2u * kAdapterPlaneWords + h] = (uint16_t)base_fragment(v, 'C');
        half[2u * 2u * kAdapterPlaneWords + h] = (uint16_t)base_fragment(v, 'G');
        half[3u * 2u * kAdapterPlaneWords + h] = (uint16_t)base_fragment(v, 'T');
    }
    __threadfence_block();
    __builtin_amdgcn_wave_barrier();
    // ---- words lane, lane + 1, lane + 2 of V and of the planes, read coordinates (bit 0 = R[0])
    uint32_t V[3], P[4][3];
#pragma unroll
    for (uint32_t k = 0; k < 3u; ++k) V[k] = low_bits((int32_t)n_span - (int32_t)(32u * (lane + k)));
#pragma unroll
    for (uint32_t b = 0; b < 4u; ++b) {
        const uint32_t *pl = planes + b * kAdapterPlaneWords + lane;
        const uint32_t d0 = pl[0], d1 = pl[1], d2 = pl[2], d3 = pl[3];
        P[b][0] = __builtin_amdgcn_alignbit(d1, d0, sh) & V[0];
        P[b][1] = __builtin_amdgcn_alignbit(d2, d1, sh) & V[1];
        P[b][2] = __builtin_amdgcn_alignbit(d3, d2, sh) & V[2];
    }
    // ---- scan: one step per base of the adapter, 32 offsets a lane
    SlicedCount cnt;
    cnt.c0 = cnt.c1 = cnt.c2 = cnt.ovf = 0u;
#pragma unroll
    for (uint32_t b = 0; b < 4u; ++b) {
        uint32_t mlo = (uint32_t)__builtin_amdgcn_readfirstlane((int)A.base_lo[j][b]);
        while (mlo) {   // shifts 0..31: words lane, lane + 1
            const uint32_t q = (uint32_t)__builtin_ctz(mlo);
            mlo &= mlo - 1u;
            const uint32_t eq = __builtin_amdgcn_alignbit(P[b][1], P[b][0], q);
            sliced_add(cnt, __builtin_amdgcn_alignbit(V[1], V[0], q) & ~eq);
        }
        uint32_t mhi = (uint32_t)__builtin_amdgcn_readfirstlane((int)A.base_hi[j][b]);
        while (mhi) {   // shifts 32..63: words lane + 1, lane + 2
            const uint32_t q = (uint32_t)__builtin_ctz(mhi);
            mhi &= mhi - 1u;
            const uint32_t eq = __builtin_amdgcn_alignbit(P[b][2], P[b][1], q);
            sliced_add(cnt, __builtin_amdgcn_alignbit(V[2], V[1], q) & ~eq);
        }
    }
    // ---- decision: OR over t of (count == t) & (p <= n - ov_t)
    const uint32_t e_max = (uint32_t)__builtin_amdgcn_readfirstlane((int)A.e_max[j]);
    uint32_t hit = 0;
    for (uint32_t t = 0; t <= e_max; ++t) {
        const uint32_t is_t = ~cnt.ovf & ((t & 1u) ? cnt.c0 : ~cnt.c0) & ((t & 2u) ? cnt.c1 : ~cnt.c1) & ((t & 4u) ? cnt.c2 : ~cnt.c2);
        hit |= is_t & low_bits((int32_t)n_span - (int32_t)A.ov[j][t] + 1 - (int32_t)(32u * lane));
    }
    return row_min(hit ? 32u * lane + (uint32_t)__builtin_ctz(hit) : 0xFFFFFFFFu);
}

__global__ __launch_bounds__(kAdapterBlock) void k_adapter(TextSet T, AdapterConfig A, uint32_t n, const uint32_t *res, const uint8_t *skip,
                                                           unsigned long long *table, uint32_t n_counters, uint32_t use_lds, const ChunkStatus *st) {
    if (no_records(st)) return;
    extern __shared__ uint32_t a_lds[];   // the groups' bit-planes, then level 1: n_counters words (use_lds)
    uint32_t *tally = a_lds + kAdapterGroups * kAdapterGroupWords;
    const uint32_t tid = threadIdx.x, lane = tid & 15u, group = tid >> 4;
    uint32_t *planes = a_lds + group * kAdapterGroupWords;
    if (use_lds) {
        for (uint32_t c = tid; c < n_counters; c += kAdapterBlock) tally[c] = 0u;
        __syncthreads();
    }
    const uint32_t n_pad = (n + 3u) & ~3u;
    // (32-bit item numbers: a chunk is at most 2^22 templates of 16 inputs, the grid at most 2^16 workgroups -- fqtk_demux.hip)
    const uint32_t n_items = n_pad * A.n_ain, per_round = gridDim.x * kAdapterGroups;
    const uint32_t rounds = (n_items + per_round - 1u) / per_round;
    uint32_t w = blockIdx.x * kAdapterGroups + group;
    // (w - group % 4 is a multiple of 4 and so is n_pad: the wavefront's four items are of one input)
    uint32_t j_next = (uint32_t)__builtin_amdgcn_readfirstlane((int)min(w / n_pad, A.n_ain - 1u));
    AdapterItem next = adapter_item(T, A, n, n_pad, j_next, res, skip, w, n_items);
    for (uint32_t round = 0; round < rounds; ++round) {
        const AdapterItem it = next;
        const uint32_t j = j_next;   // wave-uniform
        w += per_round;
        if (round + 1u < rounds) {   // (the next item's view is on its way while this one is scanned)
            j_next = (uint32_t)__builtin_amdgcn_readfirstlane((int)min(w / n_pad, A.n_ain - 1u));
            next = adapter_item(T, A, n, n_pad, j_next, res, skip, w, n_items);
        }
        if (it.live) {
            const uint32_t n_span = it.n;
            uint32_t trim = 0xFFFFFFFFu;
            if (n_span <= kAdapterMaxSpan && n_span) trim = adapter_scan(T, A, j, planes, lane, it.start, n_span);
            // ---- tally: lane 0 scanned, 1 with_adapter, 2 adapter_bases, 3 short_inserts, 4 too_long
            const bool too_long = n_span > kAdapterMaxSpan, found = trim != 0xFFFFFFFFu;
            const uint32_t add = lane == 0u ? (too_long ? 0u : 1u) : lane == 1u ? (found ? 1u : 0u) : lane == 2u ? (found ? n_span - trim : 0u)
                               : lane == 3u ? (found && trim < A.short_insert ? 1u : 0u) : lane == 4u ? (too_long ? 1u : 0u) : 0u;
            if (add) {
                const uint32_t c = it.s * A.row_words + kAdapterRowWords * j + lane;
                if (use_lds) atomicAdd(tally + c, add);
                else atomicAdd(table + c, (unsigned long long)add);
            }
        }
        if (use_lds && (round + 1u) % kAdapterFlushRounds == 0u && round + 1u < rounds) {   // (uniform over the workgroup)
            __syncthreads();
            for (uint32_t c = tid; c < n_counters; c += kAdapterBlock) {
                const uint32_t v = tally[c];
                if (v) { atomicAdd(table + c, (unsigned long long)v); tally[c] = 0u; }
            }
            __syncthreads();
        }
    }
    if (use_lds) {
        __syncthreads();
        for (uint32_t c = tid; c < n_counters; c += kAdapterBlock) {
            const uint32_t v = tally[c];
            if (v) atomicAdd(table + c, (unsigned long long)v);
        }
    }
}

}  // namespace demux
}  // namespace fqtk
