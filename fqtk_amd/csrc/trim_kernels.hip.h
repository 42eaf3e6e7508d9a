// trim_kernels.hip.h -- 3' quality and adapter trimming of a chunk's template reads (include/fqtk_demux.h, fqtk_demuxer_trim_*;
// DESIGN.md section 5.1j).  k_trim runs behind the matcher and in front of k_plan_rank and shortens RecView.seq_len of the trimmed
// inputs: placement, formatting, DEFLATE and the quality tally all take a record's extent from seq_len (fmt::segment_span clamps to
// it), so every later kernel sees the trimmed record and none of them changes.
//
// THE RULE (exact integers; the header states it in full).  A TRIMMED INPUT is an input with a T segment, its span its last T
// segment, which is the last segment of its read structure.  R[0..n) / Q[0..n) are the span's sequence / quality bytes:
//   n > 512: too_long += 1, the record stays.  Otherwise scanned += 1 and
//   1. n_q: s = 0, best = 0, n_q = n; for i = n-1 .. 0: s += (cutoff + 33) - Q[i]; s < 0: stop; s > best: best = s, n_q = i
//   2. cut = the adapter rule's smallest hit in R[0..n_q) (adapter_kernels.hip.h), else n_q
//   3. kept = max(cut, min(min_length, n));  4. seq_len = lo + kept.
// A row is 8 counters per trimmed input: [scanned, quality_trimmed, quality_bases, adapter_trimmed, adapter_bases, floored,
// kept_bases, too_long].
//
// WORK SPLIT.  The adapter scan's: an ITEM is a (template, trimmed input) pair, a GROUP of 16 lanes -- one DPP row -- owns it, items
// are numbered input-major over the templates padded to 4 (adapter_item), so a wavefront's adapter is wave-uniform; the grid strides
// in rounds.
//
// QUALITY PASS.  Step 1 is a suffix sum with an early stop and an arg-max: S(i) = sum over k >= i of (cutoff + 33 - Q[k]) does not
// depend on where the loop stops, the loop stops at the LARGEST i with S(i) < 0 (the break), and n_q is the position right of the
// break with the largest S > 0, the largest such position on a tie.
//   load     the quality bytes come in as ALIGNED 16-byte loads through tile_bytes (nothing outside [lead, len) of the text is
//            touched) and go, as they are, into the group's BYTE STRIP in LDS: 33 x 16 B = 528 B (512 bytes + 15 of misalignment).
//   lane     lane w owns positions 32w .. 32w+31 (read coordinates).  It reads 9 dwords of the strip from dword (start & 15) / 4 + 8w
//            and eight v_alignbyte_b32 by start & 3 give its 32 bytes in 8 VGPRs; bytes at and beyond n are masked to zero.
//   total    L_w = count * (cutoff + 33) - sum of the bytes: eight v_sad_u8 against zero.
//   right    T_w = the sum of L_v over v > w: an inclusive suffix scan over the row by four DPP row shifts (row_shl 1, 2, 4, 8; a
//            lane shifted in from outside the row reads 0), minus L_w.
//   walk     one right-to-left walk over the lane's own bytes from T_w (at most 32 steps, no memory access): it stops at the lane's
//            first S < 0 -- the lane's largest negative position -- and keeps, over the positions right of it, the best PACKED KEY
//            S * 512 + i (S > 0 only; S <= 512 * 126 < 2^16, so the key fits 32 bits; "max key" = "max S, then largest i").
//   combine  the break is the row maximum of the lanes' negative positions.  Lanes right of the break's lane hold no negative
//            position and give their key, the break's lane gives its restricted key, lanes left of it give 0: n_q is the low 9
//            bits of the row maximum of the keys, or n when that is 0.
// No atomic, no shuffle through LDS, no per-read loop longer than 32.
//
// ADAPTER PASS.  adapter_scan of adapter_kernels.hip.h -- the bit-plane scan k_adapter runs -- with n_span := n_q, skipped by the
// group as one when n_q < min_overlap (no offset can be a hit) or no adapter was given.
//
// WRITE AND TALLY.  Lane 0 stores seq_len = lo + kept when kept != n.  Lanes 0..7 add one counter each, two levels as in
// adapter_kernels.hip.h: 32-bit counters in LDS when the table has at most kQualLdsCounters words, flushed every
// kAdapterFlushRounds rounds and at the end, else 64-bit atomics to HBM.  An item adds at most 512 to a counter (quality_bases,
// adapter_bases, kept_bases <= n), so the adapter kernel's no-wrap bound holds here as it stands.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "adapter_kernels.hip.h"

namespace fqtk {
namespace demux {

constexpr uint32_t kTrimRowWords = 8;                                  // counters per trimmed input
constexpr uint32_t kTrimStripChunks = (kAdapterMaxSpan + 15u) / 16u + 1u;   // 16-byte pieces of a group's byte strip: 33
constexpr uint32_t kTrimStripWords = kTrimStripChunks * 4u;            // 132 dwords = 528 B
constexpr uint32_t kTrimGroupWords = kTrimStripWords + kAdapterGroupWords;   // LDS words of a group: the strip, then the bit-planes
constexpr uint32_t kTrimMaxCutoff = 93;
static_assert(3u + 8u * 15u + 8u < kTrimStripWords, "lane 15 reads dwords up to 3 + 120 + 8 of the strip");
static_assert(kAdapterMaxSpan * (kTrimMaxCutoff + 33u) < (1u << 16) && kAdapterMaxSpan == 512u, "the packed key S * 512 + i fits 32 bits");

struct TrimConfig {
    AdapterConfig A;          // the trimmed inputs, their last T segments, their adapters' masks and thresholds (row_words = 8 * n_ain; short_insert unused)
    uint32_t has_adapters;    // 0: quality trimming only
    uint32_t min_overlap;
    uint32_t cutoff33;        // quality_cutoff + 33; 0: no quality trimming
    uint32_t min_length;
};

// maximum over the 16 lanes of a DPP row, in every lane of it
__device__ __forceinline__ uint32_t row_max(uint32_t v) {
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false));    // quad_perm [1,0,3,2]
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false));    // quad_perm [2,3,0,1]
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, false));   // row_half_mirror
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, false));   // row_mirror
    return v;
}

// sum of the lanes to the right of this one in its DPP row (row_shl:k -- lane i reads lane i + k; beyond the row: 0)
__device__ __forceinline__ int32_t row_right_sum(int32_t v) {
    int32_t x = v;
    x += __builtin_amdgcn_update_dpp(0, x, 0x101, 0xF, 0xF, true);
    x += __builtin_amdgcn_update_dpp(0, x, 0x102, 0xF, 0xF, true);
    x += __builtin_amdgcn_update_dpp(0, x, 0x104, 0xF, 0xF, true);
    x += __builtin_amdgcn_update_dpp(0, x, 0x108, 0xF, 0xF, true);
    return x - v;
}

// Step 1 of the rule for one item, by its group of 16 lanes: n_q of Q[0..n), Q[0] at byte `start` of the text, 1 <= n <= 512, in
// every lane of the group.  `strip`: the group's kTrimStripWords of LDS.
__device__ __forceinline__ uint32_t quality_cut(const uint8_t *text, uint32_t len, uint32_t lead, uint32_t *strip, uint32_t lane, uint32_t start, uint32_t n,
                                                uint32_t cutoff33) {
    const uint32_t a0 = start & ~15u, sh = start & 15u, end = start + n;
    // ---- load: 16-byte piece (pass * 16 + lane) of the strip, aligned coordinates
    __builtin_amdgcn_wave_barrier();   // (the round before has read its strip)
#pragma unroll
    for (uint32_t p = 0; p < kAdapterPasses; ++p) {
        const uint32_t c = p * 16u + lane, off = a0 + c * 16u;
        if (c < kTrimStripChunks && off < end) {   // (what an earlier item left in the pieces behind `end` lies at and beyond n: masked below)
            const uint4 v = tile_bytes(text, len, off / kLineTile, (off % kLineTile) / 16u, lead);
            strip[4u * c] = v.x; strip[4u * c + 1u] = v.y; strip[4u * c + 2u] = v.z; strip[4u * c + 3u] = v.w;
        }
    }
    __threadfence_block();
    __builtin_amdgcn_wave_barrier();
    // ---- the lane's 32 bytes in read coordinates (byte 0 of q[0] = Q[32 * lane]); bytes at and beyond n are zero
    const int32_t cnt = min(max((int32_t)n - (int32_t)(32u * lane), 0), 32);
    const uint32_t *src = strip + (sh >> 2) + 8u * lane;
    uint32_t q[8], lo_word = src[0], bytes = 0;
#pragma unroll
    for (uint32_t k = 0; k < 8u; ++k) {
        const uint32_t hi_word = src[k + 1u];
        q[k] = __builtin_amdgcn_alignbyte(hi_word, lo_word, sh & 3u) & low_bits(8 * (cnt - (int32_t)(4u * k)));
        bytes = __builtin_amdgcn_sad_u8(q[k], 0u, bytes);
        lo_word = hi_word;
    }
    // ---- S right of the lane, then the walk over its own positions
    int32_t s = row_right_sum(cnt * (int32_t)cutoff33 - (int32_t)bytes), best = 0;
    uint32_t key = 0, neg = 0;   // neg: 1 + the lane's largest position with S < 0; 0: none
    bool open = true;
#pragma unroll
    for (int32_t i = 31; i >= 0; --i) {
        if (i < cnt) {
            s += (int32_t)cutoff33 - (int32_t)((q[i >> 2] >> (8 * (i & 3))) & 0xFFu);
            if (open) {
                if (s < 0) { neg = 32u * lane + (uint32_t)i + 1u; open = false; }
                else if (s > best) { best = s; key = (uint32_t)s * 512u + 32u * lane + (uint32_t)i; }
            }
        }
    }
    // ---- combine: the break, then the best key at and right of the break's lane
    const uint32_t brk = row_max(neg);
    const uint32_t top = row_max(32u * lane + 32u >= brk ? key : 0u);
    return top ? (top & 511u) : n;
}

__global__ __launch_bounds__(kAdapterBlock) void k_trim(TextSet T, TrimConfig C, uint32_t n, const uint32_t *res, const uint8_t *skip,
                                                        unsigned long long *table, uint32_t n_counters, uint32_t use_lds, const ChunkStatus *st) {
    if (no_records(st)) return;
    extern __shared__ uint32_t t_lds[];   // per group the byte strip and the bit-planes, then level 1: n_counters words (use_lds)
    uint32_t *tally = t_lds + kAdapterGroups * kTrimGroupWords;
    const uint32_t tid = threadIdx.x, lane = tid & 15u, group = tid >> 4;
    uint32_t *strip = t_lds + group * kTrimGroupWords, *planes = strip + kTrimStripWords;
    if (use_lds) {
        for (uint32_t c = tid; c < n_counters; c += kAdapterBlock) tally[c] = 0u;
        __syncthreads();
    }
    const AdapterConfig &A = C.A;
    const uint32_t n_pad = (n + 3u) & ~3u;
    const uint32_t n_items = n_pad * A.n_ain, per_round = gridDim.x * kAdapterGroups;
    const uint32_t rounds = (n_items + per_round - 1u) / per_round;
    uint32_t w = blockIdx.x * kAdapterGroups + group;
    uint32_t j_next = (uint32_t)__builtin_amdgcn_readfirstlane((int)min(w / n_pad, A.n_ain - 1u));
    AdapterItem next = adapter_item(T, A, n, n_pad, j_next, res, skip, w, n_items);
    for (uint32_t round = 0; round < rounds; ++round) {
        const AdapterItem it = next;
        const uint32_t j = j_next;   // wave-uniform
        const uint32_t t = w - j * n_pad;
        w += per_round;
        if (round + 1u < rounds) {   // (another item's view: no item is written before it is read)
            j_next = (uint32_t)__builtin_amdgcn_readfirstlane((int)min(w / n_pad, A.n_ain - 1u));
            next = adapter_item(T, A, n, n_pad, j_next, res, skip, w, n_items);
        }
        if (it.live) {
            const uint32_t n_span = it.n;
            const bool too_long = n_span > kAdapterMaxSpan;
            uint32_t n_q = n_span, cut = n_span, kept = n_span;
            if (!too_long) {
                const uint32_t in = A.ain[j];
                RecView *rv = T.rec[in] + t;
                const uint32_t lo = it.start - rv->seq_off;
                if (C.cutoff33 && n_span) n_q = quality_cut(T.text[in], T.len[in], T.lead[in], strip, lane, rv->qual_off + lo, n_span, C.cutoff33);
                cut = n_q;
                if (C.has_adapters && n_q >= C.min_overlap) {   // (the group as one: n_q is the same in its 16 lanes; min_overlap >= 1)
                    const uint32_t trim = adapter_scan(T, A, j, planes, lane, it.start, n_q);
                    if (trim != 0xFFFFFFFFu) cut = trim;
                }
                kept = max(cut, min(C.min_length, n_span));
                if (lane == 0u && kept != n_span) rv->seq_len = lo + kept;
            }
            // ---- tally: lane 0 scanned, 1 quality_trimmed, 2 quality_bases, 3 adapter_trimmed, 4 adapter_bases, 5 floored, 6 kept_bases, 7 too_long
            const uint32_t add = lane == 0u ? (too_long ? 0u : 1u) : lane == 1u ? (n_q < n_span ? 1u : 0u) : lane == 2u ? n_span - n_q
                               : lane == 3u ? (cut < n_q ? 1u : 0u) : lane == 4u ? n_q - cut : lane == 5u ? (kept > cut ? 1u : 0u)
                               : lane == 6u ? (too_long ? 0u : kept) : lane == 7u ? (too_long ? 1u : 0u) : 0u;
            if (add) {
                const uint32_t c = it.s * A.row_words + kTrimRowWords * j + lane;
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
