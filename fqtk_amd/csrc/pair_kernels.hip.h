// pair_kernels.hip.h -- device-side tally of the INDEX PAIRS the unmatched reads carried (include/fqtk_match.h,
// fqtk_matcher_pairs_*): each index of a None read is assigned on its own against the run's distinct
// index-1 / index-2 strings with the matcher's own rule, and the pairs are counted in a (U_A + 1) x (U_B + 1) matrix.
//
// pairs_kernel runs behind a batch's last matcher kernel, on the batch's stream.  None reads are sparse in out[] (a few
// percent), and a scan over U_A + U_B entries with one lane per RESULT would run with almost every lane idle, so:
//   * STREAM AND COMPACT.  Workgroups of 512 lanes stride over tiles of 2048 results (coalesced, four loads in flight per lane).
//     Lanes that hold a None result of exactly L bases append the read's index to a queue in the workgroup's LDS: ballot,
//     rank by mbcnt, ONE LDS atomic per wave and load.  None reads of another length are counted as `skipped` on the spot.
//   * DRAIN IN WHOLE WAVES.  After a tile the workgroup takes the queue down in chunks of 64 entries, a wave each: every lane of
//     a draining wave has a read.  The remainder (< 64) moves to the queue's front and waits for the next tile; one more round
//     behind a workgroup's last tile drains the partial chunk.  The queue holds at most 63 + 2048 entries.
//   * SCAN.  A draining lane fetches its row (match_kernels.hip.h's load_words: unaligned bases, stride > L and the clamp to
//     the row are that code's), makes its bit-planes ONCE (encode_planes) and runs them, unshifted, over the A entries and
//     then over the B entries with update(): an entry is a whole-barcode plane word, pre-inverted, with the positions outside
//     its index left 0 = "matches anything".  The entries are wave-uniform and come through the scalar cache into SGPRs, four
//     entries (one s_load_dwordx16) ahead, as in match_kernel: up to 2 x 65534 entries of 16 bytes do not fit LDS beside the
//     matrix, and update()'s VALU ops take their table operand from an SGPR.
//   * TALLY.  At most 8192 cells: a 32-bit matrix in LDS, added to the 64-bit matrix in HBM once, at the end (the host
//     launches this form only when a workgroup sees fewer than 2^32 results, so no cell can wrap).  More cells: 64-bit atomics
//     straight to HBM, but for the last cell (neither index assigned: where every foreign read lands), which has a 64-bit
//     counter in LDS.  Either way the lanes of a wave that hit the leading lane's cell are folded into one add first.
// No lane waits for another lane's store; every loop is bounded by the batch, the table or a constant.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/fqtk_match.h"
#include "match_kernels.hip.h"
#include "matcher_internal.hpp"

namespace fqtk {

constexpr int kPairsBlock = 512;                     // 8 waves; two workgroups per CU
constexpr int kPairsR = 4;                           // results per lane and tile
constexpr uint32_t kPairsTile = kPairsBlock * kPairsR;
constexpr uint32_t kPairsQueue = kPairsTile + 64;    // a tile's worth on top of a carried remainder (< 64)
constexpr uint32_t kPairsLdsCells = 8192;            // matrices up to here are tallied in LDS (32 KiB)
constexpr uint32_t kPairsMaxLen = 32;                // one plane word
constexpr uint64_t kPairsMaxCells = 1ull << 24;      // 128 MiB of counters

struct PairsParams {
    MatchParams m;               // the batch as its matcher kernels saw it (obs, lens, out, n, stride, L, lut)
    const uint32_t *tab;         // [u_a + u_b][4] pre-inverted planes over the whole barcode's word: A's entries, then B's
    unsigned long long *mat;     // [(u_a + 1) * (u_b + 1)] cells, then [cells] = skipped
    uint32_t u_a, u_b;
    uint32_t mm_i, delta_i;      // the per-index max_mismatches / min_mismatch_delta
};

// One list (n entries from `tab` on) over one read: the packed keys (mismatches << 16 | entry) of the best and the second best
// entry, kKeyInit where there is none (per_index_kernels.hip.h turns them into a result; pairs_assign below into a cell).
__device__ __forceinline__ void pairs_scan(const_u32x4_ptr tab, uint32_t n, const Planes<1> &o, uint32_t &best, uint32_t &second) {
    best = second = kKeyInit;
    constexpr int G = 4;   // 16 dwords = one s_load_dwordx16, the next group asked for before this one's VALU work
    const uint32_t ngroups = n / G;
    SampleGroup<1, G> cur, nxt;
    if (ngroups) cur.load(tab, 0);
    for (uint32_t g = 0; g < ngroups; ++g) {
        if (g + 1 < ngroups) nxt.load(tab, (g + 1) * G);
#pragma unroll
        for (int q = 0; q < G; ++q) update<1>(o, cur.e[q], g * G + q, best, second);
        cur = nxt;
    }
    for (uint32_t s = ngroups * G; s < n; ++s) {
        SampleGroup<1, 1> one;
        one.load(tab, s);
        update<1>(o, one.e[0], s, best, second);
    }
}

// The assigned entry of one list, or n = unassigned (barcode_matching.rs:119-159 on one index).
__device__ __forceinline__ uint32_t pairs_assign(const_u32x4_ptr tab, uint32_t n, const Planes<1> &o, uint32_t mm_i, uint32_t delta_i) {
    uint32_t best, second;
    pairs_scan(tab, n, o, best, second);
    const uint32_t bm = best >> 16, nm = second >> 16;   // one entry: second stays at its initial 255
    return (bm > mm_i || (nm - bm) < delta_i) ? n : (best & 0xFFFFu);
}

// VEC: -1 = rows are whole dwords (base and stride 4-aligned, stride >= 4 * ceil(L / 4)), 0 = bytes (load_words).
// LDSMAT: the matrix has at most kPairsLdsCells cells and is tallied in LDS.
template <int VEC, bool LDSMAT>
__global__ __launch_bounds__(kPairsBlock) void pairs_kernel(const PairsParams C) {
    __shared__ unsigned long long lds_q[kPairsQueue];
    __shared__ uint32_t lds_mat[LDSMAT ? kPairsLdsCells : 1];
    __shared__ uint32_t lds_lut[256];
    __shared__ uint32_t lds_qn;
    __shared__ unsigned long long lds_skipped;
    __shared__ unsigned long long lds_neither;   // !LDSMAT: the last cell (neither index assigned; every foreign read lands there)

    const MatchParams &P = C.m;
    const uint32_t tid = threadIdx.x;
    const uint32_t lane = __lane_id();
    const uint32_t wave = tid >> 6;
    const uint32_t cells = (C.u_a + 1u) * (C.u_b + 1u);
    if (LDSMAT)
        for (uint32_t c = tid; c < cells; c += kPairsBlock) lds_mat[c] = 0u;
    if (tid < 256) lds_lut[tid] = P.lut[tid];
    if (tid == 0) {
        lds_qn = 0u;
        lds_skipped = 0ull;
        lds_neither = 0ull;
    }
    __syncthreads();

    const uint32_t L = P.L;
    const uint32_t nwords = (L + 3u) >> 2;
    const bool rows_hold_a_barcode = P.stride >= L;   // else every read is shorter than L: skipped
    const const_u32x4_ptr tab_a = (const_u32x4_ptr)(uintptr_t)C.tab;
    const const_u32x4_ptr tab_b = tab_a + C.u_a;
    unsigned long long my_skipped = 0;

    // entries [lo, lo + 64) of the queue, `have` of them filled: this wave's lanes scan one read each and tally
    const auto drain = [&](uint32_t lo, uint32_t have) {
        const bool live = lane < have;
        uint32_t row[8];
#pragma unroll
        for (int w = 0; w < 8; ++w) row[w] = 0u;
        if (live) load_words<1, VEC, 8>(P, lds_q[lo + lane], nwords, row);
        Planes<1> o;
        encode_planes<1>(row, nwords, L, lds_lut, o);
        const uint32_t a = pairs_assign(tab_a, C.u_a, o, C.mm_i, C.delta_i);
        const uint32_t b = pairs_assign(tab_b, C.u_b, o, C.mm_i, C.delta_i);
        const uint32_t cell = a * (C.u_b + 1u) + b;
        // fold the lanes that hit the first live lane's cell into that lane (all-random reads: every lane, the last cell)
        const unsigned long long lives = __ballot(live);
        const int lead = __ffsll((long long)lives) - 1;
        const bool same = live && cell == (uint32_t)__shfl((int)cell, lead);
        const unsigned long long group = __ballot(same);
        const uint32_t c = same ? (uint32_t)__popcll(group) : 1u;
        if (!live || (same && (int)lane != lead)) return;
        if (LDSMAT) atomicAdd(&lds_mat[cell], c);
        else if (cell == cells - 1u) atomicAdd(&lds_neither, (unsigned long long)c);
        else atomicAdd(&C.mat[cell], (unsigned long long)c);
    };

    const uint64_t ntiles = (P.n + kPairsTile - 1) / kPairsTile;
    for (uint64_t t = blockIdx.x;; t += gridDim.x) {
        const bool last = t >= ntiles;   // one more round behind the workgroup's last tile: the partial chunk
        if (!last) {
            uint32_t res[kPairsR];
#pragma unroll
            for (int r = 0; r < kPairsR; ++r) {
                const uint64_t i = t * kPairsTile + (uint64_t)r * kPairsBlock + tid;
                res[r] = i < P.n ? FQTK_STREAM_LOAD(&P.out[i]) : 0u;   // 0 = sample 0 matched: nothing to do
            }
#pragma unroll
            for (int r = 0; r < kPairsR; ++r) {
                const uint64_t i = t * kPairsTile + (uint64_t)r * kPairsBlock + tid;
                const bool none = (res[r] & 0xFFFFu) == kNoMatch;
                const bool queued = none && rows_hold_a_barcode && (!P.lens || P.lens[i] == L);
                if (none && !queued) ++my_skipped;
                const unsigned long long b = __ballot(queued);
                if (b == 0ull) continue;   // wave-uniform: the common case
                const int lead = __ffsll((long long)b) - 1;
                uint32_t base = 0;
                if ((int)lane == lead) base = atomicAdd(&lds_qn, (uint32_t)__popcll(b));
                base = (uint32_t)__shfl((int)base, lead);
                if (queued) lds_q[base + __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u))] = i;
            }
        }
        __syncthreads();   // the tile's appends are in
        const uint32_t filled = lds_qn;
        __syncthreads();   // every lane has read the fill: the next append may move it
        const uint32_t take = last ? filled : filled & ~63u;   // workgroup-uniform
        for (uint32_t lo = wave * 64u; lo < take; lo += (uint32_t)kPairsBlock) drain(lo, min(64u, take - lo));
        if (last) break;
        if (take == 0u) continue;
        __syncthreads();   // the whole chunks are read: their room is free
        if (wave == 0) {   // the remainder to the front; take >= 64 > remainder, so the two ranges are apart
            const uint32_t rem = filled - take;
            const unsigned long long e = lane < rem ? lds_q[take + lane] : 0ull;
            if (lane < rem) lds_q[lane] = e;
            if (lane == 0) lds_qn = rem;
        }
        __syncthreads();
    }

    if (my_skipped) atomicAdd(&lds_skipped, my_skipped);
    __syncthreads();
    if (LDSMAT)
        for (uint32_t c = tid; c < cells; c += kPairsBlock) {
            const uint32_t v = lds_mat[c];
            if (v) atomicAdd(&C.mat[c], (unsigned long long)v);
        }
    if (tid == 0 && lds_skipped) atomicAdd(&C.mat[cells], lds_skipped);
    if (!LDSMAT && tid == 1 && lds_neither) atomicAdd(&C.mat[cells - 1u], lds_neither);
}

// ---- host side: the state a fqtk_matcher owns and what its fqtk_matcher_pairs_* entry points do -------------------------
#define FQTK_PAIRS_TRY(expr)                                                                                    \
    do {                                                                                                        \
        hipError_t _e = (expr);                                                                                 \
        if (_e != hipSuccess) return internal::set_error(FQTK_EHIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

struct Pairs {
    uint32_t *d_tab = nullptr;              // [u_a + u_b][4]
    unsigned long long *d_mat = nullptr;    // [cells + 1]: the matrix, then skipped
    std::vector<std::string> index[2];      // A, B: distinct index strings in order of first appearance
    uint32_t len_a = 0, mm_i = 0, delta_i = 0;
    uint64_t cells() const { return (uint64_t)(index[0].size() + 1) * (index[1].size() + 1); }
    bool on() const { return d_mat != nullptr; }
};

inline int pairs_disable(Pairs &p) {
    if (p.d_tab || p.d_mat) FQTK_PAIRS_TRY(hipDeviceSynchronize());   // a pairs kernel may still be running
    if (p.d_tab) FQTK_PAIRS_TRY(hipFree(p.d_tab));
    p.d_tab = nullptr;
    if (p.d_mat) FQTK_PAIRS_TRY(hipFree(p.d_mat));
    p.d_mat = nullptr;
    p.index[0].clear();
    p.index[1].clear();
    return FQTK_OK;
}

inline int pairs_reset(Pairs &p) {
    if (!p.on()) return internal::set_error(FQTK_EINVAL, "the index-pair tally is not enabled");
    FQTK_PAIRS_TRY(hipDeviceSynchronize());
    FQTK_PAIRS_TRY(hipMemset(p.d_mat, 0, (p.cells() + 1) * sizeof(unsigned long long)));
    FQTK_PAIRS_TRY(hipDeviceSynchronize());   // the batches run on non-blocking streams
    return FQTK_OK;
}

// A and B of include/fqtk_match.h: the distinct strings barcode_s[0 : len_a] and barcode_s[len_a :], each in order of first appearance.
inline void pairs_split_indexes(const std::vector<std::string> &barcodes, uint32_t len_a, std::vector<std::string> (&index)[2]) {
    for (const std::string &b : barcodes) {
        const std::string part[2] = {b.substr(0, len_a), b.substr(len_a)};
        for (int w = 0; w < 2; ++w)
            if (std::find(index[w].begin(), index[w].end(), part[w]) == index[w].end()) index[w].push_back(part[w]);
    }
}

// [u_a + u_b][4] pre-inverted planes over the whole barcode's word: A's entries, then B's, the positions outside an index left 0.
inline std::vector<uint32_t> pairs_plane_table(const std::vector<std::string> (&index)[2], uint32_t len_a, uint8_t (*enc)(uint8_t)) {
    std::vector<uint32_t> tab((index[0].size() + index[1].size()) * 4, 0u);
    size_t e = 0;
    for (int w = 0; w < 2; ++w)
        for (const std::string &s : index[w]) {
            for (size_t k = 0; k < s.size(); ++k) {
                const uint32_t code = enc((uint8_t)s[k]), bit = (uint32_t)k + (w ? len_a : 0u);
                for (uint32_t j = 0; j < 4; ++j)
                    if (!((code >> j) & 1u)) tab[e * 4 + j] |= 1u << bit;
            }
            ++e;
        }
    return tab;
}

// barcodes = the table as the matcher keeps it (upper case), enc = the reference's encode() of one byte.
inline int pairs_enable(Pairs &p, const std::vector<std::string> &barcodes, uint32_t L, uint32_t len_a, uint32_t mm_i, uint32_t delta_i,
                        uint8_t (*enc)(uint8_t)) {
    if (L > kPairsMaxLen)
        return internal::set_error(FQTK_EINVAL, "the index-pair tally takes barcodes of at most 32 bases; this table's have " + std::to_string(L));
    if (len_a == 0 || len_a >= L)
        return internal::set_error(FQTK_EINVAL, "the split point len_a must leave both indexes a base: 1 <= len_a < " + std::to_string(L) +
                                                    ", got " + std::to_string(len_a));
    std::vector<std::string> index[2];
    pairs_split_indexes(barcodes, len_a, index);
    const uint64_t cells = (uint64_t)(index[0].size() + 1) * (index[1].size() + 1);
    if (cells > kPairsMaxCells)
        return internal::set_error(FQTK_EINVAL, "the index-pair matrix would have " + std::to_string(cells) + " cells; at most 2^24 (128 MiB) are tallied");
    const int rc = pairs_disable(p);
    if (rc != FQTK_OK) return rc;
    const std::vector<uint32_t> tab = pairs_plane_table(index, len_a, enc);
    FQTK_PAIRS_TRY(hipMalloc(reinterpret_cast<void **>(&p.d_tab), tab.size() * sizeof(uint32_t)));
    FQTK_PAIRS_TRY(hipMemcpy(p.d_tab, tab.data(), tab.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (hipMalloc(reinterpret_cast<void **>(&p.d_mat), (cells + 1) * sizeof(unsigned long long)) != hipSuccess) {   // on() only from here
        (void)hipGetLastError();
        p.d_mat = nullptr;
        (void)pairs_disable(p);
        return internal::set_error(FQTK_ENOMEM, "index pairs: no device memory for " + std::to_string(cells) + " cells");
    }
    p.index[0] = std::move(index[0]);
    p.index[1] = std::move(index[1]);
    p.len_a = len_a;
    p.mm_i = mm_i;
    p.delta_i = delta_i;
    return pairs_reset(p);
}

// The end of a batch (fqtk_match.hip, launch()): P = the batch, its results final on `stream`.
inline int pairs_launch(const Pairs &p, const MatchParams &P, int num_cus, hipStream_t stream) {
    if (P.n == 0) return FQTK_OK;
    PairsParams C;
    C.m = P;
    C.tab = p.d_tab;
    C.mat = p.d_mat;
    C.u_a = (uint32_t)p.index[0].size();
    C.u_b = (uint32_t)p.index[1].size();
    C.mm_i = p.mm_i;
    C.delta_i = p.delta_i;
    const uint64_t ntiles = (P.n + kPairsTile - 1) / kPairsTile;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(ntiles, (uint64_t)num_cus * 2);
    // an LDS cell is 32 bits: the LDS form only where a workgroup sees fewer than 2^32 results
    const bool lds = p.cells() <= kPairsLdsCells && (ntiles + grid - 1) / grid < (1ull << 32) / kPairsTile;
    const bool dwords = P.stride % 4 == 0 && reinterpret_cast<uintptr_t>(P.obs) % 4 == 0 && P.stride >= ((P.L + 3) / 4) * 4;
    if (lds) {
        if (dwords) hipLaunchKernelGGL((pairs_kernel<-1, true>), dim3(grid), dim3(kPairsBlock), 0, stream, C);
        else hipLaunchKernelGGL((pairs_kernel<0, true>), dim3(grid), dim3(kPairsBlock), 0, stream, C);
    } else {
        if (dwords) hipLaunchKernelGGL((pairs_kernel<-1, false>), dim3(grid), dim3(kPairsBlock), 0, stream, C);
        else hipLaunchKernelGGL((pairs_kernel<0, false>), dim3(grid), dim3(kPairsBlock), 0, stream, C);
    }
    FQTK_PAIRS_TRY(hipGetLastError());
    return FQTK_OK;
}

// Synchronises the device and copies the matrix (row-major, (u_a + 1) x (u_b + 1)) and `skipped`; the tally stays as it is.
inline int pairs_read(Pairs &p, uint64_t *matrix, uint64_t *skipped) {
    if (!p.on()) return internal::set_error(FQTK_EINVAL, "the index-pair tally is not enabled");
    FQTK_PAIRS_TRY(hipDeviceSynchronize());
    const uint64_t cells = p.cells();
    if (matrix) FQTK_PAIRS_TRY(hipMemcpy(matrix, p.d_mat, cells * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (skipped) FQTK_PAIRS_TRY(hipMemcpy(skipped, p.d_mat + cells, sizeof(uint64_t), hipMemcpyDeviceToHost));
    return FQTK_OK;
}

}  // namespace fqtk
