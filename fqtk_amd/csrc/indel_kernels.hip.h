// indel_kernels.hip.h -- INDEL RESCUE of the unmatched reads (include/fqtk_match.h, fqtk_matcher_indel_*; DESIGN.md section
// 5.1g): a read the matcher's substitution-only rule left None gets a second look under the sequence-Levenshtein distance
// (edit distance, minimum over the last row and the last column of the DP matrix: an inserted base pushes the barcode's tail
// out of a fixed-length index read, a deleted one pulls adapter bases in), and is assigned when exactly one sample is close.
//
// indel_rescue_kernel runs behind a batch's matcher kernels, on the batch's stream, in front of the census and the pair tally.
//   * STREAM AND COMPACT, as pairs_kernel does: workgroups of 512 lanes stride over tiles of 2048 results, the None reads of
//     exactly L bases are appended to a queue in LDS (ballot, rank by mbcnt, one LDS atomic per wave and load), the None reads
//     of another length are counted as `skipped`.
//   * DRAIN WHEN EVERY WAVE HAS WORK.  A (read, sample) pair costs L columns of 20 VALU ops, three orders over a Hamming
//     compare, so the kernel's time IS the drain.  The queue is left to fill over tiles until it holds a wave's worth for each
//     of the workgroup's 8 waves (512 entries); then all whole chunks of 64 go, a wave each, and the remainder (< 64) moves to
//     the front.  One more round behind the workgroup's last tile drains what is left.  At most 511 + 2048 entries.
//   * SCAN: Myers' bit-vector recurrence with THE READ AS THE PATTERN.  A lane holds one read: its four bit-planes (encode_planes,
//     once) and the vertical delta words Pv / Mv, bit i = read base i, all in VGPRs.  THE SAMPLE IS THE TEXT: text character j
//     is wave-uniform, so its four masks (all ones where bit b is NOT in enc(sample[j]), else zero) come through the scalar
//     cache into SGPRs and the mismatch word is the v_and / 3 x v_and_or chain of update() -- exact for IUPAC codes on either
//     side, no second path for flagged reads.  The table is a layout of its own, [S][ceil(L/4)][4 columns][4 masks]: a group
//     of four columns is one s_load_dwordx16, and the next group (the next sample's first, at a sample's end) is asked for
//     before this group's VALU work.  Bits above L - 1 are never masked: carries only go up.
//     D[L][j] is tracked as `score` from bit L - 1 of the horizontal deltas; the last column D[i][L] is walked up from
//     D[L][L] through Pv / Mv for min(sat, L) rows, all that can hold a value below sat because D[i][L] >= L - i.
//   * best / second as packed keys (distance << 16 | sample) through v_min / v_med3, both starting at (sat << 16 | 0xFFFF).
//   * TALLY: a histogram of S + 1 bins in LDS ([s] = rescued into s, [S] = examined and left None), added once per workgroup to
//     the matcher's counters and, for the rescued bins, to the caller's counts (+ at s, - at S).  Above kMaxLdsHist bins:
//     64-bit atomics straight to HBM for the rescued reads, 64-bit LDS counters for the two totals.
// A rescued read's result word is stored with a plain vector store; a read that stays None is not written at all.
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

constexpr int kIndelBlock = 512;                       // 8 waves; two workgroups per CU
constexpr int kIndelR = 4;                             // results per lane and tile
constexpr uint32_t kIndelTile = kIndelBlock * kIndelR;
constexpr uint32_t kIndelQueue = kIndelTile + kIndelBlock;   // a tile's worth on top of what waits for a full drain (< 512)
constexpr uint32_t kIndelMaxLen = 32;                  // one plane word
constexpr uint32_t kIndelMaxSat = 16;                  // bit 7 of `best` marks an edit distance; the distances stay far below it

struct IndelParams {
    MatchParams m;               // the batch as its matcher kernels saw it (obs, lens, out, counts, n, stride, S, L, lut)
    const uint32_t *tab;         // [S][ceil(L / 4)][4][4]: per sample base the four masks, padded to whole groups of four columns
    unsigned long long *tally;   // [S + 1] rescued into s / examined and left None, then [S + 1] = skipped
    uint32_t max_edits, delta;
};

// One text character (sample base, masks e) against the lane's read: one column of the DP matrix.
__device__ __forceinline__ void indel_column(const Planes<1> &o, const u32x4 &e, uint32_t top, uint32_t &Pv, uint32_t &Mv,
                                             uint32_t &score, uint32_t &low) {
    uint32_t mis = v_and_sv(e.x, o.p[0][0]);
    mis = v_and_or_vsv(o.p[0][1], e.y, mis);
    mis = v_and_or_vsv(o.p[0][2], e.z, mis);
    mis = v_and_or_vsv(o.p[0][3], e.w, mis);
    const uint32_t Eq = ~mis;
    const uint32_t Xv = Eq | Mv;
    const uint32_t Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
    uint32_t Ph = Mv | ~(Xh | Pv);
    const uint32_t Mh = Pv & Xh;
    score += ((Ph >> top) & 1u) - ((Mh >> top) & 1u);
    low = min(low, score);
    Ph = (Ph << 1) | 1u;   // D[0][j] = j: the row above the matrix steps +1 per column
    Pv = (Mh << 1) | ~(Xv | Ph);
    Mv = Ph & Xv;
}

// Every sample over one read: (best, second) as packed keys of the distances saturated at `sat`.
// NG = groups of four columns the instantiation unrolls; ceil(L / 4) <= NG of them are run.
template <int NG>
__device__ __forceinline__ void indel_scan(const_u32x4_ptr tab, uint32_t S, uint32_t L, uint32_t sat, const Planes<1> &o,
                                           uint32_t &best, uint32_t &second) {
    const uint32_t ng = (L + 3u) >> 2, total = S * ng, top = L - 1u, walk = min(sat, L);
    best = second = (sat << 16) | 0xFFFFu;
    SampleGroup<1, 4> cur, nxt;
    cur.load(tab, 0);
    nxt = cur;
    uint32_t f = 0;   // the group in `cur`, counted over the whole table
    for (uint32_t s = 0; s < S; ++s) {
        uint32_t Pv = ~0u, Mv = 0u, score = L, low = L;   // column 0: D[i][0] = i
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            if ((uint32_t)g >= ng) break;   // wave-uniform
            ++f;
            if (f < total) nxt.load(tab, f * 4u);
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if ((uint32_t)(g * 4 + q) < L) indel_column(o, cur.e[q][0], top, Pv, Mv, score, low);
            cur = nxt;
        }
        uint32_t d = score;   // D[L][L]; up the last column: D[i - 1][L] = D[i][L] - bit(i - 1, Pv) + bit(i - 1, Mv)
        for (uint32_t k = 0; k < walk; ++k) {
            const uint32_t bit = top - k;
            d = d - ((Pv >> bit) & 1u) + ((Mv >> bit) & 1u);
            low = min(low, d);
        }
        const uint32_t key = v_lshl_or_vs(min(low, sat), s);
        second = med3_u32(best, second, key);
        best = min(best, key);
    }
}

// VEC: -1 = rows are whole dwords (base and stride 4-aligned, stride >= 4 * ceil(L / 4)), 0 = bytes (load_words).
// NG: 2 / 4 / 8 groups of four columns (L <= 8 / 16 / 32).  LDSHIST: S + 1 <= kMaxLdsHist bins, tallied in LDS.
template <int VEC, int NG, bool LDSHIST>
__global__ __launch_bounds__(kIndelBlock) void indel_rescue_kernel(const IndelParams C) {
    __shared__ unsigned long long lds_q[kIndelQueue];
    __shared__ uint32_t lds_hist[LDSHIST ? kMaxLdsHist : 1];
    __shared__ uint32_t lds_lut[256];
    __shared__ uint32_t lds_qn;
    __shared__ unsigned long long lds_skipped;
    __shared__ unsigned long long lds_left, lds_moved;   // !LDSHIST: examined and left None / rescued, this workgroup

    const MatchParams &P = C.m;
    const uint32_t tid = threadIdx.x;
    const uint32_t lane = __lane_id();
    const uint32_t wave = tid >> 6;
    const uint32_t bins = P.S + 1u;
    if (LDSHIST)
        for (uint32_t b = tid; b < bins; b += kIndelBlock) lds_hist[b] = 0u;
    if (tid < 256) lds_lut[tid] = P.lut[tid];
    if (tid == 0) {
        lds_qn = 0u;
        lds_skipped = 0ull;
        lds_left = 0ull;
        lds_moved = 0ull;
    }
    __syncthreads();

    const uint32_t L = P.L;
    const uint32_t nwords = (L + 3u) >> 2;
    const uint32_t sat = C.max_edits + max(C.delta, 1u);   // never below max_edits + 1: a saturated distance is never accepted
    const const_u32x4_ptr tab = (const_u32x4_ptr)(uintptr_t)C.tab;
    unsigned long long my_skipped = 0;

    // entries [lo, lo + 64) of the queue, `have` of them filled: this wave's lanes scan one read each, store and tally
    const auto drain = [&](uint32_t lo, uint32_t have) {
        const bool live = lane < have;
        const unsigned long long i = live ? lds_q[lo + lane] : 0ull;
        uint32_t row[8];
#pragma unroll
        for (int w = 0; w < 8; ++w) row[w] = 0u;
        if (live) load_words<1, VEC, 8>(P, i, nwords, row);
        Planes<1> o;
        encode_planes<1>(row, nwords, L, lds_lut, o);
        uint32_t best, second;
        indel_scan<NG>(tab, P.S, L, sat, o, best, second);
        if (!live) return;
        const uint32_t bm = best >> 16, nm = second >> 16;
        const bool none = bm > C.max_edits || (nm - bm) < C.delta;
        const uint32_t s = best & 0xFFFFu;
        if (!none) P.out[i] = s | ((0x80u | bm) << 16) | (nm << 24);
        if (LDSHIST) {
            atomicAdd(&lds_hist[none ? P.S : s], 1u);
        } else if (none) {
            atomicAdd(&lds_left, 1ull);
        } else {
            atomicAdd(&lds_moved, 1ull);
            atomicAdd(&C.tally[s], 1ull);
            if (P.counts) atomicAdd(&P.counts[s], 1ull);
        }
    };

    const uint64_t ntiles = (P.n + kIndelTile - 1) / kIndelTile;
    for (uint64_t t = blockIdx.x;; t += gridDim.x) {
        const bool last = t >= ntiles;   // one more round behind the workgroup's last tile: whatever is queued
        if (!last) {
            uint32_t res[kIndelR];
#pragma unroll
            for (int r = 0; r < kIndelR; ++r) {
                const uint64_t i = t * kIndelTile + (uint64_t)r * kIndelBlock + tid;
                res[r] = i < P.n ? P.out[i] : 0u;   // 0 = sample 0 matched: nothing to do
            }
#pragma unroll
            for (int r = 0; r < kIndelR; ++r) {
                const uint64_t i = t * kIndelTile + (uint64_t)r * kIndelBlock + tid;
                const bool none = (res[r] & 0xFFFFu) == kNoMatch;
                const bool queued = none && (!P.lens || P.lens[i] == L);
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
        // workgroup-uniform: nothing until every wave has a chunk, then all whole chunks; everything in the last round
        const uint32_t take = last ? filled : (filled >= (uint32_t)kIndelBlock ? filled & ~63u : 0u);
        for (uint32_t lo = wave * 64u; lo < take; lo += (uint32_t)kIndelBlock) drain(lo, min(64u, take - lo));
        if (last) break;
        if (take == 0u) continue;
        __syncthreads();   // the whole chunks are read: their room is free
        if (wave == 0) {   // the remainder to the front; take >= 512 > remainder, so the two ranges are apart
            const uint32_t rem = filled - take;
            const unsigned long long e = lane < rem ? lds_q[take + lane] : 0ull;
            if (lane < rem) lds_q[lane] = e;
            if (lane == 0) lds_qn = rem;
        }
        __syncthreads();
    }

    if (my_skipped) atomicAdd(&lds_skipped, my_skipped);
    __syncthreads();
    unsigned long long moved = 0;   // this lane's share of the rescued reads: they leave the caller's bin S
    if (LDSHIST) {
        for (uint32_t b = tid; b < bins; b += kIndelBlock) {
            const uint32_t v = lds_hist[b];
            if (!v) continue;
            atomicAdd(&C.tally[b], (unsigned long long)v);
            if (b < P.S && P.counts) {
                atomicAdd(&P.counts[b], (unsigned long long)v);
                moved += v;
            }
        }
    } else if (tid == 1) {
        if (lds_left) atomicAdd(&C.tally[P.S], lds_left);
        if (P.counts) moved = lds_moved;
    }
    if (moved) atomicAdd(&P.counts[P.S], 0ull - moved);
    if (tid == 0 && lds_skipped) atomicAdd(&C.tally[bins], lds_skipped);
}

// ---- host side: the state a fqtk_matcher owns and what its fqtk_matcher_indel_* entry points do -------------------------
#define FQTK_INDEL_TRY(expr)                                                                                    \
    do {                                                                                                        \
        hipError_t _e = (expr);                                                                                 \
        if (_e != hipSuccess) return internal::set_error(FQTK_EHIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

struct Indel {
    uint32_t *d_tab = nullptr;               // [S][ceil(L / 4)][4][4]
    unsigned long long *d_tally = nullptr;   // [S + 2]: rescued[S + 1], then skipped
    std::vector<uint64_t> kept;              // the counters as disable found them: readable until the next enable
    uint32_t S = 0, max_edits = 0, delta = 0;
    bool on() const { return d_tally != nullptr; }
};

inline int indel_disable(Indel &x) {
    if (x.d_tab || x.d_tally) FQTK_INDEL_TRY(hipDeviceSynchronize());   // a rescue kernel may still be running
    if (x.d_tally) {
        x.kept.resize((size_t)x.S + 2);
        FQTK_INDEL_TRY(hipMemcpy(x.kept.data(), x.d_tally, x.kept.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
    }
    if (x.d_tab) FQTK_INDEL_TRY(hipFree(x.d_tab));
    x.d_tab = nullptr;
    if (x.d_tally) FQTK_INDEL_TRY(hipFree(x.d_tally));
    x.d_tally = nullptr;
    return FQTK_OK;
}

inline int indel_reset(Indel &x) {
    if (!x.on()) return internal::set_error(FQTK_EINVAL, "the indel rescue is not enabled");
    FQTK_INDEL_TRY(hipDeviceSynchronize());
    FQTK_INDEL_TRY(hipMemset(x.d_tally, 0, ((size_t)x.S + 2) * sizeof(unsigned long long)));
    FQTK_INDEL_TRY(hipDeviceSynchronize());   // the batches run on non-blocking streams
    return FQTK_OK;
}

// barcodes = the table as the matcher keeps it (upper case), enc = the reference's encode() of one byte.
inline int indel_enable(Indel &x, const std::vector<std::string> &barcodes, uint32_t L, uint32_t max_edits, uint32_t delta,
                        uint8_t (*enc)(uint8_t)) {
    if (L > kIndelMaxLen)
        return internal::set_error(FQTK_EINVAL, "the indel rescue takes barcodes of at most 32 bases; this table's have " + std::to_string(L));
    const uint64_t sat = (uint64_t)max_edits + delta;
    if (sat == 0 || sat > kIndelMaxSat)
        return internal::set_error(FQTK_EINVAL, "the indel rescue needs 1 <= max_edits + min_edit_delta <= 16, got " + std::to_string(max_edits) +
                                                    " + " + std::to_string(delta));
    if (max_edits >= L)
        return internal::set_error(FQTK_EINVAL, "the indel rescue needs max_edits below the barcode length: max_edits < " + std::to_string(L) +
                                                    ", got " + std::to_string(max_edits));
    const int rc = indel_disable(x);
    if (rc != FQTK_OK) return rc;
    x.kept.clear();
    const uint32_t S = (uint32_t)barcodes.size(), lp = ((L + 3u) / 4u) * 4u;
    std::vector<uint32_t> tab((size_t)S * lp * 4, 0u);   // the padding columns are loaded, never run
    for (uint32_t s = 0; s < S; ++s)
        for (uint32_t j = 0; j < L; ++j) {
            const uint32_t code = enc((uint8_t)barcodes[s][j]);
            for (uint32_t b = 0; b < 4; ++b)
                if (!((code >> b) & 1u)) tab[((size_t)s * lp + j) * 4 + b] = 0xFFFFFFFFu;
        }
    FQTK_INDEL_TRY(hipMalloc(reinterpret_cast<void **>(&x.d_tab), tab.size() * sizeof(uint32_t)));
    FQTK_INDEL_TRY(hipMemcpy(x.d_tab, tab.data(), tab.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (hipMalloc(reinterpret_cast<void **>(&x.d_tally), ((size_t)S + 2) * sizeof(unsigned long long)) != hipSuccess) {   // on() only from here
        (void)hipGetLastError();
        x.d_tally = nullptr;
        (void)indel_disable(x);
        return internal::set_error(FQTK_ENOMEM, "indel rescue: no device memory for the counters");
    }
    x.S = S;
    x.max_edits = max_edits;
    x.delta = delta;
    return indel_reset(x);
}

// Behind a batch's matcher kernels (fqtk_match.hip, launch()): P = the batch, its results on `stream`; P.stride >= P.L.
inline int indel_launch(const Indel &x, const MatchParams &P, int num_cus, hipStream_t stream) {
    if (P.n == 0) return FQTK_OK;
    IndelParams C;
    C.m = P;
    C.tab = x.d_tab;
    C.tally = x.d_tally;
    C.max_edits = x.max_edits;
    C.delta = x.delta;
    const uint64_t ntiles = (P.n + kIndelTile - 1) / kIndelTile;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(ntiles, (uint64_t)num_cus * 2);
    // an LDS bin is 32 bits: the LDS form only where a workgroup sees fewer than 2^32 results
    const bool lds = P.S + 1 <= kMaxLdsHist && (ntiles + grid - 1) / grid < (1ull << 32) / kIndelTile;
    const bool dwords = P.stride % 4 == 0 && reinterpret_cast<uintptr_t>(P.obs) % 4 == 0 && P.stride >= ((P.L + 3) / 4) * 4;
#define FQTK_INDEL_LAUNCH(NG)                                                                                              \
    do {                                                                                                                   \
        if (lds) {                                                                                                         \
            if (dwords) hipLaunchKernelGGL((indel_rescue_kernel<-1, NG, true>), dim3(grid), dim3(kIndelBlock), 0, stream, C);  \
            else hipLaunchKernelGGL((indel_rescue_kernel<0, NG, true>), dim3(grid), dim3(kIndelBlock), 0, stream, C);      \
        } else {                                                                                                           \
            if (dwords) hipLaunchKernelGGL((indel_rescue_kernel<-1, NG, false>), dim3(grid), dim3(kIndelBlock), 0, stream, C); \
            else hipLaunchKernelGGL((indel_rescue_kernel<0, NG, false>), dim3(grid), dim3(kIndelBlock), 0, stream, C);     \
        }                                                                                                                  \
    } while (0)
    if (P.L <= 8) FQTK_INDEL_LAUNCH(2);
    else if (P.L <= 16) FQTK_INDEL_LAUNCH(4);
    else FQTK_INDEL_LAUNCH(8);
#undef FQTK_INDEL_LAUNCH
    FQTK_INDEL_TRY(hipGetLastError());
    return FQTK_OK;
}

// Synchronises the device and copies the S + 1 counters and `skipped`; the tally stays as it is.  After disable: the counters
// as disable found them.
inline int indel_read(Indel &x, uint64_t *rescued, uint64_t *skipped) {
    if (!x.on() && !x.kept.empty()) {   // disabled: what it had
        if (rescued) std::copy(x.kept.begin(), x.kept.end() - 1, rescued);
        if (skipped) *skipped = x.kept.back();
        return FQTK_OK;
    }
    if (!x.on()) return internal::set_error(FQTK_EINVAL, "the indel rescue is not enabled");
    FQTK_INDEL_TRY(hipDeviceSynchronize());
    if (rescued) FQTK_INDEL_TRY(hipMemcpy(rescued, x.d_tally, ((size_t)x.S + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (skipped) FQTK_INDEL_TRY(hipMemcpy(skipped, x.d_tally + x.S + 1, sizeof(uint64_t), hipMemcpyDeviceToHost));
    return FQTK_OK;
}

}  // namespace fqtk
