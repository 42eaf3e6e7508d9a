// census_kernels.hip.h -- device-side census of the barcodes the matcher could NOT assign (include/fqtk_match.h,
// fqtk_matcher_census_*): a hash aggregation (barcode -> templates) over data that is already in HBM.
//
// census_kernel runs behind a batch's last matcher kernel, on the batch's stream:
//   * it STREAMS out[] (4 B per read, coalesced, four loads in flight per lane) and touches a barcode row only for a None
//     result -- with match_kernels.hip.h's load paths, so an unaligned base, stride > L and the clamp to the row are theirs;
//   * the KEY of a read is the reference's own 4-bit encoding (mod.rs:26-61), base k in nibble k % 16 of key word k / 16: one
//     64-bit word for L <= 16, two for L <= 32.  A keyed read has no zero nibble inside L and L >= 1 (17 for the second word),
//     so no key word is ever 0 -- 0 is EMPTY, and the pad nibbles above L can stay 0;
//   * LEVEL 1, the workgroup's LDS: an open-addressing table (4096 / 2048 slots of key words + a 32-bit count, 49 / 41 KiB; two
//     workgroups of 512 lanes per CU, so 98 / 82 of the CU's 160 KiB).  The grid is at most two workgroups per CU and strides
//     over the batch, so a table lives for many tiles and is flushed ONCE, at the end: level 2 sees about one add per
//     (workgroup, distinct key).  Before LDS is touched the lanes of a wave that carry the key of the wave's first keyed lane
//     are folded into one add (64 lanes, one key -- poly-G -- would otherwise serialise on one LDS address);
//   * LEVEL 2, the matcher's table in HBM: `capacity` slots of key words + a 64-bit count;
//   * at both levels a key's probe sequence is the eight slots of ONE aligned bucket, chosen by its hash and tried in order: in HBM
//     that is one 128-byte line (two key words: 192 bytes), fetched with loads that do not wait for each other.
//
// The claim protocol, the same at both levels.  A key word only ever goes EMPTY -> value.  At a slot of its probe sequence a
// key (1) reads word 0: another value rejects the slot; EMPTY is claimed with a 64-bit compare-and-swap whose old value is
// judged the same way; (2) does the same with word 1; (3) adds to the count.  Every judgement is final: a word that holds
// another value holds it for good (so a stale read can only show EMPTY, and then the compare-and-swap decides), and a word that
// holds the key's value keeps it.  Hence a key is accepted by at most one slot -- the first of its (fixed, bounded) probe
// sequence (its bucket) that did not reject it -- so no key is stored twice and a stored count is exact; and a key that ran out of probes
// once runs out of them forever after (rejections are permanent), so a dropped key can never appear later with a part of its
// count: it is in `overflow`, whole.  Two keys that share word 0 may both pass step 1 at a slot; step 2 lets one of them in and
// sends the other on.  NO LANE EVER WAITS for another lane's store: there is no spin loop, no lock and no half-published
// state to wait out -- every loop here is bounded by a constant.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/fqtk_match.h"
#include "match_kernels.hip.h"
#include "matcher_internal.hpp"

namespace fqtk {

constexpr int kCensusBlock = 512;            // 8 waves; two workgroups per CU
constexpr int kCensusR = 4;                  // results per lane and tile
constexpr uint32_t kCensusBucket = 8;        // a key's probe sequence, at both levels: the slots of one aligned bucket (level 2: 128 / 192 bytes)
constexpr uint32_t kCensusMaxLen = 32;       // two key words
template <int KW> constexpr uint32_t kCensusLdsSlots = KW == 1 ? 4096u : 2048u;

struct CensusParams {
    MatchParams m;                 // the batch as its matcher kernels saw it (obs, lens, out, n, stride, L, lut)
    unsigned long long *slots;     // [mask + 1][KW + 1]: key words, count
    uint64_t mask;                 // capacity - 1
    unsigned long long *tot;       // [0] unkeyed, [1] overflow
};

__device__ __forceinline__ uint64_t census_hash(uint64_t w0, uint64_t w1) {
    uint64_t h = (w0 ^ (w1 * 0xD6E8FEB86659FD93ull)) * 0x9E3779B97F4A7C15ull;
    h ^= h >> 29;
    h *= 0xBF58476D1CE4E5B9ull;
    return h ^ (h >> 32);
}

// One key word at one slot: true = the word holds `w` (now or already), false = it holds another key's word, for good.
__device__ __forceinline__ bool census_word(unsigned long long *p, unsigned long long w) {
    unsigned long long cur = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == 0ull) {
        cur = atomicCAS(p, 0ull, w);
        if (cur == 0ull) return true;
    }
    return cur == w;
}

// One key at one BUCKET of kCensusBucket consecutive slots -- the whole of its probe sequence, at either level.  k0 / k1 = word 0 /
// word 1 of the bucket's first slot, `stride` = 64-bit words from slot to slot, add(j) = add to the count of slot j.  The word-0
// column is read first, all of it, with loads that do not depend on each other (one latency, one or two cache lines in HBM): what
// such a read shows other than EMPTY is final, so a full bucket turns a read away without a single atomic.
template <int KW, typename Add>
__device__ __forceinline__ bool census_bucket_add(unsigned long long *k0, unsigned long long *k1, uint32_t stride, unsigned long long w0,
                                                  unsigned long long w1, Add add) {
    unsigned long long seen[kCensusBucket];
#pragma unroll
    for (uint32_t j = 0; j < kCensusBucket; ++j) seen[j] = __hip_atomic_load(k0 + j * stride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
    for (uint32_t j = 0; j < kCensusBucket; ++j) {
        unsigned long long cur = seen[j];
        if (cur == 0ull) cur = atomicCAS(k0 + j * stride, 0ull, w0);
        if (cur != 0ull && cur != w0) continue;   // another key's word, for good
        if (KW == 2 && !census_word(k1 + j * stride, w1)) continue;
        add(j);
        return true;
    }
    return false;
}

// Level 2.  `h` = the key's hash (its upper bits choose the bucket: level 1 used the lower ones).
template <int KW>
__device__ __forceinline__ bool census_global_add(const CensusParams &C, uint64_t h, unsigned long long w0, unsigned long long w1,
                                                  unsigned long long c) {
    unsigned long long *e = C.slots + (((h >> 20) & C.mask) & ~(uint64_t)(kCensusBucket - 1)) * (uint64_t)(KW + 1);
    return census_bucket_add<KW>(e, e + 1, KW + 1, w0, w1, [&](uint32_t j) { atomicAdd(e + j * (KW + 1) + KW, c); });
}

// VEC: -1 = rows are whole dwords (base and stride 4-aligned, stride >= 4 * ceil(L / 4)), 0 = bytes (load_words).
template <int KW, int VEC>
__global__ __launch_bounds__(kCensusBlock) void census_kernel(const CensusParams C) {
    constexpr uint32_t SLOTS = kCensusLdsSlots<KW>;
    __shared__ unsigned long long lds_key[KW][SLOTS];
    __shared__ uint32_t lds_cnt[SLOTS];
    __shared__ uint32_t lds_lut[256];
    __shared__ unsigned long long lds_tot[2];

    const MatchParams &P = C.m;
    const uint32_t tid = threadIdx.x;
    for (uint32_t s = tid; s < SLOTS; s += kCensusBlock) {
#pragma unroll
        for (int w = 0; w < KW; ++w) lds_key[w][s] = 0ull;
        lds_cnt[s] = 0u;
    }
    if (tid < 256) lds_lut[tid] = P.lut[tid];
    if (tid < 2) lds_tot[tid] = 0ull;
    __syncthreads();

    const uint32_t L = P.L;
    const uint32_t nwords = (L + 3u) >> 2;
    const bool rows_hold_a_barcode = P.stride >= L;   // else every read is shorter than L: unkeyed
    const uint32_t lane = __lane_id();
    unsigned long long my_unkeyed = 0, my_overflow = 0;

    const uint64_t tile = (uint64_t)kCensusBlock * kCensusR;
    const uint64_t ntiles = (P.n + tile - 1) / tile;
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        uint32_t res[kCensusR];
#pragma unroll
        for (int r = 0; r < kCensusR; ++r) {
            const uint64_t i = t * tile + (uint64_t)r * kCensusBlock + tid;
            res[r] = i < P.n ? FQTK_STREAM_LOAD(&P.out[i]) : 0u;   // 0 = sample 0 matched: nothing to do
        }
        // the rows of ALL the tile's None reads are asked for before any is looked at: one memory latency per tile, not one per read
        bool keyed_r[kCensusR];
        uint32_t words[kCensusR][KW * 4];
#pragma unroll
        for (int r = 0; r < kCensusR; ++r) {
            const uint64_t i = t * tile + (uint64_t)r * kCensusBlock + tid;
            const bool none = (res[r] & 0xFFFFu) == kNoMatch;
            keyed_r[r] = none && rows_hold_a_barcode && (!P.lens || P.lens[i] == L);
#pragma unroll
            for (int w = 0; w < KW * 4; ++w) words[r][w] = 0u;
            if (keyed_r[r]) {
                uint32_t row[8];
                load_words<1, VEC, 8>(P, i, nwords, row);
#pragma unroll
                for (int w = 0; w < KW * 4; ++w)
                    if ((uint32_t)w < nwords) words[r][w] = row[w];
            }
        }
#pragma unroll
        for (int r = 0; r < kCensusR; ++r) {
            const bool none = (res[r] & 0xFFFFu) == kNoMatch;
            if (__ballot(none) == 0ull) continue;   // wave-uniform: the common case
            bool keyed = keyed_r[r];
            unsigned long long w0 = 0, w1 = 0;
            if (keyed) {
#pragma unroll
                for (int w = 0; w < KW * 4; ++w) {
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        const uint32_t k = (uint32_t)w * 4 + b;
                        if (k >= L) break;
                        const uint32_t x = lds_lut[(words[r][w] >> (8 * b)) & 0xFFu];   // plane bits in bytes 0..3
                        const unsigned long long nib = (x | (x >> 7) | (x >> 14) | (x >> 21)) & 0xFu;
                        keyed = keyed && nib != 0;   // a byte the reference's encode() gives 0: junk
                        if (w < 4) w0 |= nib << (4 * (k & 15u));
                        else w1 |= nib << (4 * (k & 15u));
                    }
                }
            }
            if (none && !keyed) ++my_unkeyed;
            const unsigned long long have = __ballot(keyed);
            if (have == 0ull) continue;
            uint32_t c = 1;
#ifndef FQTK_CENSUS_NO_COMBINE
            {   // fold the lanes that carry the first keyed lane's key into that lane
                const int lead = __ffsll((long long)have) - 1;
                const unsigned long long l0 = __shfl(w0, lead), l1 = __shfl(w1, lead);
                const bool same = keyed && w0 == l0 && w1 == l1;
                const unsigned long long group = __ballot(same);
                if (same) {
                    c = (uint32_t)__popcll(group);
                    keyed = (int)lane == lead;
                }
            }
#endif
            if (!keyed) continue;
            const uint64_t h = census_hash(w0, w1);
            const uint32_t b0 = (uint32_t)h & (SLOTS - 1u) & ~(kCensusBucket - 1u);
            const bool placed = census_bucket_add<KW>(&lds_key[0][b0], &lds_key[KW - 1][b0], 1u, w0, w1, [&](uint32_t j) { atomicAdd(&lds_cnt[b0 + j], c); });
            if (!placed && !census_global_add<KW>(C, h, w0, w1, c)) my_overflow += c;   // level 1: this key's bucket is full
        }
    }

    __syncthreads();   // every claim of this workgroup is complete: both words of a claimed slot are there
    for (uint32_t s = tid; s < SLOTS; s += kCensusBlock) {
        const unsigned long long k0 = lds_key[0][s];
        const uint32_t c = lds_cnt[s];
        if (k0 == 0ull || c == 0u) continue;
        const unsigned long long k1 = KW == 2 ? lds_key[KW - 1][s] : 0ull;
        if (!census_global_add<KW>(C, census_hash(k0, k1), k0, k1, c)) my_overflow += c;
    }
    if (my_unkeyed) atomicAdd(&lds_tot[0], my_unkeyed);
    if (my_overflow) atomicAdd(&lds_tot[1], my_overflow);
    __syncthreads();
    if (tid < 2 && lds_tot[tid]) atomicAdd(&C.tot[tid], lds_tot[tid]);
}

// Read-out: the non-empty slots, packed.  A wave appends its slots with ONE atomic (ballot, rank by mbcnt); entries are
// {word 0, word 1, count} whatever KW.  dense == nullptr only counts.  tot[2] += slots in use, tot[3] += sum of their counts.
__global__ __launch_bounds__(256) void census_compact_kernel(const unsigned long long *slots, uint64_t capacity, uint32_t kw,
                                                             unsigned long long *dense, unsigned long long *tot) {
    const uint64_t step = (uint64_t)gridDim.x * 256;
    const uint64_t rounds = (capacity + step - 1) / step;   // the same for every lane: the ballots below see whole waves
    const uint32_t lane = __lane_id();
    unsigned long long sum = 0;
    for (uint64_t r = 0; r < rounds; ++r) {
        const uint64_t s = r * step + (uint64_t)blockIdx.x * 256 + threadIdx.x;
        unsigned long long k0 = 0, k1 = 0, c = 0;
        if (s < capacity) {
            const unsigned long long *e = slots + s * (uint64_t)(kw + 1);
            k0 = e[0];
            if (k0) {
                k1 = kw == 2 ? e[1] : 0ull;
                c = e[kw];
            }
        }
        const bool have = k0 != 0ull;
        const unsigned long long b = __ballot(have);
        if (b == 0ull) continue;
        const int lead = __ffsll((long long)b) - 1;
        unsigned long long base = 0;
        if ((int)lane == lead) base = atomicAdd(&tot[2], (unsigned long long)__popcll(b));
        base = __shfl(base, lead);
        if (have) {
            sum += c;
            if (dense) {
                const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
                unsigned long long *d = dense + (base + rank) * 3ull;
                d[0] = k0;
                d[1] = k1;
                d[2] = c;
            }
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off);
    if (lane == 0 && sum) atomicAdd(&tot[3], sum);
}

// ---- host side: the state a fqtk_matcher owns and what its fqtk_matcher_census_* entry points do -----------------------
#define FQTK_CENSUS_TRY(expr)                                                                                   \
    do {                                                                                                        \
        hipError_t _e = (expr);                                                                                 \
        if (_e != hipSuccess) return internal::set_error(FQTK_EHIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

struct Census {
    unsigned long long *d_slots = nullptr;   // [capacity][kw + 1]
    unsigned long long *d_tot = nullptr;     // [0] unkeyed [1] overflow, [2] [3] scratch of the read-out
    uint64_t capacity = 0;
    uint32_t kw = 0;
    bool on() const { return d_slots != nullptr; }
};

struct CensusEntry { unsigned long long w0, w1, count; };

inline int census_disable(Census &c) {
    if (c.d_slots || c.d_tot) FQTK_CENSUS_TRY(hipDeviceSynchronize());   // a census kernel may still be running
    if (c.d_slots) FQTK_CENSUS_TRY(hipFree(c.d_slots));
    c.d_slots = nullptr;
    if (c.d_tot) FQTK_CENSUS_TRY(hipFree(c.d_tot));
    c.d_tot = nullptr;
    c.capacity = 0;
    return FQTK_OK;
}

inline int census_reset(Census &c) {
    if (!c.on()) return internal::set_error(FQTK_EINVAL, "census is not enabled");
    FQTK_CENSUS_TRY(hipDeviceSynchronize());
    FQTK_CENSUS_TRY(hipMemset(c.d_slots, 0, c.capacity * (c.kw + 1) * sizeof(unsigned long long)));
    FQTK_CENSUS_TRY(hipMemset(c.d_tot, 0, 4 * sizeof(unsigned long long)));
    FQTK_CENSUS_TRY(hipDeviceSynchronize());   // the batches run on non-blocking streams
    return FQTK_OK;
}

inline int census_enable(Census &c, uint32_t L, uint64_t capacity_slots) {
    if (L > kCensusMaxLen)
        return internal::set_error(FQTK_EINVAL, "the census keys barcodes of at most 32 bases; this table's have " + std::to_string(L));
    if (capacity_slots == 0) capacity_slots = 1ull << 20;
    if (capacity_slots > (1ull << 32)) return internal::set_error(FQTK_EINVAL, "census capacity above 2^32 slots");
    uint64_t cap = kCensusBucket;   // at least one bucket
    while (cap < capacity_slots) cap <<= 1;
    const uint32_t kw = L <= 16 ? 1u : 2u;
    if (c.on() && (cap != c.capacity || kw != c.kw)) {
        const int rc = census_disable(c);
        if (rc != FQTK_OK) return rc;
    }
    if (!c.on()) {
        c.kw = kw;
        if (hipMalloc(reinterpret_cast<void **>(&c.d_slots), cap * (kw + 1) * sizeof(unsigned long long)) != hipSuccess) {
            (void)hipGetLastError();
            c.d_slots = nullptr;
            return internal::set_error(FQTK_ENOMEM, "census: no device memory for " + std::to_string(cap) + " slots");
        }
        c.capacity = cap;
        if (!c.d_tot) FQTK_CENSUS_TRY(hipMalloc(reinterpret_cast<void **>(&c.d_tot), 4 * sizeof(unsigned long long)));
    }
    return census_reset(c);
}

// The end of a batch (fqtk_match.hip, launch()): P = the batch, its results final on `stream`.
inline int census_launch(const Census &c, const MatchParams &P, int num_cus, hipStream_t stream) {
    if (P.n == 0) return FQTK_OK;
    CensusParams C;
    C.m = P;
    C.slots = c.d_slots;
    C.mask = c.capacity - 1;
    C.tot = c.d_tot;
    const uint64_t tile = (uint64_t)kCensusBlock * kCensusR;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((P.n + tile - 1) / tile, (uint64_t)num_cus * 2);
    const bool dwords = P.stride % 4 == 0 && reinterpret_cast<uintptr_t>(P.obs) % 4 == 0 && P.stride >= ((P.L + 3) / 4) * 4;
    if (c.kw == 1) {
        if (dwords) hipLaunchKernelGGL((census_kernel<1, -1>), dim3(grid), dim3(kCensusBlock), 0, stream, C);
        else hipLaunchKernelGGL((census_kernel<1, 0>), dim3(grid), dim3(kCensusBlock), 0, stream, C);
    } else {
        if (dwords) hipLaunchKernelGGL((census_kernel<2, -1>), dim3(grid), dim3(kCensusBlock), 0, stream, C);
        else hipLaunchKernelGGL((census_kernel<2, 0>), dim3(grid), dim3(kCensusBlock), 0, stream, C);
    }
    FQTK_CENSUS_TRY(hipGetLastError());
    return FQTK_OK;
}

// Synchronises the device, then counts (entries == nullptr) or fetches the table's entries; tot4 = unkeyed, overflow, distinct, keyed.
inline int census_read(Census &c, std::vector<CensusEntry> *entries, unsigned long long (&tot4)[4]) {
    if (!c.on()) return internal::set_error(FQTK_EINVAL, "census is not enabled");
    FQTK_CENSUS_TRY(hipDeviceSynchronize());
    const uint32_t grid = (uint32_t)std::min<uint64_t>((c.capacity + 255) / 256, 2048);
    unsigned long long *d_dense = nullptr;
    for (int pass = 0; pass < (entries ? 2 : 1); ++pass) {   // count, then -- into room for exactly that many -- pack
        FQTK_CENSUS_TRY(hipMemset(c.d_tot + 2, 0, 2 * sizeof(unsigned long long)));
        hipLaunchKernelGGL(census_compact_kernel, dim3(grid), dim3(256), 0, nullptr, c.d_slots, c.capacity, c.kw, d_dense, c.d_tot);
        FQTK_CENSUS_TRY(hipGetLastError());
        FQTK_CENSUS_TRY(hipMemcpy(tot4, c.d_tot, sizeof(tot4), hipMemcpyDeviceToHost));
        if (pass == 0 && entries && tot4[2])
            FQTK_CENSUS_TRY(hipMalloc(reinterpret_cast<void **>(&d_dense), tot4[2] * sizeof(CensusEntry)));
        if (!d_dense) break;
    }
    if (entries) {
        entries->resize(d_dense ? tot4[2] : 0);
        hipError_t e = hipSuccess;
        if (d_dense) {
            e = hipMemcpy(entries->data(), d_dense, entries->size() * sizeof(CensusEntry), hipMemcpyDeviceToHost);
            (void)hipFree(d_dense);
        }
        FQTK_CENSUS_TRY(e);
    }
    return FQTK_OK;
}

inline int census_totals(Census &c, uint64_t *distinct, uint64_t *keyed, uint64_t *unkeyed, uint64_t *overflow) {
    unsigned long long t[4];
    const int rc = census_read(c, nullptr, t);
    if (rc != FQTK_OK) return rc;
    if (unkeyed) *unkeyed = t[0];
    if (overflow) *overflow = t[1];
    if (distinct) *distinct = t[2];
    if (keyed) *keyed = t[3];
    return FQTK_OK;
}

// The k most frequent barcodes: count descending, ties by the decoded string ascending (mod.rs:68 decode()).
inline int census_top(Census &c, uint32_t L, uint32_t k, char *barcodes, uint64_t *counts, uint32_t *n_out) {
    if (!n_out || (k && (!barcodes || !counts))) return internal::set_error(FQTK_EINVAL, "NULL argument");
    *n_out = 0;
    std::vector<CensusEntry> ents;
    unsigned long long t[4];
    const int rc = census_read(c, &ents, t);
    if (rc != FQTK_OK) return rc;
    static const char kDecode[17] = "?ACMGRSVTWYHKDBN";   // by mask: A1 C2 G4 T8 M3 R5 W9 S6 Y10 K12 V7 H11 D13 B14 N15
    std::vector<std::pair<std::string, uint64_t>> rows(ents.size());
    for (size_t i = 0; i < ents.size(); ++i) {
        rows[i].first.resize(L);
        for (uint32_t b = 0; b < L; ++b) rows[i].first[b] = kDecode[((b < 16 ? ents[i].w0 : ents[i].w1) >> (4 * (b & 15u))) & 0xFu];
        rows[i].second = ents[i].count;
    }
    const auto before = [](const std::pair<std::string, uint64_t> &a, const std::pair<std::string, uint64_t> &b) {
        return a.second != b.second ? a.second > b.second : a.first < b.first;
    };
    const size_t n = std::min<size_t>(k, rows.size());
    if (n < rows.size()) std::partial_sort(rows.begin(), rows.begin() + n, rows.end(), before);
    else std::sort(rows.begin(), rows.end(), before);
    for (size_t i = 0; i < n; ++i) {
        std::memcpy(barcodes + i * L, rows[i].first.data(), L);
        counts[i] = rows[i].second;
    }
    *n_out = (uint32_t)n;
    return FQTK_OK;
}

}  // namespace fqtk
