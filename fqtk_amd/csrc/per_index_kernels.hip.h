// per_index_kernels.hip.h -- per-index mismatch budgets as an assignment mode (include/fqtk_match.h, fqtk_matcher_set_per_index;
// DESIGN.md section 5.1h): index 1 and index 2 of a dual-index read are assigned each on its own, against the run's distinct
// values of that index and with its own (max_mismatches, min_mismatch_delta), and the template goes to the sample whose pair
// (index 1, index 2) it is -- the rule of bcl2fastq's --barcode-mismatches 1,1.
//
// per_index_kernel (gfx950), the form for plain A/C/G/T tables with budgets of at most one mismatch per index:
//   * TWO MEMOS IN ONE LDS IMAGE.  A whole-barcode memo of this acceptance set has U x (1 + 4 len_a) x (1 + 4 len_b) entries (384
//     x 33 x 33); the two per-index memos have U_A x (1 + 4 len_a) + U_B x (1 + 4 len_b) (2 x 384 x 33) and sit, with the index
//     keys, the pair directory and the per-sample histogram, in one CU's 160 KiB.  Image: [entries A | entries B | keys A | keys B
//     | row starts | rows | histogram].
//   * THE KEY IS CUT, NOT THE ROW.  A lane encodes its whole row once (memo_hash.hpp encode_word: 3 VALU per four bases) and
//     packs the codes into LINEAR nibbles, base i in nibble i & 7 of word i >> 3 (one v_lshr_or + one v_perm per four bases).
//     Index 1's key is the low len_a nibbles; index 2's is the nibble string funnel-shifted down by len_a: two v_alignbit_b32
//     by the wave-uniform 4 * (len_a & 7) over words picked by the wave-uniform len_a >> 3.  Any split of up to 16 + 16.
//   * ONE ROUND TRIP.  An entry is one dword [idx : 12 | best : 1 | next : 5 | nibble : 3 | word : 1 | xnib : 3 | fingerprint : 7]
//     describing a read index RELATIVE to the list entry it resolves to, three-choice cuckoo over any slot count.  The six
//     ds_read_b32 of the two probes are issued together; each candidate is verified against its entry's key (ds_read_b64):
//     key ^ index_key[idx] == xnib << 4 * nibble.  A miss proves "unassigned": every string within one mismatch of an entry
//     that the rule assigns is stored.
//   * DIRECTORY.  (a, b) -> sample through per-a rows of (b | s << 16) scanned under the table's longest row (wave-uniform; 1
//     for unique dual indexes).  A dense matrix of 384 x 384 16-bit cells would not fit; the rows of 384 pairs take 3 KiB.
//   * ODD BYTES.  Ambiguity codes and '.' get N's code where they stand (recode_flagged_bytes).  A byte of no IUPAC meaning
//     matches everything and is in no memo: the rare wave that holds one runs that lane's key, those nibbles masked out, over
//     the index keys already in LDS (wave-uniform addresses: broadcast reads) -- no list, no second launch.
// per_index_scan_kernel, for every other table (a sample base that is not A/C/G/T, a budget above one, an image over the LDS
// budget): one lane per read, the read's planes over the A entries and then the B entries through SGPRs (pair_kernels.hip.h
// pairs_scan), the directory read from L2.  Results never depend on which of the two served a batch.
#pragma once
#include <array>
#include <string>
#include <unordered_set>
#include <vector>

#include "lds_memo_kernels.hip.h"
#include "pair_kernels.hip.h"

namespace fqtk {

constexpr int kPiBlock = 1024;                 // 16 waves: one workgroup per CU when the image is large, two when it is small
constexpr int kPiR = 4;                        // reads per lane in flight
constexpr uint32_t kPiMaxIndexLen = 16;        // two key words per index
constexpr uint32_t kPiIdxBits = 12;            // an entry's idx field; idx == U (the sentinel key row) = empty / miss
constexpr uint32_t kPiFpMask = 0xFE000000u;
constexpr uint32_t kPiMaxRow = 16;             // the LDS form's longest directory row
constexpr uint32_t kPiNone = 0xFFFFFFFFu;

// idx | best << 12 | next5 << 13 (31 = 255: a list of one) | nibble << 18 | word << 21 | xnib << 22
FQTK_HD constexpr uint32_t pi_entry_fields(uint32_t idx, uint32_t best, uint32_t next, uint32_t xnib, uint32_t pos) {
    return idx | (best << 12) | ((next > 30u ? 31u : next) << 13) | ((pos & 7u) << 18) | ((pos >> 3) << 21) | (xnib << 22);
}
// the three slots (byte offsets inside the entry table) and the fingerprint of a key: memo_hash3's two mixed words
FQTK_HD inline void pi_hash(uint32_t k0, uint32_t k1, uint32_t salt, uint32_t nslots, uint32_t (&slot_b)[3], uint32_t &fp) {
    uint32_t h, g, h3, fps;
    memo_hash3(k0, k1, 0u, 0u, salt, h, g, h3, fps);
    slot_b[0] = lds_slot_any(h & 0xFFFFu, nslots);
    slot_b[1] = lds_slot_any(g & 0xFFFFu, nslots);
    slot_b[2] = lds_slot_any(h >> 16, nslots);
    fp = g << 9;   // g[16..22], which no slot reads
}

// The two pieces of arithmetic the kernel, the planner and the planner's self-check share.
// pi_key_diff: 0 iff key (k0, k1) is the list entry's key (s0, s1) with the nibble the entry word `e` names replaced as it says.
FQTK_HD inline uint32_t pi_key_diff(uint32_t e, uint32_t k0, uint32_t k1, uint32_t s0, uint32_t s1) {
    const uint32_t tsh = ((e >> 22) & 7u) << ((e >> 16) & 28u);   // the differing nibble, in its word
    const bool w1 = (e & (1u << 21)) != 0;
    return (k0 ^ s0 ^ (w1 ? 0u : tsh)) | (k1 ^ s1 ^ (w1 ? tsh : 0u));
}
// pi_nibble_mismatches: the nonzero nibbles of the XOR of two key words (codes are at most 7: three bits a nibble).
FQTK_HD inline uint32_t pi_nibble_mismatches(uint32_t d) { return (uint32_t)__builtin_popcount((d | (d >> 1) | (d >> 2)) & 0x11111111u); }

struct PerIndexParams {
    MatchParams m;
    const uint32_t *image;
    uint32_t image_words;
    uint32_t tab_b[2], nslots[2], salt[2], keys_b[2], u[2];   // per index: entry table (byte offset), slots, salt, keys, list size
    uint32_t dir_b, rows_b, max_row;                          // row starts [u_a + 2], rows (b | s << 16), the longest row
    uint32_t q8, sh;                                          // len_a >> 3, 4 * (len_a & 7)
    uint32_t mask[2][2];                                      // nibble masks of the two keys' words
    uint32_t mm[2], delta[2];
    uint32_t hist_shift;                                      // 1 << hist_shift copies of every bin (lane & mask picks one)
};

struct PiProbe { uint32_t e[3], fp; };
__device__ __forceinline__ PiProbe pi_probe(uint32_t k0, uint32_t k1, uint32_t tab_b, uint32_t nslots, uint32_t salt) {
    uint32_t a[3];
    PiProbe p;
    pi_hash(k0, k1, salt, nslots, a, p.fp);
#pragma unroll
    for (int c = 0; c < 3; ++c) p.e[c] = lds_word(tab_b + a[c]);
    return p;
}
__device__ __forceinline__ uint32_t pi_verify(uint32_t e, uint32_t k0, uint32_t k1, uint32_t keys_b, uint32_t miss) {
    const u32x2v sk = *reinterpret_cast<lds_u2 *>((uintptr_t)(keys_b + (e & ((1u << kPiIdxBits) - 1u)) * 8u));
    return pi_key_diff(e, k0, k1, sk.x, sk.y) == 0 ? e : miss;
}
// the first candidate whose fingerprint agrees is verified; the later ones only in the rare wave where two agree.  The fingerprint is
// a hint for the order only: pi_verify alone decides, so when none agrees e[2] is verified anyway and fails (the sentinel key row is
// all ones, and no key built of nibbles <= 7 equals it)
__device__ __forceinline__ uint32_t pi_pick(const PiProbe &p, uint32_t k0, uint32_t k1, uint32_t keys_b, uint32_t miss) {
    const bool m1 = ((p.e[0] ^ p.fp) & kPiFpMask) == 0, m2 = ((p.e[1] ^ p.fp) & kPiFpMask) == 0, m3 = ((p.e[2] ^ p.fp) & kPiFpMask) == 0;
    uint32_t v = pi_verify(m1 ? p.e[0] : (m2 ? p.e[1] : p.e[2]), k0, k1, keys_b, miss);
    const bool several = (m1 && (m2 || m3)) || (m2 && m3);
    if (__ballot(several)) {   // wave-uniform
        const uint32_t v2 = pi_verify((m1 && m2) ? p.e[1] : p.e[2], k0, k1, keys_b, miss);
        const bool need2 = several && v == miss;
        if (need2) v = v2;
        const uint32_t v3 = pi_verify(p.e[2], k0, k1, keys_b, miss);
        if (need2 && v2 == miss && m1 && m2 && m3) v = v3;
    }
    return v;
}
// A key with wildcard nibbles (w0, w1: 0xF where the read's byte has no IUPAC meaning) over the U keys of one index: the rule
// itself, best / next / lowest entry, as an entry word or `miss`.  Wave-uniform addresses; the LDS form has mm <= 1.
__device__ __forceinline__ uint32_t pi_scan_keys(uint32_t k0, uint32_t k1, uint32_t w0, uint32_t w1, uint32_t keys_b, uint32_t U,
                                                 uint32_t mm_i, uint32_t delta_i, uint32_t miss) {
    uint32_t best = kKeyInit, second = kKeyInit;
    for (uint32_t u = 0; u < U; ++u) {
        const u32x2v sk = *reinterpret_cast<lds_u2 *>((uintptr_t)(keys_b + u * 8u));
        const uint32_t d0 = (k0 ^ sk.x) & ~w0, d1 = (k1 ^ sk.y) & ~w1;
        const uint32_t key = ((pi_nibble_mismatches(d0) + pi_nibble_mismatches(d1)) << 16) | u;
        second = med3_u32(best, second, key);
        best = min(best, key);
    }
    const uint32_t bm = best >> 16, nm = second >> 16;
    return (bm > mm_i || (nm - bm) < delta_i) ? miss : pi_entry_fields(best & 0xFFFFu, bm, nm, 0u, 0u);
}

// NWD: dwords of a row that hold barcode (ceil(L / 4); 8 on the byte path, absent words read as nothing).
// DWORDS: rows are whole dwords (base and stride 4-aligned, stride >= 4 * NWD); else bytes (load_words).
template <int NWD, bool DWORDS>
__global__ __launch_bounds__(kPiBlock) void per_index_kernel(const PerIndexParams Q) {
    const MatchParams &P = Q.m;
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    constexpr int KWT = (NWD + 1) / 2;   // nibble words of the whole barcode
    const uint32_t tid = threadIdx.x;
    for (uint32_t w = tid; w < Q.image_words; w += kPiBlock) smem[w] = Q.image[w];
    uint32_t *lds_hist = smem + Q.image_words;
    const uint32_t bins = P.S + 1;
    const uint32_t hist_words = bins << Q.hist_shift;
    if (P.counts)
        for (uint32_t b = tid; b < hist_words; b += kPiBlock) lds_hist[b] = 0;
    __syncthreads();

    const uint32_t base_b = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t *)smem;
    const uint32_t tab_a = base_b + Q.tab_b[0], tab_bb = base_b + Q.tab_b[1];
    const uint32_t keys_a = base_b + Q.keys_b[0], keys_bb = base_b + Q.keys_b[1];
    const uint32_t dir_b = base_b + Q.dir_b, rows_b = base_b + Q.rows_b;
    const uint32_t hist_b = base_b + (Q.image_words << 2) + ((tid & ((1u << Q.hist_shift) - 1u)) << 2);
    const uint32_t hist_bin_shift = Q.hist_shift + 2u;
    const uint32_t L = P.L;
    const uint32_t nwords = (L + 3u) >> 2;
    uint32_t kc[NWD], kv[NWD];   // encode_word's masks cut down to the row's real bases
#pragma unroll
    for (int w = 0; w < NWD; ++w) {
        const int rem = (int)L - 4 * w;
        const uint32_t keep = rem >= 4 ? 0xFFFFFFFFu : (rem <= 0 ? 0u : ((1u << (8 * rem)) - 1u));
        kc[w] = keep & 0x07070707u;
        kv[w] = keep & 0xDFDFDFDFu;
    }
    // four codes (or 0x0F flags), one per byte -> four nibbles; two such words -> one linear key word
    const auto pack8 = [](uint32_t lo4, uint32_t hi4) {
        const uint32_t t0 = lo4 | (lo4 >> 4), t1 = hi4 | (hi4 >> 4);
        return __builtin_amdgcn_perm(t1, t0, 0x06040200u);
    };
    // the whole barcode's nibble words -> the two indexes' keys (ka, kb)
    const auto cut = [&](const uint32_t (&n)[4], uint32_t (&ka)[2], uint32_t (&kb)[2]) {
        ka[0] = n[0] & Q.mask[0][0];
        ka[1] = n[1] & Q.mask[0][1];
        const uint32_t lo0 = Q.q8 == 0 ? n[0] : (Q.q8 == 1 ? n[1] : n[2]);
        const uint32_t hi0 = Q.q8 == 0 ? n[1] : (Q.q8 == 1 ? n[2] : n[3]);
        const uint32_t hi1 = Q.q8 == 0 ? n[2] : (Q.q8 == 1 ? n[3] : 0u);
        kb[0] = __builtin_amdgcn_alignbit(hi0, lo0, Q.sh) & Q.mask[1][0];
        kb[1] = __builtin_amdgcn_alignbit(hi1, hi0, Q.sh) & Q.mask[1][1];
    };

    const uint64_t tile = (uint64_t)kPiBlock * kPiR;
    const uint64_t ntiles = (P.n + tile - 1) / tile;
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        uint32_t words[kPiR][NWD], res[kPiR];
        bool live[kPiR];
        // wave-contiguous: a wave's kPiR loads cover kPiR x 64 consecutive reads (lds_memo_kernels.hip.h)
#pragma unroll
        for (int r = 0; r < kPiR; ++r) {
            const uint64_t i = t * tile + (tid >> 6) * (64u * kPiR) + (uint32_t)r * 64u + (tid & 63u);
            live[r] = i < P.n;
#pragma unroll
            for (int w = 0; w < NWD; ++w) words[r][w] = 0x41414141u;   // dead lanes look like "AAAA"
            if (live[r]) {
                if constexpr (DWORDS) {
                    const uint32_t *src = reinterpret_cast<const uint32_t *>(P.obs + i * (uint64_t)P.stride);
#pragma unroll
                    for (int w = 0; w < NWD; ++w) words[r][w] = FQTK_STREAM_LOAD(src + w);
                } else {
                    load_words<1, 0, NWD>(P, i, nwords, words[r]);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < kPiR; ++r) {
            // ---- ASCII -> codes; odd bytes recoded where they stand, bytes of no IUPAC meaning left as wildcard nibbles
            uint32_t c[8] = {0, 0, 0, 0, 0, 0, 0, 0}, bad = 0;
#pragma unroll
            for (int w = 0; w < NWD; ++w) {
                uint32_t x;
                encode_word(words[r][w], kc[w], kv[w], c[w], x);
                bad |= x;
            }
            uint32_t wild[4] = {0, 0, 0, 0};
            if (__builtin_amdgcn_uicmp(bad, 0u, 33 /* ne */)) {   // wave-uniform
                uint32_t f[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
                for (int w = 0; w < NWD; ++w) {
                    uint32_t x = flagged_bytes_of_word(words[r][w], c[w], kv[w]);
                    if (__builtin_amdgcn_uicmp(x, 0u, 33)) x = recode_flagged_bytes(words[r][w], x, c[w], kc[w]);
                    f[w] = ((x >> 7) & 0x01010101u) * 15u;
                }
#pragma unroll
                for (int k = 0; k < KWT; ++k) wild[k] = pack8(f[2 * k], f[2 * k + 1]);
            }
            uint32_t n[4] = {0, 0, 0, 0}, ka[2], kb[2];
#pragma unroll
            for (int k = 0; k < KWT; ++k) n[k] = pack8(c[2 * k], c[2 * k + 1]);
            cut(n, ka, kb);
            // ---- both probes, then one wait
            const PiProbe pa = pi_probe(ka[0], ka[1], tab_a, Q.nslots[0], Q.salt[0]);
            const PiProbe pb = pi_probe(kb[0], kb[1], tab_bb, Q.nslots[1], Q.salt[1]);
            uint32_t va = pi_pick(pa, ka[0], ka[1], keys_a, Q.u[0]);
            uint32_t vb = pi_pick(pb, kb[0], kb[1], keys_bb, Q.u[1]);
            if (__builtin_amdgcn_uicmp(wild[0] | wild[1] | wild[2] | wild[3], 0u, 33)) {   // wave-uniform, rare
                uint32_t wa[2], wb[2];
                cut(wild, wa, wb);
                const uint32_t sa = pi_scan_keys(ka[0], ka[1], wa[0], wa[1], keys_a, Q.u[0], Q.mm[0], Q.delta[0], Q.u[0]);
                const uint32_t sb = pi_scan_keys(kb[0], kb[1], wb[0], wb[1], keys_bb, Q.u[1], Q.mm[1], Q.delta[1], Q.u[1]);
                if (wa[0] | wa[1]) va = sa;
                if (wb[0] | wb[1]) vb = sb;
            }
            // ---- (a, b) -> sample: row a of the directory
            const uint32_t a = va & ((1u << kPiIdxBits) - 1u), b = vb & ((1u << kPiIdxBits) - 1u);
            const uint32_t start = lds_word(dir_b + a * 4u), end = lds_word(dir_b + a * 4u + 4u);
            uint32_t s = kNoMatch;
            for (uint32_t j = 0; j < Q.max_row; ++j) {   // wave-uniform bound
                const uint32_t p = start + j;
                const uint32_t e = lds_word(rows_b + (p < end ? p : end) * 4u);   // (the rows end in one pad word)
                if (p < end && (e & 0xFFFFu) == b) s = e >> 16;
            }
            const uint32_t ba = (va >> 12) & 1u, bb = (vb >> 12) & 1u;
            const uint32_t na5 = (va >> 13) & 31u, nb5 = (vb >> 13) & 31u;
            const uint32_t na = na5 == 31u ? 255u : na5, nb = nb5 == 31u ? 255u : nb5;
            const uint32_t next = min(255u, min(na + bb, ba + nb));
            res[r] = s == kNoMatch ? kPiNone : (s | ((ba + bb) << 16) | (next << 24));
        }
#pragma unroll
        for (int r = 0; r < kPiR; ++r) {
            if (!live[r]) continue;
            const uint64_t i = t * tile + (tid >> 6) * (64u * kPiR) + (uint32_t)r * 64u + (tid & 63u);
            FQTK_STREAM_STORE(res[r], &P.out[i]);
            if (P.counts) lds_atomic_inc(hist_b + (min(res[r] & 0xFFFFu, P.S) << hist_bin_shift));
        }
    }
    if (P.counts) {
        __syncthreads();
        for (uint32_t b = tid; b < bins; b += kPiBlock) {
            uint32_t cnt = 0;
            for (uint32_t k = 0; k < (1u << Q.hist_shift); ++k) cnt += lds_hist[(b << Q.hist_shift) + k];
            if (cnt) atomicAdd(&P.counts[b], (unsigned long long)cnt);
        }
    }
}

// ---- the scan path ------------------------------------------------------------------------------------------------------
struct PerIndexScanParams {
    MatchParams m;
    const uint32_t *tab;     // [u_a + u_b][4] pre-inverted planes (pairs_plane_table)
    const uint32_t *dir;     // row starts [u_a + 2], then the rows (b | s << 16)
    uint32_t u[2], mm[2], delta[2];
};

// VEC as in pairs_kernel: -1 = rows are whole dwords, 0 = bytes.
template <int VEC>
__global__ __launch_bounds__(kBlock) void per_index_scan_kernel(const PerIndexScanParams C) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    uint32_t *lds_lut = smem, *lds_hist = smem + 256;
    const MatchParams &P = C.m;
    const uint32_t tid = threadIdx.x;
    lds_lut[tid] = P.lut[tid];
    const uint32_t bins = P.S + 1;
    if (P.counts && P.lds_hist)
        for (uint32_t b = tid; b < bins; b += kBlock) lds_hist[b] = 0;
    __syncthreads();
    const uint32_t nwords = (P.L + 3u) >> 2;
    const const_u32x4_ptr tab_a = (const_u32x4_ptr)(uintptr_t)C.tab;
    const const_u32x4_ptr tab_b = tab_a + C.u[0];
    const uint32_t *rows = C.dir + C.u[0] + 2u;
    const uint64_t ntiles = (P.n + kBlock - 1) / kBlock;
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint64_t i = t * kBlock + tid;
        const bool live = i < P.n;
        uint32_t row[8];
#pragma unroll
        for (int w = 0; w < 8; ++w) row[w] = 0u;
        if (live) load_words<1, VEC, 8>(P, i, nwords, row);
        Planes<1> o;
        encode_planes<1>(row, nwords, P.L, lds_lut, o);
        uint32_t best[2], second[2];
        pairs_scan(tab_a, C.u[0], o, best[0], second[0]);
        pairs_scan(tab_b, C.u[1], o, best[1], second[1]);
        if (!live) continue;
        uint32_t bm[2], nm[2];
        bool assigned = true;
#pragma unroll
        for (int w = 0; w < 2; ++w) {
            bm[w] = best[w] >> 16;
            nm[w] = second[w] >> 16;   // a list of one: second stays at its initial 255
            assigned = assigned && bm[w] <= C.mm[w] && (nm[w] - bm[w]) >= C.delta[w];
        }
        uint32_t s = kNoMatch;
        if (assigned) {
            const uint32_t a = best[0] & 0xFFFFu, b = best[1] & 0xFFFFu;
            for (uint32_t p = C.dir[a], end = C.dir[a + 1]; p < end; ++p) {
                const uint32_t e = rows[p];
                if ((e & 0xFFFFu) == b) s = e >> 16;
            }
        }
        const uint32_t next = min(255u, min(nm[0] + bm[1], bm[0] + nm[1]));
        FQTK_STREAM_STORE(s == kNoMatch ? kPiNone : (s | ((bm[0] + bm[1]) << 16) | (next << 24)), &P.out[i]);
        if (P.counts) {
            const uint32_t bin = min(s, P.S);
            if (P.lds_hist) atomicAdd(&lds_hist[bin], 1u);
            else atomicAdd(&P.counts[bin], 1ull);
        }
    }
    if (P.counts && P.lds_hist) {
        __syncthreads();
        for (uint32_t b = tid; b < bins; b += kBlock) {
            const uint32_t c = lds_hist[b];
            if (c) atomicAdd(&P.counts[b], (unsigned long long)c);
        }
    }
}

// ---- host side: the plan of the LDS image and the state a fqtk_matcher owns ----------------------------------------------
struct PiEntry { uint32_t k[2], fields; };

// The keys of one index list and every entry of its memo: each list entry with at most one base replaced by another base or N,
// judged by the rule against the whole list; only the strings the rule assigns are kept.  false: a base that is not A/C/G/T.
inline bool pi_index_entries(const std::vector<std::string> &list, uint32_t mm_i, uint32_t delta_i, std::vector<std::array<uint32_t, 2>> &keys,
                             std::vector<PiEntry> &ents) {
    keys.clear();
    ents.clear();
    for (const std::string &s : list) {
        std::array<uint32_t, 2> k = {0u, 0u};
        for (size_t i = 0; i < s.size(); ++i) {
            if (s[i] != 'A' && s[i] != 'C' && s[i] != 'G' && s[i] != 'T') return false;
            k[i >> 3] |= memo_code_of(s[i]) << (4 * (i & 7));
        }
        keys.push_back(k);
    }
    std::unordered_set<uint64_t> seen;
    const auto judge = [&](uint32_t c0, uint32_t c1) {
        if (!seen.insert(((uint64_t)c1 << 32) | c0).second) return;
        uint32_t best = kKeyInit, second = kKeyInit;
        for (size_t u = 0; u < keys.size(); ++u) {
            const uint32_t mm = pi_nibble_mismatches(c0 ^ keys[u][0]) + pi_nibble_mismatches(c1 ^ keys[u][1]);
            const uint32_t key = (mm << 16) | (uint32_t)u;
            if (key < best) { second = best; best = key; }
            else if (key < second) second = key;
        }
        const uint32_t bm = best >> 16, nm = second >> 16, idx = best & 0xFFFFu;
        if (bm > mm_i || bm > 1u || (nm - bm) < delta_i) return;
        uint32_t pos = 0, xnib = 0;
        for (uint32_t b = 0; b < 16; ++b) {
            const uint32_t x = (((b >> 3) ? c1 : c0) ^ keys[idx][b >> 3]) >> (4 * (b & 7)) & 0xFu;
            if (x) { pos = b; xnib = x; }
        }
        ents.push_back(PiEntry{{c0, c1}, pi_entry_fields(idx, bm, nm, xnib, pos)});
    };
    static const uint32_t codes[5] = {0u, 1u, 2u, 3u, 7u};
    for (size_t u = 0; u < keys.size(); ++u) {
        judge(keys[u][0], keys[u][1]);
        for (uint32_t b = 0; b < list[u].size(); ++b)
            for (uint32_t code : codes) {
                std::array<uint32_t, 2> c = keys[u];
                c[b >> 3] = (c[b >> 3] & ~(0xFu << (4 * (b & 7)))) | (code << (4 * (b & 7)));
                judge(c[0], c[1]);
            }
    }
    return true;
}

// The kernel's look-up of one index on the host (the planner's self-check): the entry word, or U.
inline uint32_t pi_lookup_host(const uint32_t *tab, uint32_t nslots, uint32_t salt, const uint32_t *keys, uint32_t U, uint32_t k0, uint32_t k1) {
    uint32_t a[3], fp;
    pi_hash(k0, k1, salt, nslots, a, fp);
    for (int c = 0; c < 3; ++c) {
        const uint32_t e = tab[a[c] >> 2];
        if ((e ^ fp) & kPiFpMask) continue;
        const uint32_t idx = e & ((1u << kPiIdxBits) - 1u);
        if (pi_key_diff(e, k0, k1, keys[2 * idx], keys[2 * idx + 1]) == 0) return e;
    }
    return U;
}

// Three-choice cuckoo placement (random-walk eviction) of the entries into nslots slots; empty slots read `U`.
inline bool pi_place(const std::vector<PiEntry> &ents, uint32_t nslots, uint32_t U, const uint32_t *keys, std::vector<uint32_t> &tab, uint32_t &salt_out) {
    std::vector<int64_t> owner;
    for (uint32_t attempt = 1; attempt <= 12; ++attempt) {
        const uint32_t salt = 0x51ED27u * attempt;
        owner.assign(nslots, -1);
        uint64_t rng = 0x9E3779B97F4A7C15ull ^ salt;
        const auto slot_of = [&](int64_t i, int c) {
            uint32_t a[3], fp;
            pi_hash(ents[(size_t)i].k[0], ents[(size_t)i].k[1], salt, nslots, a, fp);
            return a[c] >> 2;
        };
        bool ok = true;
        for (size_t i = 0; i < ents.size() && ok; ++i) {
            int64_t cur = (int64_t)i, avoid = -1;
            ok = false;
            for (int kick = 0; kick < 5000 && !ok; ++kick) {
                for (int c = 0; c < 3 && !ok; ++c) {
                    const uint32_t p = slot_of(cur, c);
                    if (owner[p] < 0) { owner[p] = cur; ok = true; }
                }
                if (ok) break;
                uint32_t p = 0;
                int tries = 0;
                do {
                    rng = rng * 6364136223846793005ull + 1442695040888963407ull;
                    p = slot_of(cur, (int)((rng >> 33) % 3u));
                } while ((int64_t)p == avoid && ++tries < 8);
                std::swap(cur, owner[p]);
                avoid = p;
            }
        }
        if (!ok) continue;
        tab.assign(nslots, U);
        for (uint32_t p = 0; p < nslots; ++p)
            if (owner[p] >= 0) {
                uint32_t a[3], fp;
                const PiEntry &e = ents[(size_t)owner[p]];
                pi_hash(e.k[0], e.k[1], salt, nslots, a, fp);
                tab[p] = e.fields | (fp & kPiFpMask);
            }
        bool good = true;
        for (size_t i = 0; i < ents.size() && good; ++i)
            good = (pi_lookup_host(tab.data(), nslots, salt, keys, U, ents[i].k[0], ents[i].k[1]) & ~kPiFpMask) == ents[i].fields;
        if (good) { salt_out = salt; return true; }
    }
    return false;
}

struct PerIndex {
    bool on = false;
    uint32_t len_a = 0, mm[2] = {0, 0}, delta[2] = {0, 0};
    std::vector<std::string> index[2];
    uint32_t *d_tab = nullptr;      // the scan path's planes
    uint32_t *d_dir = nullptr;      // the scan path's directory
    uint32_t *d_image = nullptr;    // the LDS form's image; nullptr: the scan path serves
    PerIndexParams q{};
    size_t lds_bytes = 0;           // image + histogram
    uint64_t entries = 0;           // both memos
    bool pin_scan = false;
    bool lds_form() const { return d_image != nullptr && !pin_scan; }
};

inline int per_index_off(PerIndex &p) {
    if (p.d_tab || p.d_dir || p.d_image) FQTK_PAIRS_TRY(hipDeviceSynchronize());
    if (p.d_tab) FQTK_PAIRS_TRY(hipFree(p.d_tab));
    if (p.d_dir) FQTK_PAIRS_TRY(hipFree(p.d_dir));
    if (p.d_image) FQTK_PAIRS_TRY(hipFree(p.d_image));
    p.d_tab = p.d_dir = p.d_image = nullptr;
    p.on = false;
    return FQTK_OK;
}

// The LDS image, when the table and the budgets are of its shape and it fits `budget` bytes beside the histogram.
inline bool per_index_plan(const std::vector<std::string> (&index)[2], const std::vector<uint32_t> &dir, uint32_t max_row, uint32_t S, uint32_t len_a,
                           uint32_t L, const uint32_t (&mm)[2], const uint32_t (&delta)[2], size_t budget, PerIndexParams &q, std::vector<uint32_t> &image,
                           size_t &lds_bytes, uint64_t &entries) {
    const uint32_t len[2] = {len_a, L - len_a};
    if (mm[0] > 1 || mm[1] > 1 || max_row > kPiMaxRow || S + 1 > kMaxLdsHist) return false;
    uint64_t cand = 0;
    for (int w = 0; w < 2; ++w) {
        if (index[w].size() + 1 >= (1u << kPiIdxBits)) return false;
        cand += (uint64_t)index[w].size() * (1 + 4 * len[w]);
    }
    if (cand * 4 > budget) return false;   // (before anything is enumerated)
    std::vector<std::array<uint32_t, 2>> keys[2];
    std::vector<PiEntry> ents[2];
    for (int w = 0; w < 2; ++w)
        if (!pi_index_entries(index[w], mm[w], delta[w], keys[w], ents[w])) return false;
    uint32_t hist_shift = 0;
    while (hist_shift < 5 && ((S + 1) << (hist_shift + 1)) <= 2048u) ++hist_shift;
    const size_t hist_bytes = ((size_t)(S + 1) << hist_shift) * 4;
    const size_t fixed = (keys[0].size() + keys[1].size() + 2) * 8 + (dir.size() + 1) * 4 + hist_bytes;
    if (fixed + 1024 > budget) return false;
    // slots: load 0.80 where there is room, whatever fits otherwise, down to load 0.88
    uint32_t nslots[2];
    const size_t total = ents[0].size() + ents[1].size();
    const size_t room = (budget - fixed) / 4;
    for (int w = 0; w < 2; ++w) {
        size_t want = std::max<size_t>(64, (ents[w].size() * 5 + 3) / 4);
        if ((total * 5 + 3) / 4 + 128 > room) want = std::max<size_t>(64, (size_t)((double)room * ((double)ents[w].size() + 32) / ((double)total + 64)));
        nslots[w] = (uint32_t)std::min<size_t>(want, 65534) & ~1u;
        if ((double)nslots[w] * 0.88 < (double)ents[w].size()) return false;
    }
    if (((size_t)nslots[0] + nslots[1]) * 4 + fixed > budget) return false;
    image.clear();
    for (int w = 0; w < 2; ++w) {
        std::vector<uint32_t> flat;
        for (const auto &k : keys[w]) { flat.push_back(k[0]); flat.push_back(k[1]); }
        flat.push_back(0xFFFFFFFFu);   // row U = "no entry": equals no key
        flat.push_back(0xFFFFFFFFu);
        std::vector<uint32_t> tab;
        if (!pi_place(ents[w], nslots[w], (uint32_t)keys[w].size(), flat.data(), tab, q.salt[w])) return false;
        q.tab_b[w] = (uint32_t)image.size() * 4;
        q.nslots[w] = nslots[w];
        q.u[w] = (uint32_t)keys[w].size();
        image.insert(image.end(), tab.begin(), tab.end());
        keys[w].clear();
        for (size_t i = 0; i < flat.size(); i += 2) keys[w].push_back({flat[i], flat[i + 1]});
    }
    for (int w = 0; w < 2; ++w) {
        q.keys_b[w] = (uint32_t)image.size() * 4;   // both tables have an even slot count: 8-byte aligned
        for (const auto &k : keys[w]) { image.push_back(k[0]); image.push_back(k[1]); }
    }
    q.dir_b = (uint32_t)image.size() * 4;
    q.rows_b = q.dir_b + (q.u[0] + 2) * 4;
    image.insert(image.end(), dir.begin(), dir.end());
    image.push_back(0xFFFFFFFFu);   // the pad word behind the last row
    q.image_words = (uint32_t)image.size();
    q.max_row = max_row;
    q.q8 = len_a >> 3;
    q.sh = 4 * (len_a & 7);
    for (int w = 0; w < 2; ++w)
        for (uint32_t k = 0; k < 2; ++k) {
            const int rem = (int)len[w] - 8 * (int)k;
            q.mask[w][k] = rem >= 8 ? 0xFFFFFFFFu : (rem <= 0 ? 0u : ((1u << (4 * rem)) - 1u));
        }
    q.hist_shift = hist_shift;
    lds_bytes = image.size() * 4 + hist_bytes;
    entries = total;
    return lds_bytes <= budget;
}

// barcodes = the table as the matcher keeps it (upper case), enc = the reference's encode() of one byte.
inline int per_index_set(PerIndex &p, const std::vector<std::string> &barcodes, uint32_t L, uint32_t len_a, const uint32_t (&mm)[2],
                         const uint32_t (&delta)[2], uint8_t (*enc)(uint8_t), size_t lds_budget) {
    if (L > kPairsMaxLen)
        return internal::set_error(FQTK_EINVAL, "per-index assignment takes barcodes of at most 32 bases; this table's have " + std::to_string(L));
    if (len_a == 0 || len_a >= L)
        return internal::set_error(FQTK_EINVAL, "the split point len_a must leave both indexes a base: 1 <= len_a < " + std::to_string(L) +
                                                    ", got " + std::to_string(len_a));
    if (len_a > kPiMaxIndexLen || L - len_a > kPiMaxIndexLen)
        return internal::set_error(FQTK_EINVAL, "per-index assignment takes indexes of at most 16 bases; these have " + std::to_string(len_a) + " + " +
                                                    std::to_string(L - len_a));
    std::vector<std::string> index[2];
    pairs_split_indexes(barcodes, len_a, index);
    // the directory: row a = the (b, s) of every sample whose index 1 is entry a, the lowest s of a pair only
    std::vector<std::vector<uint32_t>> rows(index[0].size());
    for (size_t s = 0; s < barcodes.size(); ++s) {
        const size_t a = std::find(index[0].begin(), index[0].end(), barcodes[s].substr(0, len_a)) - index[0].begin();
        const uint32_t b = (uint32_t)(std::find(index[1].begin(), index[1].end(), barcodes[s].substr(len_a)) - index[1].begin());
        bool have = false;
        for (uint32_t e : rows[a]) have = have || (e & 0xFFFFu) == b;
        if (!have) rows[a].push_back(b | ((uint32_t)s << 16));
    }
    std::vector<uint32_t> dir;
    uint32_t at = 0, max_row = 0;
    for (const auto &r : rows) { dir.push_back(at); at += (uint32_t)r.size(); max_row = std::max(max_row, (uint32_t)r.size()); }
    dir.push_back(at);   // row u_a ("index 1 unassigned") is empty
    dir.push_back(at);
    for (const auto &r : rows) dir.insert(dir.end(), r.begin(), r.end());
    const int rc = per_index_off(p);
    if (rc != FQTK_OK) return rc;
    const std::vector<uint32_t> tab = pairs_plane_table(index, len_a, enc);
    std::vector<uint32_t> image;
    PerIndexParams q{};
    size_t lds_bytes = 0;
    uint64_t entries = 0;
    const bool lds = per_index_plan(index, dir, max_row, (uint32_t)barcodes.size(), len_a, L, mm, delta, lds_budget, q, image, lds_bytes, entries);
    const auto upload = [](uint32_t *&d, const std::vector<uint32_t> &v) {
        if (hipMalloc(reinterpret_cast<void **>(&d), v.size() * sizeof(uint32_t)) != hipSuccess) { (void)hipGetLastError(); d = nullptr; return false; }
        return hipMemcpy(d, v.data(), v.size() * sizeof(uint32_t), hipMemcpyHostToDevice) == hipSuccess;
    };
    if (!upload(p.d_tab, tab) || !upload(p.d_dir, dir) || (lds && !upload(p.d_image, image))) {
        (void)per_index_off(p);
        return internal::set_error(FQTK_ENOMEM, "per-index assignment: no device memory for the index tables");
    }
    p.index[0] = std::move(index[0]);
    p.index[1] = std::move(index[1]);
    p.len_a = len_a;
    for (int w = 0; w < 2; ++w) { p.mm[w] = mm[w]; p.delta[w] = delta[w]; }
    p.q = q;
    p.q.image = p.d_image;
    p.lds_bytes = lds ? lds_bytes : 0;
    p.entries = lds ? entries : 0;
    p.on = true;
    return FQTK_OK;
}

template <int NWD, bool DWORDS>
inline int per_index_launch_t(const PerIndex &p, const PerIndexParams &Q, int num_cus, hipStream_t stream, std::vector<const void *> &big_lds_ok) {
    auto kern = per_index_kernel<NWD, DWORDS>;
    const void *fn = reinterpret_cast<const void *>(kern);
    if (p.lds_bytes > 64 * 1024 && std::find(big_lds_ok.begin(), big_lds_ok.end(), fn) == big_lds_ok.end()) {
        FQTK_PAIRS_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMemoMaxBytes));
        big_lds_ok.push_back(fn);
    }
    const uint64_t tile = (uint64_t)kPiBlock * kPiR;
    const uint64_t ntiles = (Q.m.n + tile - 1) / tile;
    const uint64_t per_cu = p.lds_bytes * 2 <= kLdsMemoMaxBytes ? 2 : 1;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(ntiles, (uint64_t)num_cus * per_cu);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(kPiBlock), p.lds_bytes, stream, Q);
    FQTK_PAIRS_TRY(hipGetLastError());
    return FQTK_OK;
}

// One batch (P.lens is NULL, P.stride >= P.L): the LDS form where it was planned, else the scan.
inline int per_index_launch(const PerIndex &p, const MatchParams &P, int num_cus, hipStream_t stream, std::vector<const void *> &big_lds_ok) {
    if (P.n == 0) return FQTK_OK;
    const uint32_t nwords = (P.L + 3) / 4;
    const bool dwords = P.stride % 4 == 0 && reinterpret_cast<uintptr_t>(P.obs) % 4 == 0 && P.stride >= nwords * 4;
    if (p.lds_form()) {
        PerIndexParams Q = p.q;
        Q.m = P;
        for (int w = 0; w < 2; ++w) { Q.mm[w] = p.mm[w]; Q.delta[w] = p.delta[w]; }
        if (dwords && nwords == 4) return per_index_launch_t<4, true>(p, Q, num_cus, stream, big_lds_ok);
        if (dwords && nwords == 5) return per_index_launch_t<5, true>(p, Q, num_cus, stream, big_lds_ok);
        if (dwords && nwords == 6) return per_index_launch_t<6, true>(p, Q, num_cus, stream, big_lds_ok);
        if (dwords && nwords == 8) return per_index_launch_t<8, true>(p, Q, num_cus, stream, big_lds_ok);
        return per_index_launch_t<8, false>(p, Q, num_cus, stream, big_lds_ok);
    }
    PerIndexScanParams C;
    C.m = P;
    C.tab = p.d_tab;
    C.dir = p.d_dir;
    for (int w = 0; w < 2; ++w) { C.u[w] = (uint32_t)p.index[w].size(); C.mm[w] = p.mm[w]; C.delta[w] = p.delta[w]; }
    const uint64_t ntiles = (P.n + kBlock - 1) / kBlock;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(ntiles, (uint64_t)num_cus * 8);
    const size_t lds = (256 + (P.lds_hist ? (size_t)P.S + 1 : 0)) * sizeof(uint32_t);
    if (dwords) hipLaunchKernelGGL(per_index_scan_kernel<-1>, dim3(grid), dim3(kBlock), lds, stream, C);
    else hipLaunchKernelGGL(per_index_scan_kernel<0>, dim3(grid), dim3(kBlock), lds, stream, C);
    FQTK_PAIRS_TRY(hipGetLastError());
    return FQTK_OK;
}

}  // namespace fqtk
