// weighted_scan_kernels.hip.h -- quality-weighted barcode assignment on the matrix cores of gfx950.
//
// What it computes (all integer; include/fqtk_match.h, fqtk_matcher_set_weighted):
//     w[i]    = clamp(qual[i] - 33, 0, 93)
//     cost[s] = sum over i < L of  w[i] * [ enc(read[i]) & ~enc(barcode_s[i]) != 0 ]
//     best = min cost, idx = the LOWEST s that has it, next = the second smallest with multiplicity (0xFFFF when S == 1)
//     None  iff  best > max_cost  or  next - best < min_cost_delta
// No memo can serve this rule -- the answer depends on the qualities -- so every read takes this scan.
//
// How: the int8 contraction of mfma_scan_kernel (mfma_scan_kernels.hip.h), with the base's weight in the read operand.
//   * sample operand: the rows mfma_scan_kernel uses, unchanged (built at create; 0x80 = -128 where the sample does NOT
//     admit the channel, then s & 127 and -(s >> 7) in the two index channels), same row stride, same LDS staging;
//   * read operand: the same 5 channels per base, but the one-hot channel (or the N channel) of base i holds -w[i]
//     (int8, 0 .. -93) instead of -128, so a product is w * 128 and an accumulator is  cost << 7;
//     the first index channel holds 1, the second 0: the accumulator becomes  cost << 7 | (s & 127);
//   * the key: only 7 index bits are free under the cost, which is the sample's row number inside a GROUP of four tiles
//     (128 samples, aligned: s & 127).  v_min_u32 / v_med3_u32 run straight on the accumulators inside a group, as in
//     the unweighted scan; once per group a lane widens its two keys to  cost << 14 | s  and folds them into the running
//     pair:  best' = min(b1, b2),  next' = min(max(b1, b2), n1, n2).  Per read tile that is 32 VALU per tile step (the
//     unweighted scan's; 34 with the hazard step of weighted_tile) plus 14 per group = 3.5 per tile step; shifting
//     every accumulator element into a wide key instead (one v_lshl_add_u32 each) would be 16 more per tile step;
//   * rows past S start from kWeightedPadRow (cost 0xFFFF), above every real key; a cost read out of a key is clamped
//     to 0xFFFF, so S == 1 reports next = 0xFFFF whichever of the initial key or a pad row it came from;
//   * the encode reads the quality row next to the base row through the same load path (load_words) and turns a base
//     into its operand bytes with one LDS look-up, one clamp and one multiply per channel dword;
//   * a read with a two- or three-bit IUPAC code is flagged, as there, and recomputed by its lane after the tiles:
//     planes, AND-NOT per sample, and the sum of w[i] over the mismatch mask's set bits, the qualities read byte by
//     byte from the read's own row -- nothing indexed dynamically, so no scratch, and nothing of it in the tile loop.
// Scope: every read has exactly L bases (no obs_len), L <= 32 (costs <= 32 * 93 = 2976), S <= 16384.
#pragma once
#include "mfma_scan_kernels.hip.h"

namespace fqtk {

constexpr uint32_t kWeightedMaxLen = 32;
constexpr uint32_t kWeightedNoCost = 0xFFFFu;                                   // `next` of a table of one sample
constexpr uint32_t kWeightedGroupInit = (kWeightedNoCost << 7) | 127u;          // inside a group: cost << 7 | s & 127
constexpr int kWeightedPadRow = (int)(kWeightedNoCost << 7);                    // accumulator start of a row past S
constexpr uint32_t kWeightedKeyInit = (kWeightedNoCost << 14) | (kMfmaMaxSamples - 1u);   // across groups: cost << 14 | s

struct WeightedScanParams {
    MfmaScanParams q;       // q.m.obs: bases; q.m.lens is not used (every read has L bases); q.m.max_mm / delta are not used
    const uint8_t *qual;    // n x stride quality bytes, rows as q.m.obs
    uint32_t *costs;        // nullable, n x (best_cost | next_cost << 16)
    uint32_t max_cost;
    uint32_t min_cost_delta;
};

#ifdef __HIPCC__

__device__ __forceinline__ uint32_t weight_of(uint32_t qual_byte) {
    const int w = (int)qual_byte - 33;
    return (uint32_t)(w < 0 ? 0 : (w > 93 ? 93 : w));
}

// One read's operand row: as encode_row, with -w[i] where that one writes 0x80.  mlut: encode_row's.  NG: dwords of bases a variant can meet.
template <int NG>
__device__ __forceinline__ uint32_t encode_weighted_row(const uint32_t (&words)[8], const uint32_t (&quals)[8], uint32_t L, uint32_t lq,
                                                        uint32_t kend, const uint32_t *mlut, uint8_t *row) {
    uint32_t flag = 0;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        if ((uint32_t)g * 4 < lq) {
            // bytes at positions >= L never count: they encode as 0 whatever their quality says
            const int rem = (int)L - g * 4;
            const uint32_t keep = rem >= 4 ? 0xFFFFFFFFu : ((1u << (8 * rem)) - 1u);
            const uint32_t w = words[g] & keep, q = quals[g];
            const uint32_t e0 = mlut[w & 0xFFu], e1 = mlut[(w >> 8) & 0xFFu], e2 = mlut[(w >> 16) & 0xFFu], e3 = mlut[w >> 24];
            // -w as an int8 byte
            const uint32_t n0 = (0u - weight_of(q & 0xFFu)) & 0xFFu, n1 = (0u - weight_of((q >> 8) & 0xFFu)) & 0xFFu;
            const uint32_t n2 = (0u - weight_of((q >> 16) & 0xFFu)) & 0xFFu, n3 = (0u - weight_of(q >> 24)) & 0xFFu;
            flag |= e0 | e1 | e2 | e3;
            u32x4v a;   // (a full multiply: T's bit 24 is past the 24 bits of v_mul_u32_u24)
            a.x = ((e0 >> 7) & 0x01010101u) * n0;
            a.y = ((e1 >> 7) & 0x01010101u) * n1;
            a.z = ((e2 >> 7) & 0x01010101u) * n2;
            a.w = ((e3 >> 7) & 0x01010101u) * n3;
            *reinterpret_cast<u32x4v *>(row + 16 * g) = a;
            *reinterpret_cast<uint32_t *>(row + 4 * lq + 4 * g) =
                __umul24(e0 & 1u, n0) | (__umul24(e1 & 1u, n1) << 8) | (__umul24(e2 & 1u, n2) << 16) | (__umul24(e3 & 1u, n3) << 24);
        }
    }
    *reinterpret_cast<uint32_t *>(row + 5 * lq) = 0x00000001u;   // index channels: 1, 0 -> s & 127
    for (uint32_t o = 5 * lq + 4; o < kend; o += 4) *reinterpret_cast<uint32_t *>(row + o) = 0u;
    return flag & 2u;
}

// One tile of 32 samples against the wave's two read tiles: scan_tile with the fragments in registers, the keys being
// cost << 7 | s & 127.  KS: the table's K steps exactly -- no branch between the MFMAs.
template <int KS, bool TAIL>
__device__ __forceinline__ void weighted_tile(const uint8_t *a, const v4i (&B)[2][KS], uint32_t first_row, uint32_t S, uint32_t h,
                                              uint32_t (&best)[2], uint32_t (&second)[2]) {
    v16i acc[2];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int v = 0; v < 16; ++v)
            acc[rt][v] = (TAIL && first_row + 8u * (v / 4) + 4u * h + (v % 4) >= S) ? kWeightedPadRow : 0;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        const v4i A = *reinterpret_cast<const v4i *>(a + ks * 32);
#pragma unroll
        for (int rt = 0; rt < 2; ++rt) acc[rt] = __builtin_amdgcn_mfma_i32_32x32x32_i8(A, B[rt][ks], acc[rt], 0, 0, 0);
    }
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
        // The first element of a tile goes through plain C++ (v_min, v_xor3: max = a ^ b ^ min, v_min): the compiler sees this
        // read of the MFMA's result and waits out the matrix pipe before it.  med3_u32 is an asm statement, whose operands the
        // hazard recogniser does not follow back to an MFMA; behind this step (a data dependency) every element is complete.
        {
            const uint32_t key = (uint32_t)acc[rt][0];
            const uint32_t nb = min(best[rt], key);
            second[rt] = min(second[rt], best[rt] ^ key ^ nb);
            best[rt] = nb;
        }
#pragma unroll
        for (int v = 1; v < 16; ++v) {
            const uint32_t key = (uint32_t)acc[rt][v];
            second[rt] = med3_u32(best[rt], second[rt], key);
            best[rt] = min(best[rt], key);
        }
    }
}

// A group's pair (keys cost << 7 | local) into the running pair (keys cost << 14 | s); base = the group's first sample.
__device__ __forceinline__ void merge_group(uint32_t gb, uint32_t gn, uint32_t base, uint32_t &best, uint32_t &second) {
    const uint32_t wb = ((gb & ~127u) << 7) + ((gb & 127u) + base);
    const uint32_t wn = ((gn & ~127u) << 7) + ((gn & 127u) + base);
    second = min(max(best, wb), min(second, wn));
    best = min(best, wb);
}

// Every sample tile against the wave's 64 reads: the fragments out of the wave's rows into registers, then chunk by chunk
// (`stage` refills the LDS rows when the table takes more than one), group by group.  Leaves the pairs  cost << 14 | s.
template <int KS, typename Stage>
__device__ __forceinline__ void weighted_tiles(const MfmaScanParams &Q, const uint8_t *smp, const uint8_t *rd_wave, uint32_t frag, uint32_t h,
                                               uint32_t nchunks, Stage &stage, uint32_t (&best)[2], uint32_t (&second)[2]) {
    const uint32_t S = Q.m.S;
    const bool partial = (S & 31u) != 0;
    v4i B[2][KS];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) B[rt][ks] = *reinterpret_cast<const v4i *>(rd_wave + (size_t)rt * 32 * Q.rs + frag + ks * 32);
    wave_lds_sync();   // the next trip's encode overwrites the rows
    for (uint32_t c = 0; c < nchunks; ++c) {
        if (nchunks > 1) {
            __syncthreads();   // the previous chunk has been read by every wave
            stage(c);
            __syncthreads();
        }
        const uint32_t t0 = c * Q.chunk_tiles;
        const uint32_t nt = min(Q.chunk_tiles, Q.ntiles - t0);
        // groups of four tiles by the GLOBAL tile number (the index channel gives s & 127); a chunk edge may cut one
        for (uint32_t st = 0; st < nt;) {
            const uint32_t gt = t0 + st;
            const uint32_t ng = min(4u - (gt & 3u), nt - st);
            const uint32_t nfull = (partial && gt + ng == Q.ntiles) ? ng - 1 : ng;
            uint32_t gb[2], gn[2];
#pragma unroll
            for (int rt = 0; rt < 2; ++rt) gb[rt] = gn[rt] = kWeightedGroupInit;
            const uint8_t *a = smp + (size_t)st * 32 * Q.rs + frag;
#pragma unroll 1
            for (uint32_t k = 0; k < nfull; ++k) weighted_tile<KS, false>(a + (size_t)k * 32 * Q.rs, B, 0, S, h, gb, gn);
            if (nfull < ng) weighted_tile<KS, true>(a + (size_t)nfull * 32 * Q.rs, B, (gt + nfull) * 32u, S, h, gb, gn);
#pragma unroll
            for (int rt = 0; rt < 2; ++rt) merge_group(gb[rt], gn[rt], (gt >> 2) << 7, best[rt], second[rt]);
            st += ng;
        }
    }
}

// KB: K steps of read fragments held in registers (3: L <= 16, 6: L <= 32); VEC: the load path (load_words), of both rows.
template <int KB, int VEC>
__global__ __launch_bounds__(mfma_block_cap(KB)) void weighted_scan_kernel(const WeightedScanParams W) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    const MfmaScanParams &Q = W.q;
    const MatchParams &P = Q.m;
    constexpr int NG = KB == 3 ? 4 : 8;   // dwords of a read's bases
    uint32_t *mlut = smem;             // 256 entries: operand bytes of a read's base (encode_row)
    uint32_t *lds_lut = smem + 256;    // 256 entries: match_kernel's plane LUT, for flagged reads
    uint32_t *lds_hist = smem + 512;   // S+1 entries when P.lds_hist
    const uint32_t bins = P.S + 1;
    const uint32_t hist_dw = P.lds_hist ? ((bins + 3u) & ~3u) : 0u;
    uint8_t *smp = reinterpret_cast<uint8_t *>(smem + 512 + hist_dw);   // chunk_tiles * 32 sample rows
    uint8_t *rd = smp + (size_t)Q.chunk_tiles * 32 * Q.rs;              // per wave: 64 read rows

    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, h = lane >> 5;
    uint8_t *rd_wave = rd + (size_t)wave * 64 * Q.rs;

    if (tid < 256) {
        const uint32_t x = P.lut[tid];
        const uint32_t c = __builtin_popcount(x);
        lds_lut[tid] = x;
        mlut[tid] = c == 1 ? x << 7 : (c == 4 ? 1u : (c == 0 ? 0u : 2u));
    }
    if (P.counts && P.lds_hist)
        for (uint32_t b = tid; b < bins; b += blockDim.x) lds_hist[b] = 0;
    auto stage = [&](uint32_t chunk) {
        const uint32_t t0 = chunk * Q.chunk_tiles;
        const uint32_t nt = min(Q.chunk_tiles, Q.ntiles - t0);
        const u32x4v *src = reinterpret_cast<const u32x4v *>(Q.rows + (size_t)t0 * 32 * Q.rs);
        u32x4v *dst = reinterpret_cast<u32x4v *>(smp);
        const uint32_t nvec = nt * 32u * (Q.rs / 16u);
        for (uint32_t v = tid; v < nvec; v += blockDim.x) dst[v] = src[v];
    };
    const uint32_t nchunks = (Q.ntiles + Q.chunk_tiles - 1) / Q.chunk_tiles;
    if (nchunks == 1) stage(0);
    __syncthreads();

    const uint32_t nwords = (P.L + 3u) >> 2;
    MatchParams PQ = P;   // the quality rows lie as the base rows do
    PQ.obs = W.qual;
    const const_u32x4_ptr tab = (const_u32x4_ptr)(uintptr_t)P.table;
    const uint64_t tile = (uint64_t)(blockDim.x >> 6) * 64;
    const uint64_t ntiles = (P.n + tile - 1) / tile;
    const uint32_t frag = (lane & 31u) * Q.rs + 16u * h;   // a lane's fragment inside a tile of 32 rows

    // every wave of the workgroup makes every trip: the chunked staging below has workgroup barriers
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint64_t i = t * tile + (uint64_t)wave * 64 + lane;
        const bool live = i < P.n;
        uint32_t flagged = 0;
        {
            uint32_t words[8], quals[8];
#pragma unroll
            for (int w = 0; w < 8; ++w) words[w] = quals[w] = 0;
            if (live) {
                load_words<1, VEC, 8>(P, i, nwords, words);
                load_words<1, VEC, 8>(PQ, i, nwords, quals);
            }
            flagged = encode_weighted_row<NG>(words, quals, P.L, Q.lq, 32u * Q.ks, mlut, rd_wave + (size_t)lane * Q.rs);
        }
        wave_lds_sync();
        uint32_t best[2], second[2];
#pragma unroll
        for (int rt = 0; rt < 2; ++rt) best[rt] = second[rt] = kWeightedKeyInit;
        // the table's K steps (kernel-uniform): 1 .. 3 for L <= 16, 4 .. 6 above
        const uint32_t kv = Q.ks - (KB - 3);
        if (kv == 1) weighted_tiles<KB - 2>(Q, smp, rd_wave, frag, h, nchunks, stage, best, second);
        else if (kv == 2) weighted_tiles<KB - 1>(Q, smp, rd_wave, frag, h, nchunks, stage, best, second);
        else weighted_tiles<KB>(Q, smp, rd_wave, frag, h, nchunks, stage, best, second);

        // ---- merge the two lanes that hold a read's column: lanes < 32 own tile 0's reads, lanes >= 32 tile 1's ----
        const uint32_t mb = h ? best[1] : best[0], ms = h ? second[1] : second[0];
        const uint32_t sb = h ? best[0] : best[1], ss = h ? second[0] : second[1];
        const uint32_t ob = (uint32_t)__shfl_xor((int)sb, 32), os = (uint32_t)__shfl_xor((int)ss, 32);
        uint32_t kb = min(mb, ob);
        uint32_t kn = min(max(mb, ob), min(ms, os));

        if (live && flagged) {   // not one-hot: planes, AND-NOT per sample, the weights of the mismatch mask's bits
            uint32_t words[8];
#pragma unroll
            for (int w = 0; w < 8; ++w) words[w] = 0;
            load_words<1, 0, 8>(P, i, nwords, words);
            Planes<1> o;
            encode_planes<1>(words, nwords, P.L, lds_lut, o);
            const uint8_t *qrow = W.qual + i * (uint64_t)P.stride;
            kb = kn = kWeightedKeyInit;
            for (uint32_t s = 0; s < P.S; ++s) {
                const u32x4 e = tab[s];
                uint32_t mask = (o.p[0][0] & e.x) | (o.p[0][1] & e.y) | (o.p[0][2] & e.z) | (o.p[0][3] & e.w);   // bits >= L are clear
                uint32_t cost = 0;
                while (mask) {
                    cost += weight_of(qrow[__builtin_ctz(mask)]);
                    mask &= mask - 1u;
                }
                const uint32_t key = (cost << 14) | s;
                kn = med3_u32(kb, kn, key);
                kb = min(kb, key);
            }
        }

        if (live) {
            const uint32_t bc = min(kb >> 14, kWeightedNoCost), nc = min(kn >> 14, kWeightedNoCost);
            const bool none = bc > W.max_cost || (nc - bc) < W.min_cost_delta;
            const uint32_t idx = kb & (kMfmaMaxSamples - 1u);
            const uint32_t res = none ? 0xFFFFFFFFu : (idx | (min(bc, 255u) << 16) | (min(nc, 255u) << 24));
            FQTK_STREAM_STORE(res, &P.out[i]);
            if (W.costs) FQTK_STREAM_STORE(none ? 0xFFFFFFFFu : (bc | (nc << 16)), &W.costs[i]);
            if (P.counts) {
                const uint32_t bin = none ? P.S : idx;
                if (P.lds_hist) atomicAdd(&lds_hist[bin], 1u);
                else atomicAdd(&P.counts[bin], 1ull);
            }
        }
    }

    if (P.counts && P.lds_hist) {
        __syncthreads();
        for (uint32_t b = tid; b < bins; b += blockDim.x) {
            const uint32_t c = lds_hist[b];
            if (c) atomicAdd(&P.counts[b], (unsigned long long)c);
        }
    }
}

#endif  // __HIPCC__

}  // namespace fqtk
