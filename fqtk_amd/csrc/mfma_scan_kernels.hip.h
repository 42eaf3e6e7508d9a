// mfma_scan_kernels.hip.h -- the exhaustive scan on the matrix cores of gfx950.
//
// What it computes: exactly what match_kernel computes (match_kernels.hip.h), for every input.
//
// How: the mismatch count of every read against every sample is a contraction over one-hot vectors, so it is an int8
// GEMM, and the packed (mismatches, sample index) key that match_kernel builds with VALU shifts is made by the matrix
// pipe itself:
//   * K dimension of one barcode: 4 channels (A C G T) per base, then one N channel per base, then two index channels,
//     zero-padded to the 32-wide K step of v_mfma_i32_32x32x32_i8:
//         byte 4*i + c      (i < L, c = A C G T)   read: 0x80 iff enc(read[i]) is the one-hot code of c
//                                                  sample: 0x80 iff bit c is NOT in E[s][i]
//         byte 4*Lq + i     (Lq = L rounded to 4)  read: 0x80 iff enc(read[i]) == 15;  sample: 0x80 iff E[s][i] != 15
//         byte 5*Lq, 5*Lq+1                        read: 1, -128;                      sample: s & 127, -(s >> 7)
//     (-128) * (-128) = 1 << 14, so one accumulator element is  mismatches << 14 | s  -- no VALU work makes the key,
//     and v_med3_u32 / v_min_u32 run straight on the accumulators.  14 index bits: S <= 16384 (kMfmaMaxSamples).
//   * samples are the M operand, reads the N operand: in the 32x32 result a lane holds ONE read's column and 16 of the
//     tile's 32 sample rows, so the running (best, next) pair of a read lives in two lanes' registers across all
//     sample tiles and is merged once at the end (lane l with lane l + 32);
//   * the sample operand is built once at create (HBM, in the row layout below) and staged in LDS by the workgroup --
//     whole when it fits, else in chunks of tiles per batch of reads; a wave keeps the fragments of its 64 reads
//     (two read tiles) for all K steps in registers, so one 1 KiB sample fragment from LDS feeds two MFMAs;
//   * rows are Kpad + 16 bytes apart: an odd multiple of four dwords, so the 16-byte fragment reads of the 32 rows of a
//     tile fall in distinct banks;
//   * a lane encodes its own read (the load paths of match_kernel) into its wave's private LDS rows, from where the
//     wave reads the fragments back in operand layout -- no workgroup barrier in the loop;
//   * a read with a two- or three-bit IUPAC code (M R W S Y K V H D B) is not one-hot: a sum of channels is not the OR
//     the reference takes.  The encode flags such a read and its lane recomputes it with match_kernel's own VALU
//     step after the tiles (same kernel: no list, no second launch, nothing to size; a wave with such a read pays
//     the old scan's price for it once).
#pragma once
#include "match_kernels.hip.h"

namespace fqtk {

constexpr uint32_t kMfmaMaxSamples = 1u << 14;
constexpr uint32_t kMfmaKeyInit = (255u << 14) | (kMfmaMaxSamples - 1u);   // mm = 255: larger than any real key
constexpr int kMfmaPadRow = 0x40000000;    // accumulator start of a tile row past the last sample: above kMfmaKeyInit
constexpr int kMfmaMaxBlock = 1024;
// Threads per workgroup a variant is compiled for (its __launch_bounds__) = threads of it a CU holds: 1024 leaves a lane 128
// registers, enough with the read fragments of three K steps or none held; with six (KB == 6: 48 registers next to two
// accumulator tiles) 128 spill 45, so that variant is bounded at 512 and gets 256.
constexpr int mfma_block_cap(int kb) { return kb == 6 ? 512 : kMfmaMaxBlock; }
constexpr uint32_t kMfmaLdsBudget = 160u * 1024u;

struct MfmaScanParams {
    MatchParams m;
    const uint8_t *rows;    // [ntiles * 32][rs] sample operand
    uint32_t lq;            // L rounded up to 4
    uint32_t ks;            // 32-wide K steps
    uint32_t rs;            // row stride in bytes (32 * ks + 16)
    uint32_t ntiles;        // 32-sample tiles
    uint32_t chunk_tiles;   // tiles staged in LDS at a time (== ntiles: staged once per workgroup)
};

// Geometry of a table; shared by the create-time row builder, the launcher and the kernel's LDS carve-up.
struct MfmaScanPlan {
    bool ok;
    uint32_t lq, ks, rs, ntiles, chunk_tiles;
    uint32_t kb;      // K steps of read fragments held in registers (3: L <= 16, 6: L <= 32, 0: re-read from LDS)
    uint32_t rt;      // read tiles (of 32) per wave
    uint32_t block;   // threads per workgroup
    uint32_t hist_dw; // dwords of the LDS histogram
    size_t lds;       // dynamic LDS bytes
};

inline MfmaScanPlan plan_mfma_scan(uint32_t S, uint32_t L, bool lds_hist) {
    MfmaScanPlan p{};
    p.lq = (L + 3u) & ~3u;
    p.ks = (5u * p.lq + 4u + 31u) / 32u;
    p.rs = 32u * p.ks + 16u;
    p.ntiles = (S + 31u) / 32u;
    p.kb = L <= 16 ? 3u : (L <= 32 ? 6u : 0u);
    p.rt = p.kb ? 2u : 1u;
    p.hist_dw = lds_hist ? ((S + 1u + 3u) & ~3u) : 0u;
    const size_t fixed = 2048 + (size_t)p.hist_dw * 4;
    const size_t all = (size_t)p.ntiles * 32 * p.rs;
    // the largest workgroup whose waves' read rows fit next to the whole sample operand: one staging per workgroup
    // shared by the most waves; else four waves and as many tiles per chunk as fit
    for (uint32_t block = (uint32_t)mfma_block_cap((int)p.kb); block >= 256; block /= 2) {
        const size_t reads = (size_t)(block / 64) * 32 * p.rt * p.rs;
        if (fixed + reads + all <= kMfmaLdsBudget) {
            p.block = block;
            p.chunk_tiles = p.ntiles;
            p.lds = fixed + reads + all;
            p.ok = S <= kMfmaMaxSamples;
            return p;
        }
    }
    p.block = 256;
    const size_t reads = (size_t)4 * 32 * p.rt * p.rs;
    if (fixed + reads + (size_t)32 * p.rs > kMfmaLdsBudget) return p;
    p.chunk_tiles = (uint32_t)((kMfmaLdsBudget - fixed - reads) / ((size_t)32 * p.rs));
    p.lds = fixed + reads + (size_t)p.chunk_tiles * 32 * p.rs;
    p.ok = S <= kMfmaMaxSamples;
    return p;
}

#ifdef __HIPCC__

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

// Writes and reads of a wave's private LDS rows by different lanes of that wave: LDS executes a wave's accesses in
// order, so only the compiler has to be told.
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// One read's operand row.  mlut[b]: 0x80 in byte c for the one-hot code of channel c; 1 for a no-call; 2 for a two- or
// three-bit code (the read is flagged); 0 for a byte the reference encodes as 0.  Returns non-zero for a flagged read.
template <int NW>
__device__ __forceinline__ uint32_t encode_row(const uint32_t (&words)[NW * 8], uint32_t L, uint32_t lq, uint32_t kend,
                                               const uint32_t *mlut, uint8_t *row) {
    uint32_t flag = 0;
#pragma unroll
    for (int g = 0; g < NW * 8; ++g) {
        if ((uint32_t)g * 4 < lq) {
            // bytes at positions >= L never count
            const int rem = (int)L - g * 4;
            const uint32_t keep = rem >= 4 ? 0xFFFFFFFFu : ((1u << (8 * rem)) - 1u);
            const uint32_t w = words[g] & keep;
            const uint32_t e0 = mlut[w & 0xFFu], e1 = mlut[(w >> 8) & 0xFFu], e2 = mlut[(w >> 16) & 0xFFu], e3 = mlut[w >> 24];
            flag |= e0 | e1 | e2 | e3;
            u32x4v a;
            a.x = e0 & 0x80808080u; a.y = e1 & 0x80808080u; a.z = e2 & 0x80808080u; a.w = e3 & 0x80808080u;
            *reinterpret_cast<u32x4v *>(row + 16 * g) = a;
            *reinterpret_cast<uint32_t *>(row + 4 * lq + 4 * g) =
                ((e0 & 1u) << 7) | ((e1 & 1u) << 15) | ((e2 & 1u) << 23) | ((e3 & 1u) << 31);
        }
    }
    *reinterpret_cast<uint32_t *>(row + 5 * lq) = 0x00008001u;   // index channels: 1, -128
    for (uint32_t o = 5 * lq + 4; o < kend; o += 4) *reinterpret_cast<uint32_t *>(row + o) = 0u;
    return flag & 2u;
}

// One tile of 32 samples against the wave's RT read tiles: KS MFMAs per read tile, then min / med3 over the 16
// accumulators a lane holds of each (rows 8 * (v / 4) + 4 * (lane / 32) + v % 4 of the tile, column lane % 32).
// a: this lane's fragment of the tile's first K step; b: the same of its wave's read rows (KB == 0 only).
// TAIL: the table's last, partial tile -- rows past S start from kMfmaPadRow and so never win.
template <int KB, int RT, bool TAIL>
__device__ __forceinline__ void scan_tile(const uint8_t *a, const uint8_t *b, uint32_t rs, uint32_t KS,
                                          const v4i (&B)[RT][KB > 0 ? KB : 1], uint32_t first_row, uint32_t S, uint32_t h,
                                          uint32_t (&best)[RT], uint32_t (&second)[RT]) {
    v16i acc[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int v = 0; v < 16; ++v)
            acc[rt][v] = (TAIL && first_row + 8u * (v / 4) + 4u * h + (v % 4) >= S) ? kMfmaPadRow : 0;
    if constexpr (KB > 0) {
#pragma unroll
        for (int ks = 0; ks < KB; ++ks) {
            if ((uint32_t)ks < KS) {
                const v4i A = *reinterpret_cast<const v4i *>(a + ks * 32);
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) acc[rt] = __builtin_amdgcn_mfma_i32_32x32x32_i8(A, B[rt][ks], acc[rt], 0, 0, 0);
            }
        }
    } else {
        for (uint32_t ks = 0; ks < KS; ++ks) {
            const v4i A = *reinterpret_cast<const v4i *>(a + ks * 32);
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                const v4i Bv = *reinterpret_cast<const v4i *>(b + (size_t)rt * 32 * rs + ks * 32);
                acc[rt] = __builtin_amdgcn_mfma_i32_32x32x32_i8(A, Bv, acc[rt], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const uint32_t key = (uint32_t)acc[rt][v];
            second[rt] = med3_u32(best[rt], second[rt], key);
            best[rt] = min(best[rt], key);
        }
}

// NW, VEC: as match_kernel (the flagged reads' VALU step, the load path).  KB, RT: MfmaScanPlan::kb, rt.
template <int NW, int KB, int RT, int VEC>
__global__ __launch_bounds__(mfma_block_cap(KB)) void mfma_scan_kernel(const MfmaScanParams Q) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    const MatchParams &P = Q.m;
    uint32_t *mlut = smem;             // 256 entries: operand bytes of a read's base (encode_row)
    uint32_t *lds_lut = smem + 256;    // 256 entries: match_kernel's plane LUT, for flagged reads
    uint32_t *lds_hist = smem + 512;   // S+1 entries when P.lds_hist
    const uint32_t bins = P.S + 1;
    const uint32_t hist_dw = P.lds_hist ? ((bins + 3u) & ~3u) : 0u;
    uint8_t *smp = reinterpret_cast<uint8_t *>(smem + 512 + hist_dw);   // chunk_tiles * 32 sample rows
    uint8_t *rd = smp + (size_t)Q.chunk_tiles * 32 * Q.rs;              // per wave: 32 * RT read rows

    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, h = lane >> 5;
    constexpr uint32_t RW = 32u * RT;
    uint8_t *rd_wave = rd + (size_t)wave * RW * Q.rs;

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
    const const_u32x4_ptr tab = (const_u32x4_ptr)(uintptr_t)P.table;
    const uint64_t tile = (uint64_t)(blockDim.x >> 6) * RW;
    const uint64_t ntiles = (P.n + tile - 1) / tile;
    const uint32_t frag = (lane & 31u) * Q.rs + 16u * h;   // a lane's fragment inside a tile of 32 rows
    const bool partial = (P.S & 31u) != 0;

    // every wave of the workgroup makes every trip: the chunked staging below has workgroup barriers
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint64_t i = t * tile + (uint64_t)wave * RW + lane;
        const bool live = lane < RW && i < P.n;
        uint32_t flagged = 0;
        if (lane < RW) {
            uint32_t words[NW * 8];
#pragma unroll
            for (int w = 0; w < NW * 8; ++w) words[w] = 0;
            if (live) load_words<NW, VEC, NW * 8>(P, i, nwords, words);
            flagged = encode_row<NW>(words, P.L, Q.lq, 32u * Q.ks, mlut, rd_wave + (size_t)lane * Q.rs);
        }
        wave_lds_sync();
        v4i B[RT][KB > 0 ? KB : 1];
        if constexpr (KB > 0) {
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int ks = 0; ks < KB; ++ks)
                    if ((uint32_t)ks < Q.ks) B[rt][ks] = *reinterpret_cast<const v4i *>(rd_wave + (size_t)rt * 32 * Q.rs + frag + ks * 32);
            wave_lds_sync();   // the next trip's encode overwrites the rows
        }

        uint32_t best[RT], second[RT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) best[rt] = second[rt] = kMfmaKeyInit;

        for (uint32_t c = 0; c < nchunks; ++c) {
            if (nchunks > 1) {
                __syncthreads();   // the previous chunk has been read by every wave
                stage(c);
                __syncthreads();
            }
            const uint32_t t0 = c * Q.chunk_tiles;
            const uint32_t nt = min(Q.chunk_tiles, Q.ntiles - t0);
            const uint32_t nfull = (partial && t0 + nt == Q.ntiles) ? nt - 1 : nt;
            for (uint32_t st = 0; st < nfull; ++st)
                scan_tile<KB, RT, false>(smp + (size_t)st * 32 * Q.rs + frag, rd_wave + frag, Q.rs, Q.ks, B, 0, P.S, h, best, second);
            if (nfull < nt)
                scan_tile<KB, RT, true>(smp + (size_t)nfull * 32 * Q.rs + frag, rd_wave + frag, Q.rs, Q.ks, B, (t0 + nfull) * 32u, P.S, h, best, second);
        }
        if constexpr (KB == 0) wave_lds_sync();

        // ---- merge the two lanes that hold a read's column: lanes < 32 own tile 0's reads, lanes >= 32 tile 1's ----
        uint32_t mb = best[0], ms = second[0], sb = best[0], ss = second[0];
        if constexpr (RT == 2) {
            mb = h ? best[1] : best[0];
            ms = h ? second[1] : second[0];
            sb = h ? best[0] : best[1];
            ss = h ? second[0] : second[1];
        }
        const uint32_t ob = (uint32_t)__shfl_xor((int)sb, 32), os = (uint32_t)__shfl_xor((int)ss, 32);
        const uint32_t kb = min(mb, ob);
        const uint32_t kn = min(max(mb, ob), min(ms, os));
        uint32_t bm = kb >> 14, nm = kn >> 14, bi = kb & (kMfmaMaxSamples - 1u);

        if (live && flagged) {   // not one-hot: the exact VALU step of match_kernel for this read
            uint32_t words[NW * 8];
#pragma unroll
            for (int w = 0; w < NW * 8; ++w) words[w] = 0;
            load_words<NW, 0, NW * 8>(P, i, nwords, words);
            Planes<NW> o;
            encode_planes<NW>(words, nwords, P.L, lds_lut, o);
            uint32_t b16 = kKeyInit, s16 = kKeyInit;
            for (uint32_t s = 0; s < P.S; ++s) {
                SampleGroup<NW, 1> one;
                one.load(tab, s);
                update<NW>(o, one.e[0], s, b16, s16);
            }
            bm = b16 >> 16;
            nm = s16 >> 16;
            bi = b16 & 0xFFFFu;
        }

        // ---- decision + length rules: as match_kernel ---------------------------------------------------------
        if (live) {
            bool none = bm > P.max_mm || (nm - bm) < P.delta;
            if (P.lens) {
                const uint32_t len = P.lens[i];
                if (len < P.L) {
                    none = true;
                } else if (len > P.L) {
                    none = true;
                    overlong_read(P, i, len);
                }
            }
            const uint32_t idx = none ? kNoMatch : bi;
            const uint32_t res = none ? 0xFFFFFFFFu : (idx | (bm << 16) | (nm << 24));
            FQTK_STREAM_STORE(res, &P.out[i]);
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
