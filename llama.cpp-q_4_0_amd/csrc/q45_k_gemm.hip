// q45_k_gemm.hip — the prefill GEMM of the Q5_K / Q4_K x F32 mul_mat (gfx950, wave64): k_gemm_q45_K on the int8
// matrix cores, one template parameter QH (true: Q5_K, false: Q4_K), y bit for bit what the GEMV k_gemv_q45_K
// (q45_k.hip) gives.
//
// The GEMV computes, per output and superblock b of 256 elements, the exact int32
//   isum_b = sum_s sc[s] sum_(l) q q8        0 <= sc[s] q <= 63 * 31 (Q5_K) / 63 * 15 (Q4_K), |q8| <= 128
//   msum_b = sum_s m[s] bsum32[s]            0 <= m[s] <= 63, bsum32[s] = the sum of the 32 q8 of sub-block s
// and then t_b = fmaf(d_x d, (float)isum_b, -((d_x dmin) (float)msum_b)), acc = acc + t_b, superblocks in order
// from +0 (d_x d and d_x dmin one rounded multiply each).  Both sums come off the matrix cores exactly:
//   isum  The scaled weight w' = sc[s] q is an integer in [0, 1953] and splits into two int8 digits, w' = 128 hi
//         + lo with lo = w' & 127 in [0, 127] and hi = w' >> 7 in [0, 15].  Two chains of eight
//         v_mfma_i32_32x32x32_i8 over the superblock's K = 256, hi . q8 and lo . q8, with nothing in between,
//         accumulate H (|H| <= 15 * 128 * 256 < 2^19) and L (|L| <= 127 * 128 * 256 < 2^22); isum_b = 128 H + L
//         (|isum_b| <= 1953 * 128 * 256 < 2^26).
//   msum  bsum32 is in [-4096, 4064] (q8_K gives -128 to the block's extreme element when it is negative, so a
//         sub-block can be all -128; the other end is 32 * 127) and splits into bl = bsum32 & 127 in [0, 127] and
//         bh = bsum32 >> 7 (arithmetic) in [-32, 31].  One v_mfma_i32_32x32x16_i8 per digit against the row's
//         eight m bytes (K slots 0..7; the slots 8..15 of the weight operand are zero) gives Ml (|Ml| <= 8 * 63 *
//         127 < 2^16) and Mh (|Mh| <= 8 * 63 * 32 < 2^14); msum_b = 128 Mh + Ml (|msum_b| <= 8 * 63 * 4096 < 2^21,
//         exact in fp32).
// The fp32 step that follows is the GEMV's, in the GEMV's order (K is never split across waves or workgroups;
// the GEMV's (acc + t_even) + t_odd with a dead t = +0 is the same sequence, since acc is never -0).  Hence
// equality, not a tolerance, and a result that does not depend on the tile shape or the grid.
//
// Weights are read in place (no image): the workgroup decodes its 64-row tile's superblock into the two digit
// planes in LDS once, and every column of the tile reuses it.  Blocks are multiples of 16 bytes in a 16-byte
// aligned matrix, so the decode is the GEMV's: half a wave per row and superblock, lane t of the half (j = t / 8,
// i = t % 8) loads the block's 16-byte header (one address per half), qs dword t = four low nibbles of sub-block
// 2j and four high nibbles of sub-block 2j + 1, for Q5_K also qh dword i; every load is a naturally aligned vector
// load inside the matrix.  Rows >= M and columns >= N of a ragged tile read the last row / column (inside the
// operands) and are never stored.  x is the q8_K quantization (q8k_block_lane, the GEMV prologue's bits) written
// once per call as planes: qs int8 [N][K], d f32 [N][K / 256] and dig int8 [N][K / 256][16], the eight bl then
// the eight bh of the (token, superblock)'s bsum32 (k_quantize_q8_K_planes<true>, kquant_gemm.h).
//
// Tile: 64 rows x 32 WN TN columns, 2 x WN waves, each TN 32 x 32 MFMA tiles ((WN, TN) = (2, 1) up to N = 64,
// (4, 1) up to 128 and wherever its grid still fits on the device at once, else (4, 2): the set of k_gemm_q6_K;
// the rule is gemm_tile_columns, launch.h); MFMA A = x (D's register index = column), B = weights
// (D's lane = row), so d and dmin are one value each per lane and the y stores run along m.  Registers: a wave has
// 256 at two waves per SIMD (launch bound 512), and at TN = 2 the prefetched operands take about 60 of them, so
// a wave finishes one 32 x 32 tile (H, L, Mh, Ml: 64) before it starts the next; acc is 16 TN.
// LDS: the digit and x rows are 256 + 16 bytes, which spreads the 32 rows of an operand read (ds_read_b128, 16
// bytes per lane, banks mod 64 in groups of 16 lanes) over all 64 banks: row c starts at bank 4c mod 64, and the 16
// lanes of a group have 16 distinct c mod 16.  The decode's ds_write_b32 (banks mod 32 per 32-lane half = one row)
// go to dwords 16j + i and 16j + 8 + i of the row: j and j + 2 share banks, a 2-way conflict on stores that take 4
// issue cycles for 2 array cycles anyway.  The m bytes and the bsum32 digits are 8 bytes per row / column
// (ds_read_b64, 32 lanes on 64 distinct banks).  One superblock per stage in a single LDS buffer; the next
// superblock's global loads are issued before the current one's MFMAs.
#include "kquant_gemm.h"
#include "q45_k_device.h"

namespace ghip {

// four 4- or 5-bit values (one per byte) and their sub-block's scale (<= 63) -> the int8 digits of w' = sc q =
// 128 hi + lo, packed in element order.  Elements 0, 2 and 1, 3 go through 16-bit fields of one 24-bit multiply:
// a field is at most 1953 < 2^11, so nothing carries from one field into the next.
__device__ __forceinline__ void q45_digits(uint32_t q, uint32_t sc, uint32_t &hi, uint32_t &lo) {
    const uint32_t we = __umul24(q & 0x00FF00FFu, sc), wo = __umul24((q >> 8) & 0x00FF00FFu, sc);
    lo = (we & 0x007F007Fu) | ((wo & 0x007F007Fu) << 8);
    hi = ((we >> 7) & 0x000F000Fu) | ((wo << 1) & 0x0F000F00u);
}

template <bool QH, int WN, int TN>
__global__ __launch_bounds__(128 * WN) void k_gemm_q45_K(const uint8_t *__restrict__ W, int nb, int M,
                                                          const uint8_t *__restrict__ xqs, const float *__restrict__ xd,
                                                          const uint8_t *__restrict__ xdig, int N, int ntn,
                                                          float *__restrict__ y, int64_t ldy) {
    constexpr int BS = Q45<QH>::BYTES, QS = Q45<QH>::QS;
    constexpr int THREADS = 128 * WN;                  // 2 x WN waves
    constexpr int BN = 32 * WN * TN;                   // columns per workgroup
    constexpr int NP = KG_BM / (4 * WN);              // row pairs a wave decodes per superblock (half a wave per row)
    constexpr int XP = BN * 16 / THREADS;              // 16-byte pieces of the x tile per thread (4 TN)
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint8_t *whi = smem;                               // [64][KG_LD]
    uint8_t *wlo = whi + KG_BM * KG_LD;              // [64][KG_LD]
    uint8_t *xs = wlo + KG_BM * KG_LD;               // [BN][KG_LD]
    uint8_t *ms = xs + BN * KG_LD;                    // [64][8]   m[0..7]
    uint8_t *xdl = ms + KG_BM * 8;                    // [BN][8]   bl[0..7]
    uint8_t *xdh = xdl + BN * 8;                       // [BN][8]   bh[0..7]
    float *dws = reinterpret_cast<float *>(xdh + BN * 8);      // [64]
    float *dmws = dws + KG_BM;                        // [64]
    float *dxs = dmws + KG_BM;                        // [BN]
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // the column tiles of one row tile are neighbours in the grid (they share the weight rows)
    const int mt = (int)(blockIdx.x / (unsigned)ntn), nt = (int)(blockIdx.x - (unsigned)mt * (unsigned)ntn);
    const int m0 = mt * KG_BM, n0 = nt * BN;
    const int K = nb * QK_K;
    const int64_t rowbytes = (int64_t)nb * BS;

    // decoding lane: half a wave per row, lane t of the half owns elements 4i .. 4i + 3 of sub-blocks 2j, 2j + 1
    const int half = lane >> 5, t = lane & 31, j = t >> 3, i = t & 7;

    // (unconditional loads at clamped indices, always inside the operands)
    const uint8_t *rowp[NP];
#pragma unroll
    for (int u = 0; u < NP; u++) {
        const int m = m0 + wave * 2 * NP + 2 * u + half;
        rowp[u] = W + (int64_t)(m < M ? m : M - 1) * rowbytes;
    }
    int xoff[XP];
#pragma unroll
    for (int ii = 0; ii < XP; ii++) {
        const int p = tid + THREADS * ii, n = n0 + (p >> 4);
        xoff[ii] = (n < N ? n : N - 1) * K + (p & 15) * 16;             // N K < 2^31 (host check)
    }
    const int dn = n0 + (tid & (BN - 1));
    const int dxoff = (dn < N ? dn : N - 1) * nb;

    struct Regs {                                      // one superblock of the tile's operands, as loaded
        u32x4 hdr[NP];
        uint32_t qs[NP], qh[NP];
        u32x4 x[XP];
        u32x4 dig;
        float dx;
    };
    auto prefetch = [&](int b, Regs &g) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < NP; u++) {
            const uint8_t *p = rowp[u] + b * BS;
            g.hdr[u] = *reinterpret_cast<const u32x4 *>(p);
            g.qs[u] = reinterpret_cast<const uint32_t *>(p + QS)[t];
            g.qh[u] = QH ? reinterpret_cast<const uint32_t *>(p + 16)[i] : 0u;
        }
#pragma unroll
        for (int p = 0; p < XP; p++) g.x[p] = *reinterpret_cast<const u32x4 *>(xqs + xoff[p] + b * QK_K);
        g.dig = *reinterpret_cast<const u32x4 *>(xdig + (dxoff + b) * 16);
        g.dx = xd[dxoff + b];
    };
    auto stage = [&](const Regs &g) __attribute__((always_inline)) {          // a superblock's registers -> LDS
#pragma unroll
        for (int u = 0; u < NP; u++) {
            const int r = wave * 2 * NP + 2 * u + half;
            const u32x4 hdr = g.hdr[u];
            const ScaleMin sm = unpack_scales_k4(hdr.y, hdr.z, hdr.w);
            const uint32_t scw = (j < 2 ? sm.sc_lo : sm.sc_hi) >> (16 * (j & 1));
            uint32_t qlo = g.qs[u] & 0x0F0F0F0Fu, qhi = (g.qs[u] >> 4) & 0x0F0F0F0Fu;
            if (QH) {
                qlo |= ((g.qh[u] >> (2 * j)) & 0x01010101u) << 4;
                qhi |= ((g.qh[u] >> (2 * j + 1)) & 0x01010101u) << 4;
            }
            uint32_t h0, l0, h1, l1;
            q45_digits(qlo, scw & 0xFFu, h0, l0);
            q45_digits(qhi, (scw >> 8) & 0xFFu, h1, l1);
            const int o = r * KG_LD + 64 * j + 4 * i;
            *reinterpret_cast<uint32_t *>(whi + o) = h0;
            *reinterpret_cast<uint32_t *>(whi + o + 32) = h1;
            *reinterpret_cast<uint32_t *>(wlo + o) = l0;
            *reinterpret_cast<uint32_t *>(wlo + o + 32) = l1;
            if (t == 0) {
                *reinterpret_cast<u32x2 *>(ms + 8 * r) = u32x2{sm.m_lo, sm.m_hi};
                dws[r] = h2f(hdr.x & 0xFFFFu);
                dmws[r] = h2f(hdr.x >> 16);
            }
        }
#pragma unroll
        for (int p = 0; p < XP; p++) {
            const int pp = tid + THREADS * p;
            *reinterpret_cast<u32x4 *>(xs + (pp >> 4) * KG_LD + (pp & 15) * 16) = g.x[p];
        }
        if (tid < BN) {
            *reinterpret_cast<u32x2 *>(xdl + 8 * tid) = u32x2{g.dig.x, g.dig.y};
            *reinterpret_cast<u32x2 *>(xdh + 8 * tid) = u32x2{g.dig.z, g.dig.w};
            dxs[tid] = g.dx;
        }
    };

    const int wr = wave & 1, wt = wave >> 1;
    const int c = lane & 31, h = lane >> 5;
    const uint8_t *bh_p = whi + (32 * wr + c) * KG_LD + 16 * h;
    const uint8_t *bl_p = wlo + (32 * wr + c) * KG_LD + 16 * h;
    const uint8_t *a_p = xs + (32 * TN * wt + c) * KG_LD + 16 * h;
    const i32x16 iz = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    float acc[TN][16];
#pragma unroll
    for (int tt = 0; tt < TN; tt++)
#pragma unroll
        for (int e = 0; e < 16; e++) acc[tt][e] = 0.0f;

    // superblock b: its registers -> LDS, the loads of b + 1 into the same registers, then the MFMAs and the
    // fp32 step
    Regs g;
    prefetch(0, g);
    for (int b = 0; b < nb; b++) {
        __syncthreads();                               // the previous superblock's LDS reads are done
        stage(g);
        __syncthreads();
        prefetch(b + 1 < nb ? b + 1 : nb - 1, g);
        const float dw = dws[32 * wr + c], dmw = dmws[32 * wr + c];
        // the mins: K slots 0..7 (the lanes of h = 0) carry m[s] against the bsum32 digits; the weight operand's
        // slots 8..15 are zero, whatever the x operand holds there
        const long mrow = *reinterpret_cast<const long *>(ms + 8 * (32 * wr + c));
        const long bm = h ? 0L : mrow;
        // one 32 x 32 tile at a time (the weight digits are read from LDS again for the second tile: at TN = 2
        // H, L, the mins' term and acc of both tiles at once do not fit beside the prefetched operands)
#pragma unroll
        for (int tt = 0; tt < TN; tt++) {
            const int col = 32 * TN * wt + 32 * tt + c;
            const long al = *reinterpret_cast<const long *>(xdl + 8 * col);
            const long ah = *reinterpret_cast<const long *>(xdh + 8 * col);
            const i32x16 Ml = __builtin_amdgcn_mfma_i32_32x32x16_i8(al, bm, iz, 0, 0, 0);
            const i32x16 Mh = __builtin_amdgcn_mfma_i32_32x32x16_i8(ah, bm, iz, 0, 0, 0);
            i32x16 H = iz, L = iz;
#pragma unroll
            for (int s = 0; s < QK_K / 32; s++) {
                const i32x4 a = *reinterpret_cast<const i32x4 *>(a_p + 32 * tt * KG_LD + 32 * s);
                const i32x4 bh = *reinterpret_cast<const i32x4 *>(bh_p + 32 * s);
                const i32x4 bl = *reinterpret_cast<const i32x4 *>(bl_p + 32 * s);
                H = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, bh, H, 0, 0, 0);
                L = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, bl, L, 0, 0, 0);
            }
            // the superblock's fp32 step per output: the GEMV's, in the GEMV's order
#pragma unroll
            for (int e = 0; e < 16; e++) {
                const float dx = dxs[kquant_col(32 * TN * wt + 32 * tt, e, h)];
                const int msum = Mh[e] * 128 + Ml[e], isum = H[e] * 128 + L[e];
                const float negp = -__fmul_rn(__fmul_rn(dx, dmw), (float)msum);
                const float tb = __builtin_fmaf(__fmul_rn(dx, dw), (float)isum, negp);
                acc[tt][e] = __fadd_rn(acc[tt][e], tb);
            }
        }
    }

    const int row = m0 + 32 * wr + c;
    if (row < M) {
#pragma unroll
        for (int t = 0; t < TN; t++)
#pragma unroll
            for (int e = 0; e < 16; e++) {
                const int n = kquant_col(n0 + 32 * TN * wt + 32 * t, e, h);
                if (n < N) y[(int64_t)n * ldy + row] = acc[t][e];
            }
    }
}

template <bool QH>
static hipError_t gemm_q45_K_t(const void *W, int64_t K, int64_t M, const void *xqs, const float *xd, const void *xdig,
                               int64_t N, float *y, int64_t ldy, int num_cus, hipStream_t s) {
    return with_kquant_tile(K, M, N, num_cus, true, [&](auto wn, auto tn, int nb) {
        constexpr int WN = decltype(wn)::value, TN = decltype(tn)::value, BN = 32 * WN * TN;
        constexpr size_t lds = (size_t)(2 * KG_BM + BN) * KG_LD + (size_t)(KG_BM + 2 * BN) * 8 + (size_t)(2 * KG_BM + BN) * 4;
        return launch_gemm_kquant<k_gemm_q45_K<QH, WN, TN>, WN, TN>(lds, M, N, [&](dim3 grid, dim3 block, int ntn) {
            launch_k(k_gemm_q45_K<QH, WN, TN>, grid, block, lds, s, (const uint8_t *)W, nb, (int)M, (const uint8_t *)xqs,
                     xd, (const uint8_t *)xdig, (int)N, ntn, y, ldy);
        });
    });
}

// y[n * ldy + m] = W[m] . x[n] on the planes quantize_q8_K_planes wrote with dig; any K % 256 == 0, M, N >= 1
hipError_t gemm_q45_K(bool qh, const void *W, int64_t K, int64_t M, const void *xqs, const float *xd, const void *xdig,
                      int64_t N, float *y, int64_t ldy, const DeviceInfo &dev, hipStream_t s) {
    return qh ? gemm_q45_K_t<true>(W, K, M, xqs, xd, xdig, N, y, ldy, dev.num_cus, s)
              : gemm_q45_K_t<false>(W, K, M, xqs, xd, xdig, N, y, ldy, dev.num_cus, s);
}

}  // namespace ghip
