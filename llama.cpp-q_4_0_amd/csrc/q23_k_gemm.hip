// q23_k_gemm.hip — the prefill GEMM of the Q3_K / Q2_K x F32 mul_mat (gfx950, wave64): k_gemm_q23_K on the int8
// matrix cores, one template parameter Q3 (true: Q3_K, false: Q2_K), y bit for bit what the GEMV k_gemv_q23_K
// (q23_k.hip) gives.
//
// The GEMV computes, per output and superblock b of 256 elements, the exact int32
//   isum_b = sum_s sc[s] sum_(l) q q8        16 elements per sub-block s, |q8| <= 128
//   msum_b = sum_s m[s] bsum16[s]            Q2_K only; bsum16[s] = the sum of the 16 q8 of sub-block s
// and then t_b = (d_x d) (float)isum_b (Q3_K) or fmaf(d_x d, (float)isum_b, -((d_x dmin) (float)msum_b)) (Q2_K),
// acc = acc + t_b, superblocks in order from +0 (d_x d and d_x dmin one rounded multiply each).  Here the scale is
// folded into the int8 weight, so both sums come off the matrix cores exactly, with ONE chain of eight
// v_mfma_i32_32x32x32_i8 per 32 x 32 tile and superblock:
//   Q3_K  sc in [-32, 31], q in [-4, 3]: sc q is in [-124, 128], not an int8, but the negated product w" = (-sc) q
//         is in [-128, 124] (the ends are 32 * -4 and -31 * -4).  The chain over w" gives S with |S| <= 128 * 128 *
//         256 = 2^22, and isum_b = -S: the negation of an int32 of that size is exact, so (float)isum_b is the
//         GEMV's value.  w" is formed per byte mod 256 through 16-bit fields (q23_scaled): the product of two 8-bit
//         factors is below 2^16, so nothing carries from one field into the next, and the low byte of a field is
//         the right int8 whatever the signs, because the true value fits in one.  No mins, no digit planes.
//   Q2_K  sc in [0, 15], q in [0, 3]: w' = sc q is in [0, 45]; the four bytes of a dword times sc is one 32-bit
//         multiply without carries.  |isum_b| <= 45 * 128 * 256 < 2^21.
//   msum  bsum16 is in [-2048, 2032] (q8_K gives -128 to the block's extreme element when it is negative, so a
//         sub-block can be all -128; the other end is 16 * 127) and splits into bl = bsum16 & 127 in [0, 127] and
//         bh = bsum16 >> 7 (arithmetic) in [-16, 15].  One v_mfma_i32_32x32x16_i8 per digit against the row's
//         sixteen m bytes (0 <= m <= 15): K = 16 is exactly the sixteen sub-blocks, no padded slots.  |Ml| <= 16 *
//         15 * 127 < 2^15, |Mh| <= 16 * 15 * 16 < 2^12, msum_b = 128 Mh + Ml, |msum_b| <= 16 * 15 * 2048 < 2^19,
//         exact in fp32.
// The fp32 step that follows is the GEMV's, in the GEMV's order (K is never split across waves or workgroups;
// the GEMV's four adds per step with a dead t = +0 are the same sequence, since acc is never -0).  Hence equality,
// not a tolerance, and a result that does not depend on the tile shape or the grid.
//
// Weights are read in place (no image): the workgroup decodes its 64-row tile's superblock into one int8 plane in
// LDS once, and every column of the tile reuses it.  The decode is the GEMV's, with its alignment rule (q23_k.hip):
// a quarter wave per (row, superblock), lane t of the quarter (n = t / 8, i = t % 8) loads qs dword 8n + i, for Q3_K
// also hmask dword i, and the scales; q23_values gives the four dwords of elements 128n + 32k + 4i .. + 3 (k = 0..3),
// which the lane scales and stores at those element offsets of the row's plane, so the MFMA's K slots see x's
// natural element order.  The matrix is 4-byte aligned.  A Q2_K block (84 bytes) is dword aligned and read as
// aligned dwords 0 .. 20.  A Q3_K block (110 bytes) sits at mis = 0 or 2 mod 4; every 32-bit field comes from the
// aligned dwords that hold it (blk_dword), d is a 16-bit load.  The aligned span of a block at 2 mod 4 starts two
// bytes before it, in the previous block's d (a 4-byte aligned matrix never starts at 2 mod 4), and ends with the
// dword of bytes 106 .. 109, the block's last; the span of an aligned block ends with the dword of bytes 104 ..
// 107.  Rows >= M of a ragged tile read row M - 1 and superblocks past the end are never requested (the prefetch
// of the last iteration repeats the last superblock), so every lane's addresses are those of a real block: no byte
// outside [W, W + M (K / 256) BYTES) is read, by clamped lanes either.  Columns >= N read column N - 1 of the x
// planes.  Clamped rows and columns are never stored.  x is the q8_K quantization written once per call as planes
// by quantize_q8_K_planes (q6_k_gemm.hip; the GEMV prologue's bits): qs int8 [N][K], d f32 [N][K / 256].  The
// bsum16 digits of Q2_K need no plane: the thread that stages a 16-byte piece of the x tile holds exactly one
// sub-block, sums it (four v_dot4 against 0x01010101) and writes the two digit bytes to LDS.
//
// Tile: 64 rows x 32 WN TN columns, 2 x WN waves, each TN 32 x 32 MFMA tiles; the (WN, TN) set and the rule of
// k_gemm_q45_K (gemm_tile_columns, launch.h); MFMA A = x (D's register index = column), B = weights (D's lane = row), so d and
// dmin are one value each per lane and the y stores run along m.  Registers (256 per wave at two waves per SIMD):
// the prefetched operands are at most 9 x 4 weight dwords and 8 x 4 of x, a tile's S, Mh, Ml 48, acc 16 TN.
// LDS: the weight and x rows are 256 + 16 bytes, which spreads the 32 rows of an operand read (ds_read_b128, banks
// mod 64 in groups of 16 lanes) over all 64 banks: row c starts at bank 4c mod 64, and the 16 lanes of a group have
// 16 distinct c mod 16.  The decode's ds_write_b32 (banks mod 32, per 32-lane half = two rows): the lane of row r
// writes dword 68 r + 32 n + 8 k + i, bank 4 r + 8 k + i mod 32.  n = 0 and n = 1 share a bank, the 2-way
// conflict of k_gemm_q45_K's stores; two adjacent rows would overlap in four banks on top of that (4-way), so the
// two quarters of a half take rows r and r + 2, eight banks apart: 16 banks, 2-way.  The m bytes and the bsum16
// digits are 16 bytes per row / column, read as ds_read_b64 at 16 c + 8 h: 512 contiguous bytes per wave, the 32
// lanes of a half on 64 distinct banks.  One superblock per LDS stage; the next superblock's global loads are
// issued before the current one's MFMAs.  The 64- and 128-column tiles have two stages (at most 2 x 57 KB)
// and one barrier per superblock: a wave decodes superblock b + 1 into the other stage before its MFMAs of b, so
// its decode overlaps the other waves' MFMAs (measured 13-32 % less time than one stage on the LLaMA-7B layer
// shapes, profiles/q23k_gemm.json against q23k_gemm_build1.json; y is the same).  Two stages of the 256-column
// tile (2 x 97 KB) exceed the 160 KiB, so it keeps one stage and two barriers.
#include "kquant_gemm.h"
#include "q23_k_device.h"

namespace ghip {

// an LDS stage of a BN-column tile: the weight and x planes, Q2_K's m bytes and digit bytes, d, dmin, d_x
template <bool Q3>
constexpr int G23_stage_bytes(int BN) {
    return (KG_BM + BN) * KG_LD + (Q3 ? 0 : (KG_BM + 2 * BN) * 16) + (2 * KG_BM + BN) * 4;
}
constexpr int G23_stages(int TN) { return TN == 1 ? 2 : 1; }     // two stages of the 256-column tile exceed the LDS

// four values (one per byte; Q3_K signed, Q2_K 0..3) times their sub-block's scale -> four int8 in element order.
// Q3_K: nsc = (-sc) & 0xFF; elements 0, 2 and 1, 3 go through 16-bit fields, a field is at most 255 * 255 < 2^16.
// Q2_K: a byte is at most 3 * 15 = 45, nothing carries.
template <bool Q3>
__device__ __forceinline__ uint32_t q23_scaled(uint32_t q, uint32_t sc) {
    if (!Q3) return q * sc;
    const uint32_t we = (q & 0x00FF00FFu) * sc, wo = ((q >> 8) & 0x00FF00FFu) * sc;
    return (we & 0x00FF00FFu) | ((wo & 0x00FF00FFu) << 8);
}

template <bool Q3, int WN, int TN>
__global__ __launch_bounds__(128 * WN) void k_gemm_q23_K(const uint8_t *__restrict__ W, int nb, int M,
                                                          const uint8_t *__restrict__ xqs, const float *__restrict__ xd,
                                                          int N, int ntn, float *__restrict__ y, int64_t ldy) {
    constexpr int BS = Q23<Q3>::BYTES;
    constexpr int THREADS = 128 * WN;                  // 2 x WN waves
    constexpr int BN = 32 * WN * TN;                   // columns per workgroup
    constexpr int NP = KG_BM / (8 * WN);              // passes of four rows a wave decodes per superblock
    constexpr int XP = BN * 16 / THREADS;              // 16-byte pieces of the x tile per thread (4 TN)
    constexpr int NW = Q3 ? 9 : 5;                     // a lane's weight dwords per pass (Gemv23Regs' of q23_k.hip)
    constexpr int DG = Q3 ? 0 : 16;                    // bytes of m per row / of each bsum16 digit per column
    constexpr int SB = G23_stage_bytes<Q3>(BN);        // one LDS stage
    constexpr int NS = G23_stages(TN);                 // stages: two where they fit (header)
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint8_t *wq = smem;                                // [64][KG_LD]  the scaled weights
    uint8_t *xs = wq + KG_BM * KG_LD;                // [BN][KG_LD]
    uint8_t *ms = xs + BN * KG_LD;                    // [64][16]   m[0..15]       (Q2_K)
    uint8_t *xdl = ms + KG_BM * DG;                   // [BN][16]   bl[0..15]      (Q2_K)
    uint8_t *xdh = xdl + BN * DG;                      // [BN][16]   bh[0..15]      (Q2_K)
    float *dws = reinterpret_cast<float *>(xdh + BN * DG);     // [64]
    float *dmws = dws + KG_BM;                        // [64]       (Q2_K)
    float *dxs = dmws + KG_BM;                        // [BN]
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // the column tiles of one row tile are neighbours in the grid (they share the weight rows)
    const int mt = (int)(blockIdx.x / (unsigned)ntn), nt = (int)(blockIdx.x - (unsigned)mt * (unsigned)ntn);
    const int m0 = mt * KG_BM, n0 = nt * BN;
    const int K = nb * QK_K;
    const int64_t rowbytes = (int64_t)nb * BS;

    // decoding lane: a quarter wave per row, lane t of the quarter owns elements 128n + 32k + 4i .. + 3, k = 0..3;
    // the quarters of a 32-lane half take rows two apart (LDS banks, header)
    const int quarter = lane >> 4, t = lane & 15, n4 = t >> 3, i = t & 7, h4 = i >> 2;
    const int rq = 2 * (quarter & 1) + (quarter >> 1);

    // (unconditional loads at clamped indices, always inside the operands)
    const uint8_t *rowp[NP];
    uint32_t odd[NP];                                  // Q3_K: row mc nb + b is at 2 mod 4 when (odd ^ b) & 1
#pragma unroll
    for (int u = 0; u < NP; u++) {
        const int m = m0 + wave * 4 * NP + 4 * u + rq;
        const int mc = m < M ? m : M - 1;
        rowp[u] = W + (int64_t)mc * rowbytes;
        odd[u] = (uint32_t)(mc & nb);
    }
    int xoff[XP];
#pragma unroll
    for (int p = 0; p < XP; p++) {
        const int pp = tid + THREADS * p, n = n0 + (pp >> 4);
        xoff[p] = (n < N ? n : N - 1) * K + (pp & 15) * 16;            // N K < 2^31 (host check)
    }
    const int dn = n0 + (tid & (BN - 1));
    const int dxoff = (dn < N ? dn : N - 1) * nb;

    struct Regs {                                      // one superblock of the tile's operands, as loaded
        uint32_t w[NP][NW];
        u32x4 x[XP];
        float dx;
    };
    auto prefetch = [&](int b, Regs &g) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < NP; u++) {
            // (pointer arithmetic, not an integer round trip: the address stays a global one, no flat load)
            const uint8_t *p = rowp[u] + b * BS;
            if constexpr (Q3) {
                const uint32_t mis = ((odd[u] ^ (uint32_t)b) & 1u) << 1;      // 0 or 2
                const uint32_t *q = reinterpret_cast<const uint32_t *>(p - mis);
                const int hi = (int)(mis >> 1);
                g.w[u][0] = q[8 + 8 * n4 + i];
                g.w[u][1] = q[8 + 8 * n4 + i + hi];
                g.w[u][2] = q[i];
                g.w[u][3] = q[i + hi];
                g.w[u][4] = q[24];
                g.w[u][5] = q[25];
                g.w[u][6] = q[26];
                g.w[u][7] = q[26 + hi];
                g.w[u][8] = *reinterpret_cast<const uint16_t *>(p + Q23<Q3>::D);
            } else {
                const uint32_t *q = reinterpret_cast<const uint32_t *>(p);
                g.w[u][0] = q[4 + 8 * n4 + i];
                g.w[u][1] = q[2 * n4];
                g.w[u][2] = q[2 * n4 + 1];
                g.w[u][3] = q[t >> 2];
                g.w[u][4] = q[20];
            }
        }
#pragma unroll
        for (int p = 0; p < XP; p++) g.x[p] = *reinterpret_cast<const u32x4 *>(xqs + xoff[p] + b * QK_K);
        g.dx = xd[dxoff + b];
    };
    // superblock b's registers -> the LDS stage at byte offset so
    auto stage = [&](int b, const Regs &g, int so) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < NP; u++) {
            const int r = wave * 4 * NP + 4 * u + rq;
            const uint32_t *a = g.w[u];
            uint32_t v[4];
            int sc[4];
            if constexpr (Q3) {
                const uint32_t mis = ((odd[u] ^ (uint32_t)b) & 1u) << 1;
                q23_values<Q3>(blk_dword(a[0], a[1], mis), blk_dword(a[2], a[3], mis), n4, v);
                q3_scales(blk_dword(a[4], a[5], mis), blk_dword(a[5], a[6], mis), blk_dword(a[6], a[7], mis), n4, h4, sc);
            } else {
                q23_values<Q3>(a[0], 0u, n4, v);
                q2_scales(a[1], a[2], h4, sc);
            }
            uint8_t *o = wq + so + r * KG_LD + 128 * n4 + 4 * i;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t s = Q3 ? (uint32_t)(-sc[k]) & 0xFFu : (uint32_t)sc[k];
                *reinterpret_cast<uint32_t *>(o + 32 * k) = q23_scaled<Q3>(v[k], s);
            }
            if constexpr (Q3) {
                if (t == 0) *reinterpret_cast<float *>(reinterpret_cast<uint8_t *>(dws + r) + so) = h2f(a[8]);
            } else {
                // lane t holds scales dword t / 4: the lanes t = 0, 4, 8, 12 store the row's sixteen m bytes
                if ((t & 3) == 0) *reinterpret_cast<uint32_t *>(ms + so + 16 * r + t) = (a[3] >> 4) & 0x0F0F0F0Fu;
                if (t == 0) {
                    *reinterpret_cast<float *>(reinterpret_cast<uint8_t *>(dws + r) + so) = h2f(a[4] & 0xFFFFu);
                    *reinterpret_cast<float *>(reinterpret_cast<uint8_t *>(dmws + r) + so) = h2f(a[4] >> 16);
                }
            }
        }
#pragma unroll
        for (int p = 0; p < XP; p++) {
            const int pp = tid + THREADS * p;
            *reinterpret_cast<u32x4 *>(xs + so + (pp >> 4) * KG_LD + (pp & 15) * 16) = g.x[p];
            if constexpr (!Q3) {
                // the piece is sub-block pp % 16 of column pp / 16: its bsum16 in [-2048, 2032] as two digits
                int s16 = __builtin_amdgcn_sdot4((int)g.x[p].x, 0x01010101, 0, false);
                s16 = __builtin_amdgcn_sdot4((int)g.x[p].y, 0x01010101, s16, false);
                s16 = __builtin_amdgcn_sdot4((int)g.x[p].z, 0x01010101, s16, false);
                s16 = __builtin_amdgcn_sdot4((int)g.x[p].w, 0x01010101, s16, false);
                xdl[so + pp] = (uint8_t)(s16 & 127);
                xdh[so + pp] = (uint8_t)(s16 >> 7);
            }
        }
        if (tid < BN) *reinterpret_cast<float *>(reinterpret_cast<uint8_t *>(dxs + tid) + so) = g.dx;
    };

    const int wr = wave & 1, wt = wave >> 1;
    const int c = lane & 31, h = lane >> 5;
    const uint8_t *b_p = wq + (32 * wr + c) * KG_LD + 16 * h;
    const uint8_t *a_p = xs + (32 * TN * wt + c) * KG_LD + 16 * h;
    const i32x16 iz = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    float acc[TN][16];
#pragma unroll
    for (int tt = 0; tt < TN; tt++)
#pragma unroll
        for (int e = 0; e < 16; e++) acc[tt][e] = 0.0f;

    // the MFMAs and the fp32 step of the superblock in the LDS stage at byte offset so
    auto compute = [&](int so) __attribute__((always_inline)) {
        const float dw = *reinterpret_cast<const float *>(reinterpret_cast<const uint8_t *>(dws + 32 * wr + c) + so);
        float dmw = 0.0f;
        long bm = 0;                                   // the row's m bytes 8h .. 8h + 7 (K slots of lane (c, h))
        if constexpr (!Q3) {
            dmw = *reinterpret_cast<const float *>(reinterpret_cast<const uint8_t *>(dmws + 32 * wr + c) + so);
            bm = *reinterpret_cast<const long *>(ms + so + 16 * (32 * wr + c) + 8 * h);
        }
        const float *dxp = reinterpret_cast<const float *>(reinterpret_cast<const uint8_t *>(dxs) + so);
#pragma unroll
        for (int tt = 0; tt < TN; tt++) {
            const int col = 32 * TN * wt + 32 * tt + c;
            i32x16 Ml = iz, Mh = iz;
            if constexpr (!Q3) {
                const long al = *reinterpret_cast<const long *>(xdl + so + 16 * col + 8 * h);
                const long ah = *reinterpret_cast<const long *>(xdh + so + 16 * col + 8 * h);
                Ml = __builtin_amdgcn_mfma_i32_32x32x16_i8(al, bm, iz, 0, 0, 0);
                Mh = __builtin_amdgcn_mfma_i32_32x32x16_i8(ah, bm, iz, 0, 0, 0);
            }
            i32x16 S = iz;
#pragma unroll
            for (int s = 0; s < QK_K / 32; s++) {
                const i32x4 a = *reinterpret_cast<const i32x4 *>(a_p + so + 32 * tt * KG_LD + 32 * s);
                const i32x4 bw = *reinterpret_cast<const i32x4 *>(b_p + so + 32 * s);
                S = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, bw, S, 0, 0, 0);
            }
            // the superblock's fp32 step per output: the GEMV's, in the GEMV's order
#pragma unroll
            for (int e = 0; e < 16; e++) {
                // (kquant_col's sum written out: through the function Q2_K's 256-column tile compiles to another schedule)
                const float dx = dxp[32 * TN * wt + 32 * tt + (e & 3) + 8 * (e >> 2) + 4 * h];
                float tb;
                if constexpr (Q3) {
                    tb = __fmul_rn(__fmul_rn(dx, dw), (float)(-S[e]));
                } else {
                    const int msum = Mh[e] * 128 + Ml[e];
                    const float negp = -__fmul_rn(__fmul_rn(dx, dmw), (float)msum);
                    tb = __builtin_fmaf(__fmul_rn(dx, dw), (float)S[e], negp);
                }
                acc[tt][e] = __fadd_rn(acc[tt][e], tb);
            }
        }
    };

    Regs g;
    prefetch(0, g);
    if constexpr (NS == 2) {
        // two stages, one barrier per superblock: a wave writes superblock b + 1 into the other stage (last read
        // for b - 1, before the previous barrier) and requests b + 2 before its MFMAs of b, so one wave's decode
        // overlaps the others' MFMAs.  No branch around the last iteration's stage and loads: it repeats superblock
        // nb - 1 into the stage nobody reads again.
        stage(0, g, 0);
        prefetch(1 < nb ? 1 : nb - 1, g);
        __syncthreads();
        for (int b = 0; b < nb; b++) {
            const int so = (b & 1) * SB;
            stage(b + 1 < nb ? b + 1 : nb - 1, g, SB - so);
            prefetch(b + 2 < nb ? b + 2 : nb - 1, g);
            compute(so);
            __syncthreads();
        }
    } else {
        // one stage: superblock b's registers -> LDS, the loads of b + 1 into the same registers, then the MFMAs
        // and the fp32 step
        for (int b = 0; b < nb; b++) {
            __syncthreads();                           // the previous superblock's LDS reads are done
            stage(b, g, 0);
            __syncthreads();
            prefetch(b + 1 < nb ? b + 1 : nb - 1, g);
            compute(0);
        }
    }

    const int row = m0 + 32 * wr + c;
    if (row < M) {
#pragma unroll
        for (int tt = 0; tt < TN; tt++)
#pragma unroll
            for (int e = 0; e < 16; e++) {
                const int n = kquant_col(n0 + 32 * TN * wt + 32 * tt, e, h);
                if (n < N) y[(int64_t)n * ldy + row] = acc[tt][e];
            }
    }
}

template <bool Q3>
static hipError_t gemm_q23_K_t(const void *W, int64_t K, int64_t M, const void *xqs, const float *xd, int64_t N, float *y,
                               int64_t ldy, int num_cus, hipStream_t s) {
    return with_kquant_tile(K, M, N, num_cus, true, [&](auto wn, auto tn, int nb) {
        constexpr int WN = decltype(wn)::value, TN = decltype(tn)::value, BN = 32 * WN * TN;
        constexpr size_t lds = (size_t)G23_stages(TN) * G23_stage_bytes<Q3>(BN);
        return launch_gemm_kquant<k_gemm_q23_K<Q3, WN, TN>, WN, TN>(lds, M, N, [&](dim3 grid, dim3 block, int ntn) {
            launch_k(k_gemm_q23_K<Q3, WN, TN>, grid, block, lds, s, (const uint8_t *)W, nb, (int)M, (const uint8_t *)xqs,
                     xd, (int)N, ntn, y, ldy);
        });
    });
}

// y[n * ldy + m] = W[m] . x[n] on the planes quantize_q8_K_planes wrote; any K % 256 == 0, M, N >= 1
hipError_t gemm_q23_K(bool q3, const void *W, int64_t K, int64_t M, const void *xqs, const float *xd, int64_t N, float *y,
                      int64_t ldy, const DeviceInfo &dev, hipStream_t s) {
    return q3 ? gemm_q23_K_t<true>(W, K, M, xqs, xd, N, y, ldy, dev.num_cus, s)
              : gemm_q23_K_t<false>(W, K, M, xqs, xd, N, y, ldy, dev.num_cus, s);
}

}  // namespace ghip
