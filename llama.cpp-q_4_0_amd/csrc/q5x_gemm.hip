// q5x_gemm.hip — the prefill GEMM of the Q4_1 / Q5_1 x F32 mul_mat (gfx950, wave64): k_gemm_q5x1 on the int8
// matrix cores, one template parameter QH (true: Q5_1, false: Q4_1).  Q5_0 has no part in it: its activations are
// q8_0 and it takes k_gemm8 (blk32_w.hip).
//
// Per output y[n][m], from acc = +0, the blocks b = 0 .. K / 32 - 1 of 32 elements in order:
//   acc = fmaf((float)isum_b, d_w[m][b] * d_x[n][b], acc)        (the product one rounded f32 multiply)
//   acc = fmaf(m_w[m][b], s_x[n][b], acc)
// isum_b = sum q q8 over the block, q the UNSIGNED 0..15 / 0..31 used as int8 and q8 the q8_1 byte: one
// v_mfma_i32_32x32x32_i8 spans exactly one block, so isum_b comes off the matrix core as an exact int32 (at most
// 32 * 31 * 127 < 2^17, exact in fp32); d_x = amax / 127 unrounded and s_x = d_x * (float)sum q8 are
// quantize_q8_1_soa's planes (the bits of quantize_row_q8_1).  This is the per-block step of the GEMV (k_gemv_blk32):
// a block's two large, opposite terms stay adjacent.  It runs as ONE chain per output, where the GEMV runs 64 lane
// chains and a tree, so y is not bitwise the GEMV's (it is within the parity bound of it, as Q8_0's and Q5_0's
// GEMMs are of their GEMVs).  K is never split across waves or workgroups, so y depends on nothing but (row,
// column, K): not on the tile shape, the grid, M, N or a column's position in the call.
//
// Weights are read in place (no image, no workspace of their own).  K % 64 == 0 and nothing more: a row is a whole
// number of block PAIRS of 40 / 48 bytes, 4-byte aligned and nothing more (load_pairx, blk32_device.h).  A stage is
// G5G_SP = 4 pairs = 256 elements: the first 256 threads of the workgroup each load one (row, pair) of the 64-row
// tile (the four pairs of a row on neighbouring lanes: 160 / 192 contiguous bytes), decode it (q5x_decode_pair) and
// store the 64 bytes in element order into the LDS plane, with d_w and m_w of the two blocks as f32 beside it; every
// column of the tile reuses the decode.  The last stage of K = 4160 (65 pairs) holds one pair: the loads of the
// others are clamped to the row's last pair / the x row's last bytes, and their blocks are not part of the chain
// (the block loop ends at the stage's count).  Rows >= M and columns >= N of a ragged tile read the last row /
// column (inside the operands) and are never stored.
//
// Tile: 64 rows x 32 WN TN columns, 2 x WN waves, each TN 32 x 32 MFMA tiles, (WN, TN) by gemm_tile_columns' fit rule
// (launch.h); MFMA A = x (D's register index = column), B = weights (D's lane = row), so d_w and m_w are one
// value each per lane and block and the y stores run along m.  LDS: the int8 rows are 256 + 16 bytes (row c starts
// at bank 4c mod 64: the 32 rows of a ds_read_b128 operand read spread over all banks); d_w / m_w are [8][64] and
// d_x / s_x [8][BN] f32, block-major, so a lane's d_w is conflict-free and the four columns of a D register group
// are one ds_read_b128 (two addresses per wave: a broadcast).  One stage in a single LDS buffer; the next stage's
// global loads are issued before the current one's MFMAs.
#include "blk32_device.h"

namespace ghip {

static constexpr int G5G_BM = 64;                      // rows per workgroup
static constexpr int G5G_SP = 4;                       // block pairs per stage
static constexpr int G5G_SB = 2 * G5G_SP;              // blocks per stage
static constexpr int G5G_SK = 32 * G5G_SB;             // elements per stage
static constexpr int G5G_LD = G5G_SK + 16;             // LDS row pitch of the int8 planes

typedef float g5g_f32x2 __attribute__((ext_vector_type(2)));
typedef float g5g_f32x4 __attribute__((ext_vector_type(4)));

template <bool QH, int WN, int TN>
__global__ __launch_bounds__(128 * WN) void k_gemm_q5x1(const uint8_t *__restrict__ W, int nb, int M,
                                                         const uint8_t *__restrict__ xqs, const float *__restrict__ xd,
                                                         const float *__restrict__ xsum, int N, int ntn,
                                                         float *__restrict__ y, int64_t ldy) {
    using T = Q5x<QH, true>;
    typedef PairX<T::DW> Pair;
    constexpr int THREADS = 128 * WN;                  // 2 x WN waves
    constexpr int BN = 32 * WN * TN;                   // columns per workgroup
    constexpr int XP = BN * (G5G_SK / 16) / THREADS;   // 16-byte pieces of the x tile per thread (4 TN)
    constexpr int SP = BN * (G5G_SB / 2) / THREADS;    // block pairs of the d_x / s_x tile per thread (TN)
    static_assert(G5G_BM * G5G_SP == 256 && THREADS >= 256, "one (row, pair) per thread of the first four waves");
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint8_t *ws = smem;                                // [64][G5G_LD]
    uint8_t *xs = ws + G5G_BM * G5G_LD;                // [BN][G5G_LD]
    float *dws = reinterpret_cast<float *>(xs + BN * G5G_LD);  // [8][64]
    float *mws = dws + G5G_SB * G5G_BM;                // [8][64]
    float *dxs = mws + G5G_SB * G5G_BM;                // [8][BN]
    float *sxs = dxs + G5G_SB * BN;                    // [8][BN]
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // the column tiles of one row tile are neighbours in the grid (they share the weight rows)
    const int mt = (int)(blockIdx.x / (unsigned)ntn), nt = (int)(blockIdx.x - (unsigned)mt * (unsigned)ntn);
    const int m0 = mt * G5G_BM, n0 = nt * BN;
    const int K = nb * 32, npairs = nb >> 1;
    const int nstage = (npairs + G5G_SP - 1) / G5G_SP;
    const bool decoder = wave < 4;                     // wave-uniform

    // (unconditional loads at clamped indices, always inside the operands)
    const int drow = (tid >> 2) & (G5G_BM - 1), dpair = tid & 3;
    const uint8_t *rowp;
    {
        const int m = m0 + drow;
        rowp = W + (int64_t)(m < M ? m : M - 1) * ((int64_t)nb * T::BLK);
    }
    int xrow[XP];                                      // N K < 2^31 (host check)
#pragma unroll
    for (int p = 0; p < XP; p++) {
        const int n = n0 + ((tid + THREADS * p) >> 4);
        xrow[p] = (n < N ? n : N - 1) * K;
    }
    int srow[SP];
#pragma unroll
    for (int p = 0; p < SP; p++) {
        const int n = n0 + ((tid + THREADS * p) >> 2);
        srow[p] = (n < N ? n : N - 1) * nb;
    }

    struct Regs {                                      // one stage of the tile's operands, as loaded
        Pair w;
        u32x4 x[XP];
        g5g_f32x2 d[SP], s[SP];
    };
    auto prefetch = [&](int st, Regs &g) __attribute__((always_inline)) {
        if (decoder) {
            const int pr = G5G_SP * st + dpair;
            g.w = load_pairx<T::DW>(rowp + (int64_t)(pr < npairs ? pr : npairs - 1) * T::PAIR);
        }
#pragma unroll
        for (int p = 0; p < XP; p++) {
            const int k = G5G_SK * st + ((tid + THREADS * p) & 15) * 16;
            g.x[p] = *reinterpret_cast<const u32x4 *>(xqs + xrow[p] + (k < K ? k : K - 16));
        }
#pragma unroll
        for (int p = 0; p < SP; p++) {                 // nb is even: the pair of floats is 8-byte aligned
            const int b = G5G_SB * st + 2 * ((tid + THREADS * p) & 3);
            const int o = srow[p] + (b < nb ? b : nb - 2);
            g.d[p] = *reinterpret_cast<const g5g_f32x2 *>(xd + o);
            g.s[p] = *reinterpret_cast<const g5g_f32x2 *>(xsum + o);
        }
    };
    auto stage = [&](const Regs &g) __attribute__((always_inline)) {           // a stage's registers -> LDS
        if (decoder) {
            BlockX A, B;
            q5x_decode_pair<QH, true>(g.w, A, B);
            u32x4 *dst = reinterpret_cast<u32x4 *>(ws + drow * G5G_LD + 64 * dpair);
            dst[0] = u32x4{A.q[0], A.q[1], A.q[2], A.q[3]};
            dst[1] = u32x4{A.q[4], A.q[5], A.q[6], A.q[7]};
            dst[2] = u32x4{B.q[0], B.q[1], B.q[2], B.q[3]};
            dst[3] = u32x4{B.q[4], B.q[5], B.q[6], B.q[7]};
            dws[(2 * dpair) * G5G_BM + drow] = A.d;
            dws[(2 * dpair + 1) * G5G_BM + drow] = B.d;
            mws[(2 * dpair) * G5G_BM + drow] = A.m;
            mws[(2 * dpair + 1) * G5G_BM + drow] = B.m;
        }
#pragma unroll
        for (int p = 0; p < XP; p++) {
            const int pp = tid + THREADS * p;
            *reinterpret_cast<u32x4 *>(xs + (pp >> 4) * G5G_LD + (pp & 15) * 16) = g.x[p];
        }
#pragma unroll
        for (int p = 0; p < SP; p++) {
            const int pp = tid + THREADS * p, col = pp >> 2, b = 2 * (pp & 3);
            dxs[b * BN + col] = g.d[p].x;
            dxs[(b + 1) * BN + col] = g.d[p].y;
            sxs[b * BN + col] = g.s[p].x;
            sxs[(b + 1) * BN + col] = g.s[p].y;
        }
    };

    const int wr = wave & 1, wt = wave >> 1;
    const int c = lane & 31, h = lane >> 5;
    const uint8_t *b_p = ws + (32 * wr + c) * G5G_LD + 16 * h;
    const uint8_t *a_p = xs + (32 * TN * wt + c) * G5G_LD + 16 * h;
    const float *dw_p = dws + 32 * wr + c, *mw_p = mws + 32 * wr + c;
    const float *dx_p = dxs + 32 * TN * wt + 4 * h, *sx_p = sxs + 32 * TN * wt + 4 * h;
    const i32x16 iz = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    float acc[TN][16];
#pragma unroll
    for (int tt = 0; tt < TN; tt++)
#pragma unroll
        for (int e = 0; e < 16; e++) acc[tt][e] = 0.0f;

    // stage st: its registers -> LDS, the loads of st + 1 into the same registers, then per block the MFMA and the
    // fp32 step (two and three stages of loads in flight measured 15 - 25 % slower on the LLaMA-7B shapes with
    // M = 4096: load latency is not what a stage waits for)
    Regs g;
    prefetch(0, g);
    for (int st = 0; st < nstage; st++) {
        __syncthreads();                               // the previous stage's LDS reads are done
        stage(g);
        __syncthreads();
        prefetch(st + 1 < nstage ? st + 1 : nstage - 1, g);
        const int left = nb - G5G_SB * st;             // the blocks of this stage that exist
#pragma unroll
        for (int s = 0; s < G5G_SB; s++) {
            if (s >= left) break;                      // workgroup-uniform
            const float dw = dw_p[s * G5G_BM], mw = mw_p[s * G5G_BM];
            const i32x4 b = *reinterpret_cast<const i32x4 *>(b_p + 32 * s);
#pragma unroll
            for (int tt = 0; tt < TN; tt++) {
                const i32x4 a = *reinterpret_cast<const i32x4 *>(a_p + 32 * tt * G5G_LD + 32 * s);
                const i32x16 I = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b, iz, 0, 0, 0);
                // D register e = 4 g + k holds column k + 8 g + 4 h of the 32 x 32 tile
#pragma unroll
                for (int gq = 0; gq < 4; gq++) {
                    const g5g_f32x4 dx = *reinterpret_cast<const g5g_f32x4 *>(dx_p + s * BN + 32 * tt + 8 * gq);
                    const g5g_f32x4 sx = *reinterpret_cast<const g5g_f32x4 *>(sx_p + s * BN + 32 * tt + 8 * gq);
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const int e = 4 * gq + k;
                        float a1 = __builtin_fmaf((float)I[e], __fmul_rn(dw, dx[k]), acc[tt][e]);
                        acc[tt][e] = __builtin_fmaf(mw, sx[k], a1);
                    }
                }
            }
        }
    }

    const int row = m0 + 32 * wr + c;
    if (row < M) {
#pragma unroll
        for (int tt = 0; tt < TN; tt++)
#pragma unroll
            for (int e = 0; e < 16; e++) {
                const int n = n0 + 32 * TN * wt + 32 * tt + (e & 3) + 8 * (e >> 2) + 4 * h;
                if (n < N) y[(int64_t)n * ldy + row] = acc[tt][e];
            }
    }
}

template <bool QH, int WN, int TN>
static hipError_t launch_gemm5x1(const uint8_t *W, int nb, int M, const uint8_t *xqs, const float *xd, const float *xsum,
                                 int N, float *y, int64_t ldy, hipStream_t s) {
    constexpr int BN = 32 * WN * TN;
    constexpr size_t lds = (size_t)(G5G_BM + BN) * G5G_LD + (size_t)(2 * G5G_BM + 2 * BN) * G5G_SB * 4;
    if (const hipError_t e = raise_dynamic_lds<k_gemm_q5x1<QH, WN, TN>>((int)lds); e != hipSuccess) return e;
    const int64_t ntm = ((int64_t)M + G5G_BM - 1) / G5G_BM, ntn = ((int64_t)N + BN - 1) / BN;
    if (ntm * ntn >= ((int64_t)1 << 31)) return hipErrorInvalidValue;
    (void)hipGetLastError();  // report only this launch's error
    launch_k(k_gemm_q5x1<QH, WN, TN>, dim3((unsigned)(ntm * ntn)), dim3(128 * WN), lds, s, W, nb, M, xqs, xd, xsum, N,
             (int)ntn, y, ldy);
    return hipGetLastError();
}

template <bool QH>
static hipError_t gemm_q5x1_t(const void *W, int64_t K, int64_t M, const int8_t *xqs, const float *xd, const float *xsum,
                              int64_t N, float *y, int64_t ldy, int num_cus, hipStream_t s) {
    if (K <= 0 || K % 64 || M < 1 || M >= ((int64_t)1 << 30) || N < 1 || N * K >= ((int64_t)1 << 31))
        return hipErrorInvalidValue;
    const int nb = (int)(K / 32);
    const uint8_t *w = (const uint8_t *)W, *q = (const uint8_t *)xqs;
    switch (gemm_tile_columns(M, N, num_cus, true)) {
        case 64: return launch_gemm5x1<QH, 2, 1>(w, nb, (int)M, q, xd, xsum, (int)N, y, ldy, s);
        case 128: return launch_gemm5x1<QH, 4, 1>(w, nb, (int)M, q, xd, xsum, (int)N, y, ldy, s);
        default: return launch_gemm5x1<QH, 4, 2>(w, nb, (int)M, q, xd, xsum, (int)N, y, ldy, s);
    }
}

// y[n * ldy + m] = W[m] . x[n] on the planes quantize_q8_1_soa wrote (qs 16-byte, d and s 8-byte aligned); any
// K % 64 == 0, M, N >= 1
hipError_t gemm_q5x1(bool qh, const void *W, int64_t K, int64_t M, const int8_t *xqs, const float *xd, const float *xsum,
                     int64_t N, float *y, int64_t ldy, const DeviceInfo &dev, hipStream_t s) {
    return qh ? gemm_q5x1_t<true>(W, K, M, xqs, xd, xsum, N, y, ldy, dev.num_cus, s)
              : gemm_q5x1_t<false>(W, K, M, xqs, xd, xsum, N, y, ldy, dev.num_cus, s);
}

}  // namespace ghip
