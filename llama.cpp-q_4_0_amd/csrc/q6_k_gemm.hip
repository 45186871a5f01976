// q6_k_gemm.hip — the prefill GEMM of the Q6_K x F32 mul_mat (gfx950, wave64): k_gemm_q6_K on the int8 matrix
// cores (v_mfma_i32_32x32x32_i8), y bit for bit what the GEMV k_gemv_q6_K (q6_k.hip) gives.
//
// The GEMV computes, per output and superblock b of 256 elements, the exact int32
//   isum_b = sum_g sc[g] sum_(e in g) (q_e - 32) q8_e,   |isum_b| <= 2^27,
// and then acc = fmaf(d_x[n][b] * d_w[m][b], (float)isum_b, acc), superblocks in order from +0: ONE fp32 step per
// 256 weights.  Q6_K's scales are integers, so the scaled weight w' = sc (q - 32) is an integer in
// [-4064, 4096] and splits exactly into two int8 digits, w' = 128 hi + lo with lo in [-64, 63], hi in [-32, 32].
// Two MFMA chains over the superblock's K = 256, hi . q8 and lo . q8, accumulate H (|H| <= 2^20) and
// L (|L| <= 2^21) in int32 with nothing in between; isum_b = 128 H + L exactly, and the fp32 step that follows
// is the GEMV's, in the GEMV's order (K is never split across waves or workgroups).  Hence equality, not a
// tolerance, and a result that does not depend on the tile shape or the grid.
//
// Weights are read in place (no image): the workgroup decodes its 64-row tile's superblock into the two digit
// planes in LDS once, and every column of the tile reuses it.  The block fields are fetched as in the GEMV: the
// 53 naturally aligned dwords that hold a 210-byte block are one coalesced load per wave, a wave shift and
// v_alignbyte_b32 realign a block at 2 mod 4, three ds_bpermute_b32 hand lane t the ql / qh / scale of its
// elements 4t .. 4t + 3.  Rows >= M and columns >= N of a ragged tile read the last row / column (inside the
// operands) and are never stored.  x is the q8_K quantization (q8k_block_lane, the GEMV prologue's bits) written
// as planes: qs int8 [N][K] and d f32 [N][K / 256] (k_quantize_q8_K_planes), so that a column's superblock is
// sixteen aligned 16-byte loads.
//
// Tile: 64 rows x 32 WN TN columns, 2 x WN waves, each TN 32 x 32 MFMA tiles with their H and L ((WN, TN) =
// (2, 1) up to N = 64, (4, 1) up to 128, else (4, 2): the wider the tile, the more columns share one decode of
// the weights); MFMA A = x (D's register index = column), B = weights (D's lane = row): a lane's 16 accumulator
// registers are 16 columns of ONE row, so d_w is one value per lane and the y stores run along m.  LDS rows are
// 256 + 16 bytes, which spreads the 32 rows of an operand read (16 bytes per lane) over all banks.  One superblock
// per stage in a single LDS buffer; the next superblock's global loads are issued before the current one's MFMAs.
#include "kquant_gemm.h"

namespace ghip {

typedef short s16x2 __attribute__((ext_vector_type(2)));

// x as the planes of kquant_gemm.h; dig null: none (only Q5_K / Q4_K read one)
hipError_t quantize_q8_K_planes(const float *x, int64_t K, int64_t N, void *qs, float *xd, void *dig, hipStream_t s) {
    const int64_t nblocks = N * (K / QK_K);
    if (dig) return launch_1d(k_quantize_q8_K_planes<true>, nblocks, 4, s, x, nblocks, (uint32_t *)qs, xd, (int8_t *)dig);
    return launch_1d(k_quantize_q8_K_planes<false>, nblocks, 4, s, x, nblocks, (uint32_t *)qs, xd, (int8_t *)nullptr);
}

// four 6-bit values (one per byte) and their scale -> the int8 digits of w' = sc (q - 32) = 128 hi + lo, packed
// in element order.  Elements 0, 2 and 1, 3 go through 16-bit pairs: lo = ((w' + 64) & 127) - 64 in [-64, 63],
// hi = (w' - lo) >> 7 in [-32, 32]; v_perm_b32 interleaves the pairs' low bytes (selector bytes 0..3 name the
// bytes of the second operand, 4..7 those of the first).
__device__ __forceinline__ void q6_digits(uint32_t q6, int sc, uint32_t &hi, uint32_t &lo) {
    const s16x2 s = {(short)sc, (short)sc};
    const s16x2 c32 = {32, 32}, c64 = {64, 64}, c127 = {127, 127}, c7 = {7, 7};
    const uint32_t ev_u = q6 & 0x00FF00FFu, od_u = (q6 >> 8) & 0x00FF00FFu;
    s16x2 ev, od;
    __builtin_memcpy(&ev, &ev_u, 4);
    __builtin_memcpy(&od, &od_u, 4);
    const s16x2 we = (ev - c32) * s, wo = (od - c32) * s;
    const s16x2 le = ((we + c64) & c127) - c64, lod = ((wo + c64) & c127) - c64;
    const s16x2 he = (we - le) >> c7, hod = (wo - lod) >> c7;
    uint32_t le_u, lo_u, he_u, ho_u;
    __builtin_memcpy(&le_u, &le, 4);
    __builtin_memcpy(&lo_u, &lod, 4);
    __builtin_memcpy(&he_u, &he, 4);
    __builtin_memcpy(&ho_u, &hod, 4);
    lo = __builtin_amdgcn_perm(lo_u, le_u, 0x06020400u);
    hi = __builtin_amdgcn_perm(ho_u, he_u, 0x06020400u);
}

template <int WN, int TN>
__global__ __launch_bounds__(128 * WN) void k_gemm_q6_K(const uint8_t *__restrict__ W, int nb, int M,
                                                         const uint8_t *__restrict__ xqs, const float *__restrict__ xd,
                                                         int N, int ntn, float *__restrict__ y, int64_t ldy) {
    constexpr int THREADS = 128 * WN;                  // 2 x WN waves
    constexpr int BN = 32 * WN * TN;                   // columns per workgroup
    constexpr int RPW = KG_BM / (2 * WN);              // rows a wave decodes per superblock
    constexpr int XP = BN * 16 / THREADS;              // 16-byte pieces of the x tile per thread (4 TN)
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint8_t *whi = smem;                               // [64][KG_LD]
    uint8_t *wlo = whi + KG_BM * KG_LD;                // [64][KG_LD]
    uint8_t *xs = wlo + KG_BM * KG_LD;                 // [BN][KG_LD]
    float *dws = reinterpret_cast<float *>(xs + BN * KG_LD);   // [64]
    float *dxs = dws + KG_BM;                          // [BN]
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // the column tiles of one row tile are neighbours in the grid (they share the weight rows)
    const int mt = (int)(blockIdx.x / (unsigned)ntn), nt = (int)(blockIdx.x - (unsigned)mt * (unsigned)ntn);
    const int m0 = mt * KG_BM, n0 = nt * BN;
    const int K = nb * QK_K;
    const int64_t rowbytes = (int64_t)nb * Q6KB;

    // lane t of the decoding wave owns elements 4t .. 4t + 3 of a superblock: group (h, j), one scale
    const int eh = lane >> 5, ej = (lane >> 3) & 3, ei = lane & 7;
    const int ql_src = 4 * (16 * eh + 8 * (ej & 1) + ei), ql_sh = 4 * (ej >> 1);   // byte address of the source lane
    const int qh_src = 4 * (32 + 8 * eh + ei), qh_sh = 2 * ej;
    const int sc_idx = 8 * eh + 2 * ej + (ei >> 2);
    const int sc_src = 4 * (48 + (sc_idx >> 2)), sc_sh = 8 * (sc_idx & 3);
    const int ld_lane = lane < 53 ? lane : 52;

    // (unconditional loads at clamped indices, always inside the operands)
    const uint8_t *rowp[RPW];
#pragma unroll
    for (int u = 0; u < RPW; u++) {
        const int m = m0 + wave * RPW + u;
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
        uint32_t w[RPW];
        u32x4 x[XP];
        float dx;
    };
    auto prefetch = [&](int b, Regs &g) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < RPW; u++) {
            // (pointer arithmetic, not an integer round trip: the address stays a global one, no flat load)
            const uint8_t *p = rowp[u] + b * Q6KB;
            g.w[u] = reinterpret_cast<const uint32_t *>(p - ((uintptr_t)p & 3))[ld_lane];
        }
#pragma unroll
        for (int i = 0; i < XP; i++) g.x[i] = *reinterpret_cast<const u32x4 *>(xqs + xoff[i] + b * QK_K);
        g.dx = xd[dxoff + b];
    };
    auto stage = [&](int b, const Regs &g) __attribute__((always_inline)) {   // registers of superblock b -> LDS
        uint32_t dwv = 0;                              // lane u: the fp16 d of the wave's row u
        // (no branch per row: the rows' cross-lane round trips must overlap)
#pragma unroll
        for (int u = 0; u < RPW; u++) {
            const int r = wave * RPW + u;
            const uintptr_t a = (uintptr_t)(rowp[u] + b * Q6KB);
            const uint32_t raw = g.w[u];
            const uint32_t nx = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)raw, DPP_WAVE_SHL1, 0xF, 0xF, false);
            const uint32_t own = (a & 2) ? __builtin_amdgcn_alignbyte(nx, raw, 2) : raw;
            const uint32_t ql = (uint32_t)__builtin_amdgcn_ds_bpermute(ql_src, (int)own) >> ql_sh;
            const uint32_t qh = (uint32_t)__builtin_amdgcn_ds_bpermute(qh_src, (int)own) >> qh_sh;
            const int sc = (int)(int8_t)((uint32_t)__builtin_amdgcn_ds_bpermute(sc_src, (int)own) >> sc_sh);
            const uint32_t dw = (uint32_t)__builtin_amdgcn_readlane((int)own, 52);
            dwv = lane == u ? dw : dwv;
            uint32_t hi, lo;
            q6_digits((ql & 0x0F0F0F0Fu) | ((qh & 0x03030303u) << 4), sc, hi, lo);
            *reinterpret_cast<uint32_t *>(whi + r * KG_LD + 4 * lane) = hi;
            *reinterpret_cast<uint32_t *>(wlo + r * KG_LD + 4 * lane) = lo;
        }
        if (lane < RPW) dws[wave * RPW + lane] = h2f(dwv);
#pragma unroll
        for (int i = 0; i < XP; i++) {
            const int p = tid + THREADS * i;
            *reinterpret_cast<u32x4 *>(xs + (p >> 4) * KG_LD + (p & 15) * 16) = g.x[i];
        }
        if (tid < BN) dxs[tid] = g.dx;
    };

    const int wr = wave & 1, wt = wave >> 1;
    const int c = lane & 31, h = lane >> 5;
    const uint8_t *bh_p = whi + (32 * wr + c) * KG_LD + 16 * h;
    const uint8_t *bl_p = wlo + (32 * wr + c) * KG_LD + 16 * h;
    const uint8_t *a_p = xs + (32 * TN * wt + c) * KG_LD + 16 * h;
    const i32x16 iz = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    float acc[TN][16];
#pragma unroll
    for (int t = 0; t < TN; t++)
#pragma unroll
        for (int i = 0; i < 16; i++) acc[t][i] = 0.0f;

    // superblock b: its registers -> LDS, the loads of b + 1 into the same registers, then the MFMAs and the
    // fp32 step.  (Loading two superblocks ahead measured the same: the stage is bound by instruction issue.)
    Regs g;
    prefetch(0, g);
    for (int b = 0; b < nb; b++) {
        __syncthreads();                               // the previous superblock's LDS reads are done
        stage(b, g);
        __syncthreads();
        prefetch(b + 1 < nb ? b + 1 : nb - 1, g);
        i32x16 H[TN], L[TN];
#pragma unroll
        for (int t = 0; t < TN; t++) H[t] = L[t] = iz;
#pragma unroll
        for (int s = 0; s < QK_K / 32; s++) {
            const i32x4 bh = *reinterpret_cast<const i32x4 *>(bh_p + 32 * s);
            const i32x4 bl = *reinterpret_cast<const i32x4 *>(bl_p + 32 * s);
#pragma unroll
            for (int t = 0; t < TN; t++) {
                const i32x4 a = *reinterpret_cast<const i32x4 *>(a_p + 32 * t * KG_LD + 32 * s);
                H[t] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, bh, H[t], 0, 0, 0);
                L[t] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, bl, L[t], 0, 0, 0);
            }
        }
        // the superblock's one fp32 step per output: the GEMV's, in the GEMV's order
        const float dw = dws[32 * wr + c];
#pragma unroll
        for (int t = 0; t < TN; t++)
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const int tok = kquant_col(32 * TN * wt + 32 * t, i, h);
                const int isum = H[t][i] * 128 + L[t][i];
                acc[t][i] = __builtin_fmaf(dxs[tok] * dw, (float)isum, acc[t][i]);
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

// y[n * ldy + m] = W[m] . x[n] on the planes quantize_q8_K_planes wrote; any K % 256 == 0, M, N >= 1.  The 256-column
// tile for every N > 128 (no fit rule).
hipError_t gemm_q6_K(const void *W, int64_t K, int64_t M, const void *xqs, const float *xd, int64_t N, float *y,
                     int64_t ldy, const DeviceInfo &dev, hipStream_t s) {
    return with_kquant_tile(K, M, N, dev.num_cus, false, [&](auto wn, auto tn, int nb) {
        constexpr int WN = decltype(wn)::value, TN = decltype(tn)::value, BN = 32 * WN * TN;
        constexpr size_t lds = (size_t)(2 * KG_BM + BN) * KG_LD + (size_t)(KG_BM + BN) * 4;
        return launch_gemm_kquant<k_gemm_q6_K<WN, TN>, WN, TN>(lds, M, N, [&](dim3 grid, dim3 block, int ntn) {
            launch_k(k_gemm_q6_K<WN, TN>, grid, block, lds, s, (const uint8_t *)W, nb, (int)M, (const uint8_t *)xqs, xd,
                     (int)N, ntn, y, ldy);
        });
    });
}

}  // namespace ghip
