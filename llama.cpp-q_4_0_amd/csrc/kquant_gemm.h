// kquant_gemm.h — what the prefill GEMMs of the five k-quants share (k_gemm_q6_K in q6_k_gemm.hip, k_gemm_q45_K in
// q45_k_gemm.hip, k_gemm_q23_K in q23_k_gemm.hip; gfx950, wave64, the int8 matrix cores): the tile geometry, the
// accumulator-to-column map, the x quantizer, and on the host the launch, the K / M / N check and the tile choice.
// The kernels' bodies are not shared.  One template over per-type traits was built and measured: y was the same bits,
// but the compiler scheduled the same arithmetic differently and a third of the (type, shape, N) cells left the old
// kernels' spread, up to +9 % (Q5_K, 128 columns).  These kernels' schedules follow the order of the source
// statements: moving one declaration, or the x clamps or the y store into an inline function, already changes them.
// So only pieces that leave every instantiation's instructions as they were are shared, which was checked by
// comparing the compiled kernels with those of the text written out.
//
// Tile: 64 rows x 32 WN TN columns, 2 x WN waves, each TN 32 x 32 MFMA tiles ((WN, TN) = (2, 1) up to N = 64, then
// (4, 1) or (4, 2) by gemm_tile_columns, launch.h: the wider the tile, the more columns share one decode of the
// weights); MFMA A = x (D's register index = column, kquant_col), B = weights (D's lane = row): a lane's 16
// accumulator registers are 16 columns of ONE row, so d and dmin are one value each per lane and the y stores run
// along m.  Rows >= M and columns >= N of a ragged tile read the last row / column (inside the operands) and are
// never stored.  LDS: the int8 plane and x rows are 256 + 16 bytes (KG_LD), which spreads the 32 rows of an operand
// read (ds_read_b128, 16 bytes per lane, banks mod 64 in groups of 16 lanes) over all 64 banks: row c starts at bank
// 4c mod 64, and the 16 lanes of a group have 16 distinct c mod 16.  x is the q8_K quantization (q8k_block_lane, the
// GEMV prologue's bits) written once per call as planes by k_quantize_q8_K_planes: qs int8 [N][K] and d f32
// [N][K / 256], so that a column's superblock is sixteen aligned 16-byte loads; with DIGITS also dig int8
// [N][K / 256][16], the eight low then the eight high base-128 digits of the (token, superblock)'s sums of 32.
#pragma once
#include "q6_k_device.h"

namespace ghip {

static constexpr int KG_BM = 64;                       // rows per workgroup
static constexpr int KG_LD = QK_K + 16;                // LDS row pitch of the int8 planes

// x f32 [N][K] -> qs int8 [N][K] + d f32 [N][K / 256] (+ dig int8 [N][K / 256][16]); one wave per block, the values
// of the GEMV prologue (q8k_block_lane, group8_sum of the lane's four q8)
template <bool DIGITS>
__global__ __launch_bounds__(256) void k_quantize_q8_K_planes(const float *__restrict__ x, int64_t nblocks,
                                                               uint32_t *__restrict__ qs, float *__restrict__ xd,
                                                               int8_t *__restrict__ dig) {
    const int lane = threadIdx.x & 63;
    const int64_t blk = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (blk >= nblocks) return;                      // wave-uniform
    const float4 v = reinterpret_cast<const float4 *>(x)[blk * 64 + lane];
    float d;
    const uint32_t p = q8k_block_lane(v, lane, d);
    qs[blk * 64 + lane] = p;
    if constexpr (DIGITS) {
        const int s32 = group8_sum(__builtin_amdgcn_sdot4((int)p, 0x01010101, 0, false));   // [-4096, 4064]
        if ((lane & 7) == 0) {
            dig[blk * 16 + (lane >> 3)] = (int8_t)(s32 & 127);
            dig[blk * 16 + 8 + (lane >> 3)] = (int8_t)(s32 >> 7);
        }
    }
    if (lane == 0) xd[blk] = d;
}

// col0 + the column of accumulator register e in lane half h of a 32 x 32 MFMA tile (one sum, in this order)
__device__ __forceinline__ int kquant_col(int col0, int e, int h) { return col0 + (e & 3) + 8 * (e >> 2) + 4 * h; }

// the launch of one (WN, TN) instantiation: its LDS raised once per device, one workgroup per 64 x 32 WN TN tile, the
// column tiles of one row tile neighbours in the grid; launch(grid, block, ntn) issues the kernel with its arguments
template <auto Kernel, int WN, int TN, class F>
static hipError_t launch_gemm_kquant(size_t lds, int64_t M, int64_t N, F &&launch) {
    constexpr int BN = 32 * WN * TN;
    if (const hipError_t e = raise_dynamic_lds<Kernel>((int)lds); e != hipSuccess) return e;
    const int64_t ntm = (M + KG_BM - 1) / KG_BM, ntn = (N + BN - 1) / BN;
    if (ntm * ntn >= ((int64_t)1 << 31)) return hipErrorInvalidValue;
    (void)hipGetLastError();  // report only this launch's error
    launch(dim3((unsigned)(ntm * ntn)), dim3(128 * WN), (int)ntn);
    return hipGetLastError();
}

// any K % 256 == 0 (N K < 2^31), M, N >= 1: f(WN, TN as integral constants, K / 256) on the tile gemm_tile_columns picks
template <class F>
static hipError_t with_kquant_tile(int64_t K, int64_t M, int64_t N, int num_cus, bool fit_rule, F &&f) {
    if (K <= 0 || K % QK_K || M < 1 || M >= ((int64_t)1 << 31) || N < 1 || N * K >= ((int64_t)1 << 31))
        return hipErrorInvalidValue;
    const int nb = (int)(K / QK_K);
    using std::integral_constant;
    switch (gemm_tile_columns(M, N, num_cus, fit_rule)) {
        case 64: return f(integral_constant<int, 2>{}, integral_constant<int, 1>{}, nb);
        case 128: return f(integral_constant<int, 4>{}, integral_constant<int, 1>{}, nb);
        default: return f(integral_constant<int, 4>{}, integral_constant<int, 2>{}, nb);
    }
}

}  // namespace ghip
