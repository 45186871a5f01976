// q6_k.hip — the Q6_K x F32 mul_mat of a k-quants model's output.weight (gfx950, wave64): the q8_K
// quantizer, the Q6_K dequantizer, the fused GEMV (N <= 8 per launch) and the exact kernel.
// Shared device helpers: q4_0_device.h, q6_k_device.h (shared with the prefill GEMM, q6_k_gemm.hip).  What each
// kernel restates (reference = k_quants.c of Fcucgvhhhvjv/llama.cpp-q_4_0, QK_K = 256):
//   k_quantize_q8_K    quantize_row_q8_K_reference k_quants.c:1133-1168 (bit-exact)
//   k_dequantize_q6_K  dequantize_row_q6_K k_quants.c:1065-1110 (bit-exact)
//   k_gemv_q6_K<NT>    ggml_vec_dot_q6_K_q8_K with the q8_K quantization of x fused into the prologue
//                      (LDS, once per workgroup), one wave64 per weight row; y within the parity bound
//   k_mm_exact_q6_K    the AVX2 branch k_quants.c:3484-3561, bit for bit
//
// Layouts: block_q6_K = ql[128] | qh[64] | int8 scales[16] | fp16 d (210 bytes); element e = 128h + 32j + l
// (h = 0..1, j = 0..3, l = 0..31) is nibble j >> 1 of ql[64h + 32(j & 1) + l] with bits 2j, 2j + 1 of
// qh[32h + l] on top, minus 32, scaled by scales[8h + 2j + l / 16].  block_q8_K = f32 d | int8 qs[256] |
// int16 bsums[16] (292 bytes).
//
// Alignment: a row is 210 K / 256 bytes, so a block is only 2-byte aligned.  The programming guides for this
// part make no statement about misaligned vector-memory loads, so no load here relies on them: a 32-bit field
// of a block comes from the two naturally aligned dwords that hold it and one v_alignbyte_b32 (ld_u32_a2 in
// the exact kernel; the GEMV loads the block's 53 aligned dwords once and shifts them across lanes);
// scales and d are byte / 16-bit loads, which a 2-byte aligned block keeps naturally aligned.  The dwords
// read lie inside [block - 2, block + 212): at most the two bytes that share an aligned dword (and so a page)
// with the block's first or last two bytes are read beside it, and they are never used.
#include "q6_k_device.h"

namespace ghip {

// ---------------------------------------------------------------------------------------------
// x f32 [N][K] -> block_q8_K AoS; one wave per block.  bsums of an amax == 0 block are written as zeros
// (the reference leaves them unwritten).
__global__ __launch_bounds__(256) void k_quantize_q8_K(const float *__restrict__ x, int64_t nblocks,
                                                        uint8_t *__restrict__ xq) {
    const int lane = threadIdx.x & 63;
    const int64_t blk = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (blk >= nblocks) return;                      // wave-uniform
    const float4 v = reinterpret_cast<const float4 *>(x)[blk * 64 + lane];
    float d;
    const uint32_t p = q8k_block_lane(v, lane, d);
    uint8_t *o = xq + blk * Q8KB;
    if (lane == 0) *reinterpret_cast<float *>(o) = d;
    reinterpret_cast<uint32_t *>(o + 4)[lane] = p;
    int s = __builtin_amdgcn_sdot4((int)p, 0x01010101, 0, false);
    s += dpp_i<DPP_QUAD_XOR1>(s);
    s += dpp_i<DPP_QUAD_XOR2>(s);
    if ((lane & 3) == 0) reinterpret_cast<int16_t *>(o + 4 + QK_K)[lane >> 2] = (int16_t)s;
}

hipError_t quantize_q8_K(const float *x, int64_t K, int64_t N, void *xq, hipStream_t s) {
    const int64_t nblocks = N * (K / QK_K);
    return launch_1d(k_quantize_q8_K, nblocks, 4, s, x, nblocks, (uint8_t *)xq);
}

// ---------------------------------------------------------------------------------------------
// block_q6_K rows -> f32; one thread per four consecutive elements (one scale): (d * (float)sc) * (float)q,
// two rounded multiplies as the reference's `d * sc[is] * q`
__global__ __launch_bounds__(256) void k_dequantize_q6_K(const uint8_t *__restrict__ wq, int64_t nquads,
                                                          float *__restrict__ w) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= nquads) return;
    const uint8_t *p = wq + (idx >> 6) * Q6KB;
    const int t = (int)(idx & 63), h = t >> 5, j = (t >> 3) & 3, i = t & 7;
    const float d = h2f(*reinterpret_cast<const uint16_t *>(p + 208));
    const float ds = __fmul_rn(d, (float)(int)(int8_t)p[192 + 8 * h + 2 * j + (i >> 2)]);
    float o[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint32_t ql = p[64 * h + 32 * (j & 1) + 4 * i + k], qh = p[128 + 32 * h + 4 * i + k];
        const int q = (int)(((j >> 1) ? ql >> 4 : ql & 0xFu) | (((qh >> (2 * j)) & 3u) << 4)) - 32;
        o[k] = __fmul_rn(ds, (float)q);
    }
    reinterpret_cast<float4 *>(w)[idx] = make_float4(o[0], o[1], o[2], o[3]);
}

hipError_t dequantize_q6_K(const void *wq, int64_t K, int64_t M, float *w, hipStream_t s) {
    const int64_t nquads = M * K / 4;
    return launch_1d(k_dequantize_q6_K, nquads, 256, s, (const uint8_t *)wq, nquads, w);
}

// ---------------------------------------------------------------------------------------------
// GEMV, NT <= 8 tokens.  Prologue: the workgroup's four waves quantize x to q8_K into LDS (qs [NT][K] int8,
// d [NT][K / 256] f32; the arithmetic of k_quantize_q8_K).  Then one wave per weight row, rows strided over
// the grid, one superblock per step: the 53 naturally aligned dwords that hold the 210-byte block are ONE
// coalesced load (lane l: dword l), a wave shift and v_alignbyte_b32 turn them into the block's own dwords
// where the block sits at 2 mod 4, and three ds_bpermute_b32 hand lane t the fields of its elements
// 4t .. 4t + 3 (group h = t / 32, j = t / 8 % 4, one scale): the ql dword 16h + 8(j & 1) + t % 8 (nibble
// j / 2), the qh dword 8h + t % 8 (bits 2j) and the scale byte; d is read from lane 52.  The four 6-bit
// values are recentred to q - 32 and go through v_dot4_i32_i8 against the q8_K bytes; the lanes' parts
// sc * dot are added over the wave by DPP into the exact int32 isum_b = sum_g sc[g] sum_(j in g) (q_j - 32) q8_j
// (|isum_b| <= 2^27), and lane 63 accumulates y += (d_x[b] d_w[b]) * (float)isum_b by f32 fma, superblocks
// in order (deterministic; x -> 2x doubles every term exactly).  The loads of GEMV6_UNROLL superblocks are
// issued before the first is used.
static constexpr int GEMV6_THREADS = 256;
static constexpr int GEMV6_MAX_K = 16384;
static constexpr int GEMV6_UNROLL = 4;    // superblocks in flight per wave

template <int NT>
__global__ __launch_bounds__(GEMV6_THREADS) void k_gemv_q6_K(const uint8_t *__restrict__ W, int nb, int M,
                                                              const float *__restrict__ x, float *__restrict__ y,
                                                              int64_t ldy) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int K = nb * QK_K;
    uint32_t *xq = reinterpret_cast<uint32_t *>(smem);
    float *xd = reinterpret_cast<float *>(smem + (size_t)NT * K);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int blk = wave; blk < NT * nb; blk += GEMV6_THREADS / 64) {
        const float4 v = reinterpret_cast<const float4 *>(x)[blk * 64 + lane];
        float d;
        const uint32_t p = q8k_block_lane(v, lane, d);
        xq[blk * 64 + lane] = p;
        if (lane == 0) xd[blk] = d;
    }
    __syncthreads();
    // lane t of the wave owns elements 4t .. 4t + 3 of a superblock: group (h, j), one scale
    const int h = lane >> 5, j = (lane >> 3) & 3, i = lane & 7;
    const int ql_src = 4 * (16 * h + 8 * (j & 1) + i), ql_sh = 4 * (j >> 1);      // byte address of the source lane
    const int qh_src = 4 * (32 + 8 * h + i), qh_sh = 2 * j;
    const int sc_idx = 8 * h + 2 * j + (i >> 2);
    const int sc_src = 4 * (48 + (sc_idx >> 2)), sc_sh = 8 * (sc_idx & 3);
    const int64_t rowbytes = (int64_t)nb * Q6KB;
    // the wave's steps: batches of GEMV6_UNROLL superblocks along its rows m, m + stride, ...; the loads of the
    // next batch (of the next row after a row's last) are in flight while the current one is consumed
    const int stride = gridDim.x * (GEMV6_THREADS / 64);
    // (unconditional loads at clamped indices, always inside the matrix: a load under a branch would make the
    // compiler wait for every load in flight, the prefetched batch included, before the first use)
    const int ld_lane = lane < 53 ? lane : 52;
    auto load_batch = [&](int m, int b0, uint32_t *r) __attribute__((always_inline)) {
        const uint8_t *row = W + (int64_t)(m < M ? m : M - 1) * rowbytes;
#pragma unroll
        for (int u = 0; u < GEMV6_UNROLL; u++) {
            // (pointer arithmetic, not an integer round trip: the address stays a global one, no flat load)
            const uint8_t *p = row + (b0 + u < nb ? b0 + u : nb - 1) * Q6KB;
            r[u] = reinterpret_cast<const uint32_t *>(p - ((uintptr_t)p & 3))[ld_lane];
        }
    };
    int m = blockIdx.x * (GEMV6_THREADS / 64) + wave, b0 = 0;
    uint32_t cur[GEMV6_UNROLL], nxt[GEMV6_UNROLL];
    load_batch(m, b0, cur);
    float acc[NT];
#pragma unroll
    for (int n = 0; n < NT; n++) acc[n] = 0.0f;
    while (m < M) {                                       // wave-uniform
        const bool last = b0 + GEMV6_UNROLL >= nb;        // of this row
        const int nm = last ? m + stride : m, nb0 = last ? 0 : b0 + GEMV6_UNROLL;
        load_batch(nm, nb0, nxt);
#pragma unroll
        for (int u = 0; u < GEMV6_UNROLL; u++) {          // (written out: the cross-lane steps keep the compiler
            // from unrolling a loop with a run-time trip count.)  No branch per superblock, so that the batch's
            // independent chains interleave: a step past the row's end repeats its last block with d_w = 0,
            // which adds +-0 to an accumulator that is never -0
            const bool live = b0 + u < nb;
            const int b = live ? b0 + u : nb - 1;
            const uintptr_t a = (uintptr_t)(W + (int64_t)m * rowbytes + b * Q6KB);
            const uint32_t raw = cur[u];
            const uint32_t nx = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)raw, DPP_WAVE_SHL1, 0xF, 0xF, false);
            const uint32_t own = (a & 2) ? __builtin_amdgcn_alignbyte(nx, raw, 2) : raw;
            const uint32_t ql = (uint32_t)__builtin_amdgcn_ds_bpermute(ql_src, (int)own) >> ql_sh;
            const uint32_t qh = (uint32_t)__builtin_amdgcn_ds_bpermute(qh_src, (int)own) >> qh_sh;
            const int sc = (int)(int8_t)((uint32_t)__builtin_amdgcn_ds_bpermute(sc_src, (int)own) >> sc_sh);
            const float dw = live ? h2f((uint32_t)__builtin_amdgcn_readlane((int)own, 52)) : 0.0f;
            const uint32_t q = q6_recentre((ql & 0x0F0F0F0Fu) | ((qh & 0x03030303u) << 4));
#pragma unroll
            for (int n = 0; n < NT; n++) {
                const int part = sc * __builtin_amdgcn_sdot4((int)q, (int)xq[(n * nb + b) * 64 + lane], 0, false);
                const int isum = wave_isum_lane63(part);            // lane 63: the superblock's exact sum
                acc[n] = __builtin_fmaf(xd[n * nb + b] * dw, (float)isum, acc[n]);
            }
        }
        if (last) {
#pragma unroll
            for (int n = 0; n < NT; n++) {
                if (lane == 63) y[(int64_t)n * ldy + m] = acc[n];
                acc[n] = 0.0f;
            }
        }
#pragma unroll
        for (int u = 0; u < GEMV6_UNROLL; u++) cur[u] = nxt[u];
        m = nm;
        b0 = nb0;
    }
}

template <int NT>
static hipError_t launch_gemv6(const uint8_t *W, int nb, int M, const float *x, float *y, int64_t ldy, int num_cus,
                               hipStream_t s) {
    const size_t lds = (size_t)NT * ((size_t)nb * QK_K + (size_t)nb * 4);
    // (the limit for GEMV6_MAX_K, not this launch's lds: it is set once)
    const hipError_t e = raise_dynamic_lds<k_gemv_q6_K<NT>>(NT * (GEMV6_MAX_K + GEMV6_MAX_K / QK_K * 4));
    if (e != hipSuccess) return e;
    const int per = GEMV6_THREADS / 64;
    const int64_t want = ((int64_t)M + per - 1) / per;
    const int64_t cap = (int64_t)(num_cus > 0 ? num_cus : 256) * 8;
    (void)hipGetLastError();  // report only this launch's error
    launch_k(k_gemv_q6_K<NT>, dim3((unsigned)(want < cap ? want : cap)), dim3(GEMV6_THREADS), lds, s, W, nb, M, x, y, ldy);
    return hipGetLastError();
}

// any N: column tiles of 8 through the same kernel (each tile is exactly the call on those columns)
hipError_t gemv_q6_K(const void *W, int64_t K, int64_t M, const float *x, int64_t N, float *y, int64_t ldy,
                     const DeviceInfo &dev, hipStream_t s) {
    if (K <= 0 || K % QK_K || K > GEMV6_MAX_K || M < 1 || M >= ((int64_t)1 << 31)) return hipErrorInvalidValue;
    const int nb = (int)(K / QK_K);
    return for_column_tiles(N, 8, [&](int64_t n0, int nt) {
        return with_token_tile(nt, [&](auto NT) {
            return launch_gemv6<decltype(NT)::value>((const uint8_t *)W, nb, (int)M, x + n0 * K, y + n0 * ldy, ldy,
                                                     dev.num_cus, s);
        });
    });
}

// ---------------------------------------------------------------------------------------------
// Exact mode: y bit-identical to the AVX2 branch of ggml_vec_dot_q6_K_q8_K (k_quants.c:3484-3561), a fixed
// fp32 schedule: per superblock eight int32 lanes, lane m = sum over the 32-element groups g = 0..7 of
// sc[2g + (m >= 4)] * sum of (q - 32) q8 over elements 32g + 4m .. 32g + 4m + 3 (maddubs pairs, madd with the
// scales; 2 * 63 * 128 + 2 * 32 * 128 < 32767, so the int16 steps are exact), then acc_m = fma(d, (float)lane m,
// acc_m) with d = d_x * fp32(d_w), superblocks in order, and hsum_float_8's tree at the end.  Eight threads per
// output run the eight chains; x is the AoS q8_K of k_quantize_q8_K.
static constexpr int EX6_ROWS = 16;

__global__ __launch_bounds__(EX6_ROWS * 8) void k_mm_exact_q6_K(const uint8_t *__restrict__ W, int nb, int M,
                                                                 const uint8_t *__restrict__ xq, float *__restrict__ y,
                                                                 int64_t ldy) {
    const int m8 = threadIdx.x & 7, r = threadIdx.x >> 3;
    const int m = blockIdx.x * EX6_ROWS + r, n = blockIdx.y;
    const bool live = m < M;
    const uint8_t *row = W + (int64_t)(live ? m : M - 1) * nb * Q6KB;     // idle rows shadow the last one (shuffles)
    const uint8_t *xr = xq + (int64_t)n * nb * Q8KB;
    const int sc_hi = m8 >> 2;
    float acc = 0.0f;
    for (int b = 0; b < nb; b++) {
        const uint8_t *blk = row + b * Q6KB, *xb = xr + b * Q8KB;
        const float d = *reinterpret_cast<const float *>(xb) * h2f(*reinterpret_cast<const uint16_t *>(blk + 208));
        int sumi = 0;
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const uint32_t qla = ld_u32_a2(blk + 64 * h + 4 * m8), qlb = ld_u32_a2(blk + 64 * h + 32 + 4 * m8);
            const uint32_t qh = ld_u32_a2(blk + 128 + 32 * h + 4 * m8);
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int g = 4 * h + j;
                const uint32_t ql = (j & 1) ? qlb : qla;
                const uint32_t nib = ((j >> 1) ? ql >> 4 : ql) & 0x0F0F0F0Fu;
                const uint32_t q = q6_recentre(nib | (((qh >> (2 * j)) & 0x03030303u) << 4));
                const uint32_t x4 = *reinterpret_cast<const uint32_t *>(xb + 4 + 32 * g + 4 * m8);
                sumi += (int)(int8_t)blk[192 + 2 * g + sc_hi] * __builtin_amdgcn_sdot4((int)q, (int)x4, 0, false);
            }
        }
        acc = __builtin_fmaf(d, (float)sumi, acc);
    }
    float v = acc;
    v = v + __shfl_xor(v, 4, 8);       // r_k = acc_k + acc_{k+4}
    v = v + __shfl_xor(v, 2, 8);       // lane 0: r0 + r2, lane 1: r1 + r3
    v = v + __shfl_xor(v, 1, 8);       // lane 0: (r0 + r2) + (r1 + r3)
    if (m8 == 0 && live) y[(int64_t)n * ldy + m] = v;
}

hipError_t mm_exact_q6_K(const void *W, int64_t K, int64_t M, const void *xq8k, int64_t N, float *y, int64_t ldy,
                         hipStream_t s) {
    if (K <= 0 || K % QK_K || M < 1 || M >= ((int64_t)1 << 31)) return hipErrorInvalidValue;
    return launch_column_chunks(N, [&](int64_t n0, unsigned nn) {
        launch_k(k_mm_exact_q6_K, dim3((unsigned)((M + EX6_ROWS - 1) / EX6_ROWS), nn), dim3(EX6_ROWS * 8), 0, s,
                 (const uint8_t *)W, (int)(K / QK_K), (int)M, (const uint8_t *)xq8k + n0 * (K / QK_K) * Q8KB, y + n0 * ldy, ldy);
    });
}

}  // namespace ghip
