// q45_k.hip — the Q5_K / Q4_K x F32 mul_mat of a "mostly Q5_K" / "mostly Q4_K" file's layer matrices (gfx950,
// wave64): the dequantizer, the fused GEMV (N <= 8 per launch) and the exact kernel, one template parameter QH
// (true: Q5_K, false: Q4_K); the prefill GEMM is q45_k_gemm.hip.  Shared device helpers: q4_0_device.h,
// q6_k_device.h (q8k_block_lane), q45_k_device.h (Q45<QH>, unpack_scales_k4).  What each
// kernel restates (reference = k_quants.c of Fcucgvhhhvjv/llama.cpp-q_4_0, QK_K = 256):
//   k_dequantize_q45_K<QH>  dequantize_row_q4_K k_quants.c:733-770 / dequantize_row_q5_K 926-969 (bit-exact)
//   k_gemv_q45_K<QH, NT>    ggml_vec_dot_q4_K_q8_K / _q5_K_q8_K with the q8_K quantization of x fused into the
//                           prologue (LDS, once per workgroup), one wave64 per weight row; y within the parity bound
//   k_mm_exact_q45_K<QH>    the AVX2 branches k_quants.c:2450-2513 (Q4_K) and 2927-3010 (Q5_K), bit for bit
//
// Layouts: block_q5_K = fp16 d | fp16 dmin | scales[12] | qh[32] | qs[128] (176 bytes); block_q4_K the same
// without qh (144 bytes).  Element 64j + 32h + l (j = 0..3, h = 0..1, l = 0..31) is nibble h of qs[32j + l], plus 16
// where bit 2j + h of qh[l] is set; sub-block s = 2j + h has the 6-bit scale sc[s] and min m[s] packed in
// scales[12] (unpacked as k_quants.c:2462-2467 does): w = d sc[s] q - dmin m[s].  block_q8_K = f32 d | int8 qs[256]
// | int16 bsums[16] (292 bytes).
//
// Alignment: both block sizes are multiples of 16 bytes, so with a 16-byte aligned matrix every block, its
// 16-byte header (d, dmin, scales) and every dword of qh and qs are naturally aligned; every load is a naturally
// aligned vector load of bytes inside the matrix.
//
// The GEMV's fp32 order (tests/q45k_ref.py gemv_schedule restates it): per superblock b the exact int32 sums
// isum_b = sum_s sc[s] sum_(l) q q8 and msum_b = sum_s m[s] (sum of the 32 q8 of sub-block s), then
//   t_b = fma(d_x d, (float)isum_b, -((d_x dmin) (float)msum_b))      (d_x d and d_x dmin: one rounded multiply each)
//   acc = acc + t_b,  b = 0, 1, ..., K / 256 - 1, K never split
// so y does not depend on the grid, the row mapping or the token tile, and x -> 2x doubles every term exactly.
#include "q45_k_device.h"

namespace ghip {

// ---------------------------------------------------------------------------------------------
// block rows -> f32; one thread per four consecutive elements (one sub-block): d1 * (float)q - m1 with
// d1 = d * (float)sc and m1 = dmin * (float)m, rounded multiplies and a rounded subtraction as the reference's
// `d1 * q - m1` without contraction
template <bool QH>
__global__ __launch_bounds__(256) void k_dequantize_q45_K(const uint8_t *__restrict__ wq, int64_t nquads,
                                                           float *__restrict__ w) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= nquads) return;
    const uint32_t *p = reinterpret_cast<const uint32_t *>(wq + (idx >> 6) * Q45<QH>::BYTES);
    const int t = (int)(idx & 63), s = t >> 3, i = t & 7;           // sub-block s = 2j + h, elements 4i .. 4i + 3 of it
    const uint32_t h0 = p[0];
    const ScaleMin u = unpack_scales_k4(p[1], p[2], p[3]);
    const uint32_t sc = ((s < 4 ? u.sc_lo : u.sc_hi) >> (8 * (s & 3))) & 0xFFu;
    const uint32_t mn = ((s < 4 ? u.m_lo : u.m_hi) >> (8 * (s & 3))) & 0xFFu;
    const float d1 = __fmul_rn(h2f(h0 & 0xFFFFu), (float)sc), m1 = __fmul_rn(h2f(h0 >> 16), (float)mn);
    uint32_t q = (p[Q45<QH>::QS / 4 + 8 * (s >> 1) + i] >> (4 * (s & 1))) & 0x0F0F0F0Fu;
    if (QH) q |= ((p[4 + i] >> s) & 0x01010101u) << 4;
    float o[4];
#pragma unroll
    for (int k = 0; k < 4; k++) o[k] = __fsub_rn(__fmul_rn(d1, (float)((q >> (8 * k)) & 0xFFu)), m1);
    reinterpret_cast<float4 *>(w)[idx] = make_float4(o[0], o[1], o[2], o[3]);
}

template <bool QH>
static hipError_t dequantize_q45_K_t(const void *wq, int64_t K, int64_t M, float *w, hipStream_t s) {
    const int64_t nquads = M * K / 4;
    return launch_1d(k_dequantize_q45_K<QH>, nquads, 256, s, (const uint8_t *)wq, nquads, w);
}

hipError_t dequantize_q45_K(bool qh, const void *wq, int64_t K, int64_t M, float *w, hipStream_t s) {
    return qh ? dequantize_q45_K_t<true>(wq, K, M, w, s) : dequantize_q45_K_t<false>(wq, K, M, w, s);
}

// ---------------------------------------------------------------------------------------------
// GEMV, NT <= 8 tokens.  Prologue: the workgroup's waves quantize x to q8_K into LDS (the arithmetic of
// k_quantize_q8_K): per (token, superblock) the 64 q8 dwords, the eight per-32-element sums of the q8 values
// (int32; the reference's bsums pairs added exactly) and d_x.  The q8 dwords are stored permuted: the dword of
// elements 64j + 32h + 4i .. + 3 sits at dword 2 (8j + i) + h, so that the main loop's lane reads its two dwords
// with one 8-byte LDS load, conflict-free.
// Main loop: one wave per weight row, rows strided over the grid; half a wave per superblock, two superblocks
// per step.  Lane t of the half (j = t / 8, i = t % 8) loads qs dword t = four low nibbles of sub-block 2j and
// four high nibbles of sub-block 2j + 1 (elements 4i .. 4i + 3 of each), for Q5_K also qh dword i (bit 2j of each
// byte goes to sub-block 2j, bit 2j + 1 to sub-block 2j + 1), and the block's 16-byte header (the same address in
// every lane of the half: one request).  The 4- or 5-bit values (<= 31, a signed byte) go through two
// v_dot4_i32_i8 against the lane's q8 dwords; the lane's part sc[2j] dot_lo + sc[2j + 1] dot_hi is added over the
// half by DPP into the exact int32 isum_b (|isum_b| < 2^26), valid in the half's upper 16 lanes; the half's last
// eight lanes hold m[i] bsum32[i] and add them into the exact msum_b (< 2^21).  Per-lane partials cancel within
// a superblock, so nothing is converted to fp32 before these sums.  The half's last lane forms t_b (header
// comment), lane 63 receives the even superblock's t_b from lane 31 and accumulates both in superblock order.
// The loads of GEMV45_UNROLL steps are issued before the first is used, and two such batches are in flight: at
// K = 4096 a wave has its whole row requested before it consumes the first byte.  The workgroup is 16 waves: on the
// LLaMA-7B layer shapes a wave owns one to three rows, so a launch is one wave's chain of prologue and load
// latencies, and the prologue's share per wave shrinks with the waves that divide the x blocks among them
// (measurements: DESIGN §4b).
static constexpr int GEMV45_THREADS = 1024;
static constexpr int GEMV45_MAX_K = 16384;
static constexpr int GEMV45_UNROLL = 4;   // steps (of two superblocks) per batch
static constexpr int GEMV45_LDS_PER_BLOCK = QK_K + 8 * 4 + 4;     // q8 bytes + eight int32 sums + d_x, per token and superblock

template <bool QH>
struct Gemv45Regs {
    u32x4 hdr[GEMV45_UNROLL];
    uint32_t qs[GEMV45_UNROLL];
    uint32_t qh[GEMV45_UNROLL];
};

template <bool QH, int NT>
__global__ __launch_bounds__(GEMV45_THREADS) void k_gemv_q45_K(const uint8_t *__restrict__ W, int nb, int M,
                                                                const float *__restrict__ x, float *__restrict__ y,
                                                                int64_t ldy) {
    constexpr int BS = Q45<QH>::BYTES, QS = Q45<QH>::QS;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int K = nb * QK_K;
    uint32_t *xq = reinterpret_cast<uint32_t *>(smem);                                  // [NT nb][64] permuted
    int *xs = reinterpret_cast<int *>(smem + (size_t)NT * K);                           // [NT nb][8]
    float *xd = reinterpret_cast<float *>(smem + (size_t)NT * K + (size_t)NT * nb * 32);   // [NT nb]
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int half = lane >> 5, t = lane & 31, j = t >> 3, i = t & 7;
    const int nsteps = (nb + 1) >> 1;
    const int64_t rowbytes = (int64_t)nb * BS;
    const int stride = gridDim.x * (GEMV45_THREADS / 64);
    // (unconditional loads at clamped indices, always inside the matrix: a load under a branch would make the
    // compiler wait for every load in flight, the prefetched batch included, before the first use)
    auto load_batch = [&](int m, int s0, Gemv45Regs<QH> &r) __attribute__((always_inline)) {
        const uint8_t *row = W + (int64_t)(m < M ? m : M - 1) * rowbytes;
#pragma unroll
        for (int u = 0; u < GEMV45_UNROLL; u++) {
            const int b = 2 * (s0 + u) + half;
            const uint8_t *p = row + (b < nb ? b : nb - 1) * BS;
            r.hdr[u] = *reinterpret_cast<const u32x4 *>(p);
            r.qs[u] = reinterpret_cast<const uint32_t *>(p + QS)[t];
            r.qh[u] = QH ? reinterpret_cast<const uint32_t *>(p + 16)[i] : 0u;
        }
    };
    int m = blockIdx.x * (GEMV45_THREADS / 64) + wave, s0 = 0;
    Gemv45Regs<QH> cur, nxt;
    {
        // the wave's first x block is requested first and its first weight batch right behind it, so the weights
        // travel while x is quantized (the wait for the x block does not wait for the weights issued after it);
        // the next x block is requested before the current one is worked on
        const int nblk = NT * nb;
        const float4 *x4 = reinterpret_cast<const float4 *>(x);
        float4 v = x4[(wave < nblk ? wave : nblk - 1) * 64 + lane];
        __builtin_amdgcn_sched_barrier(0);                 // (keeps the x request in front of the weight requests)
        load_batch(m, s0, cur);
        // quantizer lane l holds elements 4l .. 4l + 3: l = 16j + 8h + i
        const int dst = 2 * (8 * (lane >> 4) + (lane & 7)) + ((lane >> 3) & 1);
        // (no branch around the first block, so that its request stays where it is written: a wave beyond the last
        // block repeats the last one and stores the same values again)
        int blk = wave;
        do {
            const int bc = blk < nblk ? blk : nblk - 1, nx = blk + GEMV45_THREADS / 64;
            const float4 vn = x4[(nx < nblk ? nx : nblk - 1) * 64 + lane];
            float d;
            const uint32_t p = q8k_block_lane(v, lane, d);
            xq[bc * 64 + dst] = p;
            const int s32 = group8_sum(__builtin_amdgcn_sdot4((int)p, 0x01010101, 0, false));
            if ((lane & 7) == 0) xs[bc * 8 + (lane >> 3)] = s32;
            if (lane == 0) xd[bc] = d;
            v = vn;
            blk = nx;
        } while (blk < nblk);
    }
    __syncthreads();
    float acc[NT];
#pragma unroll
    for (int n = 0; n < NT; n++) acc[n] = 0.0f;
    while (m < M) {                                       // wave-uniform
        const bool last = s0 + GEMV45_UNROLL >= nsteps;   // of this row
        const int nm = last ? m + stride : m, ns0 = last ? 0 : s0 + GEMV45_UNROLL;
        load_batch(nm, ns0, nxt);
#pragma unroll
        for (int u = 0; u < GEMV45_UNROLL; u++) {
            // no branch per step: a half past the row's end repeats the last block and contributes t_b = +0,
            // which leaves an accumulator that is never -0 unchanged
            const int braw = 2 * (s0 + u) + half;
            const bool live = braw < nb;
            const int b = live ? braw : nb - 1;
            const u32x4 hdr = cur.hdr[u];
            const ScaleMin sm = unpack_scales_k4(hdr.y, hdr.z, hdr.w);
            const uint32_t scw = (j < 2 ? sm.sc_lo : sm.sc_hi) >> (16 * (j & 1));
            const int sc0 = (int)(scw & 0xFFu), sc1 = (int)((scw >> 8) & 0xFFu);
            const int mn = (int)(((i < 4 ? sm.m_lo : sm.m_hi) >> (8 * (i & 3))) & 0xFFu);
            const float dw = h2f(hdr.x & 0xFFFFu), dmw = h2f(hdr.x >> 16);
            uint32_t qlo = cur.qs[u] & 0x0F0F0F0Fu, qhi = (cur.qs[u] >> 4) & 0x0F0F0F0Fu;
            if (QH) {
                qlo |= ((cur.qh[u] >> (2 * j)) & 0x01010101u) << 4;
                qhi |= ((cur.qh[u] >> (2 * j + 1)) & 0x01010101u) << 4;
            }
#pragma unroll
            for (int n = 0; n < NT; n++) {
                const int xb = n * nb + b;
                const u32x2 x8 = *reinterpret_cast<const u32x2 *>(xq + xb * 64 + 2 * t);
                int part = sc0 * __builtin_amdgcn_sdot4((int)qlo, (int)x8.x, 0, false) +
                           sc1 * __builtin_amdgcn_sdot4((int)qhi, (int)x8.y, 0, false);
                part += dpp_i<DPP_QUAD_XOR1>(part);
                part += dpp_i<DPP_QUAD_XOR2>(part);
                part += dpp_i<DPP_ROW_HALF_MIRROR>(part);
                part += dpp_i<DPP_ROW_MIRROR>(part);
                part += dpp_im<DPP_ROW_BCAST15, 0xA>(part);              // lanes 16 .. 31 of the half: isum_b
                const int msum = group8_sum(mn * xs[xb * 8 + i]);         // lanes 24 .. 31 of the half: msum_b
                const float dx = xd[xb];
                const float negp = -__fmul_rn(__fmul_rn(dx, dmw), (float)msum);
                float tb = __builtin_fmaf(__fmul_rn(dx, dw), (float)part, negp);
                tb = live ? tb : 0.0f;
                const float te = dpp_f<DPP_ROW_BCAST31, 0xC>(tb);         // lanes 32 .. 63: lane 31's t_b
                acc[n] = __fadd_rn(__fadd_rn(acc[n], te), tb);            // lane 63: even superblock, then odd
            }
        }
        if (last) {
#pragma unroll
            for (int n = 0; n < NT; n++) {
                if (lane == 63) y[(int64_t)n * ldy + m] = acc[n];
                acc[n] = 0.0f;
            }
        }
        cur = nxt;
        m = nm;
        s0 = ns0;
    }
}

template <bool QH, int NT>
static hipError_t launch_gemv45(const uint8_t *W, int nb, int M, const float *x, float *y, int64_t ldy, int num_cus,
                                hipStream_t s) {
    const size_t lds = (size_t)NT * (size_t)nb * GEMV45_LDS_PER_BLOCK;
    // (the limit for GEMV45_MAX_K, not this launch's lds: it is set once)
    const hipError_t e = raise_dynamic_lds<k_gemv_q45_K<QH, NT>>(NT * (GEMV45_MAX_K / QK_K) * GEMV45_LDS_PER_BLOCK);
    if (e != hipSuccess) return e;
    const int per = GEMV45_THREADS / 64;
    const int64_t want = ((int64_t)M + per - 1) / per;
    // one workgroup per CU; rows beyond the grid are strided (y does not depend on this choice)
    const int64_t cap = (int64_t)(num_cus > 0 ? num_cus : 256);
    (void)hipGetLastError();  // report only this launch's error
    launch_k(k_gemv_q45_K<QH, NT>, dim3((unsigned)(want < cap ? want : cap)), dim3(GEMV45_THREADS), lds, s, W, nb, M, x, y,
             ldy);
    return hipGetLastError();
}

// any N: column tiles of 8 through the same kernel (each tile is exactly the call on those columns)
template <bool QH>
static hipError_t gemv_q45_K_t(const void *W, int64_t K, int64_t M, const float *x, int64_t N, float *y, int64_t ldy,
                               const DeviceInfo &dev, hipStream_t s) {
    if (K <= 0 || K % QK_K || K > GEMV45_MAX_K || M < 1 || M >= ((int64_t)1 << 31)) return hipErrorInvalidValue;
    const int nb = (int)(K / QK_K);
    return for_column_tiles(N, 8, [&](int64_t n0, int nt) {
        return with_token_tile(nt, [&](auto NT) {
            return launch_gemv45<QH, decltype(NT)::value>((const uint8_t *)W, nb, (int)M, x + n0 * K, y + n0 * ldy, ldy,
                                                          dev.num_cus, s);
        });
    });
}

hipError_t gemv_q45_K(bool qh, const void *W, int64_t K, int64_t M, const float *x, int64_t N, float *y, int64_t ldy,
                      const DeviceInfo &dev, hipStream_t s) {
    return qh ? gemv_q45_K_t<true>(W, K, M, x, N, y, ldy, dev, s) : gemv_q45_K_t<false>(W, K, M, x, N, y, ldy, dev, s);
}

// ---------------------------------------------------------------------------------------------
// Exact mode: y bit-identical to the AVX2 branches of ggml_vec_dot_q4_K_q8_K (k_quants.c:2450-2513) and
// ggml_vec_dot_q5_K_q8_K (2927-3010), fixed fp32 schedules.  Both: per superblock eight int32 lanes, lane L = sum
// over the sub-blocks s = 0..7 of sc[s] * sum of q q8 over elements 32s + 4L .. 32s + 4L + 3 (maddubs pairs, madd
// with the scales; 2 * 31 * 128 < 32767, so the int16 steps are exact), then acc_L = fma(d, (float)lane L, acc_L)
// with d = d_x * fp32(d_w), superblocks in order, and hsum_float_8's tree at the end.  The mins: s32[k] = bsums[2k]
// + bsums[2k + 1] (hadd_epi16, exact) and prod_i = m[2i] s32[2i] + m[2i + 1] s32[2i + 1] (madd_epi16), with dmin =
// -d_x * fp32(dmin_w).
//   Q4_K: acc_m[i] = fma(dmin, (float)prod_i, acc_m[i]); y = hsum + ((a0 + a2) + (a1 + a3)).
//   Q5_K: summs = summs + dmin * (float)(prod_0 + prod_1 + prod_2 + prod_3), a rounded multiply and a rounded add
//         (the reference is built without contraction); y = hsum + summs.
// Eight threads per output run the eight chains, threads 0..3 (and their mirrors 4..7) the four prod_i; x is the
// AoS q8_K of k_quantize_q8_K.
static constexpr int EX45_ROWS = 16;

template <bool QH>
__global__ __launch_bounds__(EX45_ROWS * 8) void k_mm_exact_q45_K(const uint8_t *__restrict__ W, int nb, int M,
                                                                   const uint8_t *__restrict__ xq,
                                                                   float *__restrict__ y, int64_t ldy) {
    constexpr int BS = Q45<QH>::BYTES, QS = Q45<QH>::QS;
    const int L = threadIdx.x & 7, r = threadIdx.x >> 3;
    const int m = blockIdx.x * EX45_ROWS + r, n = blockIdx.y;
    const bool live = m < M;
    const uint8_t *row = W + (int64_t)(live ? m : M - 1) * nb * BS;       // idle rows shadow the last one (shuffles)
    const uint8_t *xr = xq + (int64_t)n * nb * Q8KB;
    const int pi = L & 3;
    float acc = 0.0f, acc_m = 0.0f;
    for (int b = 0; b < nb; b++) {
        const uint32_t *blk = reinterpret_cast<const uint32_t *>(row + b * BS);
        const uint8_t *xb = xr + b * Q8KB;
        const float dx = *reinterpret_cast<const float *>(xb);
        const uint32_t h0 = blk[0];
        const float d = __fmul_rn(dx, h2f(h0 & 0xFFFFu)), dmin = __fmul_rn(-dx, h2f(h0 >> 16));
        const ScaleMin u = unpack_scales_k4(blk[1], blk[2], blk[3]);
        // prod_pi = m[2 pi] (bsums[4 pi] + bsums[4 pi + 1]) + m[2 pi + 1] (bsums[4 pi + 2] + bsums[4 pi + 3])
        const uint32_t bs0 = *reinterpret_cast<const uint32_t *>(xb + 4 + QK_K + 8 * pi);
        const uint32_t bs1 = *reinterpret_cast<const uint32_t *>(xb + 4 + QK_K + 8 * pi + 4);
        const int sa = (int)(int16_t)(bs0 & 0xFFFFu) + (int)(int16_t)(bs0 >> 16);
        const int sb = (int)(int16_t)(bs1 & 0xFFFFu) + (int)(int16_t)(bs1 >> 16);
        const uint32_t mw = (pi < 2 ? u.m_lo : u.m_hi) >> (16 * (pi & 1));
        const int prod = (int)(mw & 0xFFu) * sa + (int)((mw >> 8) & 0xFFu) * sb;
        if (QH) {
            int tot = prod + __shfl_xor(prod, 1, 8);
            tot = tot + __shfl_xor(tot, 2, 8);                          // prod_0 + .. + prod_3 (int32, any order)
            acc_m = __fadd_rn(acc_m, __fmul_rn(dmin, (float)tot));
        } else {
            acc_m = __builtin_fmaf(dmin, (float)prod, acc_m);
        }
        const uint32_t qhw = QH ? blk[4 + L] : 0u;
        int sumi = 0;
#pragma unroll
        for (int jj = 0; jj < 4; jj++) {
            const uint32_t ql = blk[QS / 4 + 8 * jj + L];
            uint32_t qlo = ql & 0x0F0F0F0Fu, qhi = (ql >> 4) & 0x0F0F0F0Fu;
            if (QH) {
                qlo |= ((qhw >> (2 * jj)) & 0x01010101u) << 4;
                qhi |= ((qhw >> (2 * jj + 1)) & 0x01010101u) << 4;
            }
            const uint32_t xlo = *reinterpret_cast<const uint32_t *>(xb + 4 + 64 * jj + 4 * L);
            const uint32_t xhi = *reinterpret_cast<const uint32_t *>(xb + 4 + 64 * jj + 32 + 4 * L);
            const uint32_t scw = (jj < 2 ? u.sc_lo : u.sc_hi) >> (16 * (jj & 1));
            sumi += (int)(scw & 0xFFu) * __builtin_amdgcn_sdot4((int)qlo, (int)xlo, 0, false);
            sumi += (int)((scw >> 8) & 0xFFu) * __builtin_amdgcn_sdot4((int)qhi, (int)xhi, 0, false);
        }
        acc = __builtin_fmaf(d, (float)sumi, acc);
    }
    float v = acc;
    v = __fadd_rn(v, __shfl_xor(v, 4, 8));       // r_k = acc_k + acc_{k+4}
    v = __fadd_rn(v, __shfl_xor(v, 2, 8));       // lane 0: r0 + r2, lane 1: r1 + r3
    v = __fadd_rn(v, __shfl_xor(v, 1, 8));       // lane 0: (r0 + r2) + (r1 + r3)
    float am = acc_m;                            // Q5_K: summs in every lane
    if (!QH) {
        am = __fadd_rn(am, __shfl_xor(am, 2, 8));   // lane 0: a0 + a2, lane 1: a1 + a3
        am = __fadd_rn(am, __shfl_xor(am, 1, 8));   // lane 0: (a0 + a2) + (a1 + a3)
    }
    if (L == 0 && live) y[(int64_t)n * ldy + m] = __fadd_rn(v, am);
}

template <bool QH>
static hipError_t mm_exact_q45_K_t(const void *W, int64_t K, int64_t M, const void *xq8k, int64_t N, float *y,
                                   int64_t ldy, hipStream_t s) {
    if (K <= 0 || K % QK_K || M < 1 || M >= ((int64_t)1 << 31)) return hipErrorInvalidValue;
    return launch_column_chunks(N, [&](int64_t n0, unsigned nn) {
        launch_k(k_mm_exact_q45_K<QH>, dim3((unsigned)((M + EX45_ROWS - 1) / EX45_ROWS), nn), dim3(EX45_ROWS * 8), 0, s,
                 (const uint8_t *)W, (int)(K / QK_K), (int)M, (const uint8_t *)xq8k + n0 * (K / QK_K) * Q8KB, y + n0 * ldy,
                 ldy);
    });
}

hipError_t mm_exact_q45_K(bool qh, const void *W, int64_t K, int64_t M, const void *xq8k, int64_t N, float *y, int64_t ldy,
                          hipStream_t s) {
    return qh ? mm_exact_q45_K_t<true>(W, K, M, xq8k, N, y, ldy, s) : mm_exact_q45_K_t<false>(W, K, M, xq8k, N, y, ldy, s);
}

}  // namespace ghip
