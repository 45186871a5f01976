// q23_k.hip — the Q3_K / Q2_K x F32 mul_mat of a "mostly Q3_K" / "mostly Q2_K" file's layer matrices (gfx950,
// wave64): the dequantizer, the fused GEMV (N <= 8 per launch) and the exact kernel, one template parameter Q3
// (true: Q3_K, false: Q2_K); the prefill GEMM, bitwise this GEMV, is q23_k_gemm.hip.  Shared device helpers:
// q4_0_device.h, q6_k_device.h (q8k_block_lane), q23_k_device.h (Q23<Q3>, q23_values, the scales).  What each
// kernel restates (reference = k_quants.c of Fcucgvhhhvjv/llama.cpp-q_4_0, QK_K = 256):
//   k_dequantize_q23_K<Q3>  dequantize_row_q3_K k_quants.c:531-579 / dequantize_row_q2_K 352-396 (bit-exact)
//   k_gemv_q23_K<Q3, NT>    ggml_vec_dot_q3_K_q8_K / _q2_K_q8_K with the q8_K quantization of x fused into the
//                           prologue (LDS, once per workgroup), one wave64 per weight row; y within the parity bound
//   k_mm_exact_q23_K<Q3>    the AVX2 branches k_quants.c:1836-1938 (Q3_K) and 1330-1394 (Q2_K), bit for bit
//
// Layouts: block_q3_K = hmask[32] | qs[64] | scales[12] | fp16 d (110 bytes); block_q2_K = scales[16] | qs[64] |
// fp16 d | fp16 dmin (84 bytes).  Element 128n + 32k + l (n = 0..1, k = 0..3, l = 0..31) has the two low bits
// (qs[32n + l] >> 2k) & 3 and the sub-block s = 8n + 2k + l / 16 (16 elements each).  Q3_K: q = low2 + 4 (bit 4n + k
// of hmask[l]) - 4, the 16 six-bit scales packed in scales[12] (k_quants.c:1854-1860) minus 32, w = d sc[s] q.
// Q2_K: q = low2, sc[s] = scales[s] & 15, m[s] = scales[s] >> 4, w = d sc[s] q - dmin m[s].  block_q8_K = f32 d |
// int8 qs[256] | int16 bsums[16] (292 bytes), the bsums per 16 elements: the sub-blocks of both types.
//
// Alignment: the matrix is 4-byte aligned.  A Q2_K block (84 bytes) is then dword aligned and every load of it is a
// naturally aligned dword.  A Q3_K block (110 bytes) sits at 0 or 2 mod 4 (a row of an odd number of superblocks puts
// the next row at 2 mod 4), and no load relies on misaligned vector-memory access: a 32-bit field comes from the
// aligned dwords that hold it and one v_alignbyte_b32 (q23_k_device.h blk_dword), d is a 16-bit load, the
// dequantizer reads bytes.  For a block at 2 mod 4 the aligned span starts two bytes before it: those are the
// previous block's d, inside the matrix, because a 4-byte aligned matrix never starts at 2 mod 4; for an aligned
// block the span ends with the dword that holds scales[8..11].  So no byte outside [W, W + M (K / 256) BYTES) is
// read, by any kernel here, for either type.
//
// The GEMV's fp32 order (tests/q23k_ref.py gemv_schedule restates it): per superblock b the exact int32 sums
// isum_b = sum_s sc[s] sum_(l) q q8 (|isum_b| <= 2^22) and, Q2_K, msum_b = sum_s m[s] bsums[s], then
//   Q3_K: t_b = (d_x d) (float)isum_b
//   Q2_K: t_b = fma(d_x d, (float)isum_b, -((d_x dmin) (float)msum_b))     (d_x d and d_x dmin: one rounded multiply each)
//   acc = acc + t_b,  b = 0, 1, ..., K / 256 - 1, K never split
// so y does not depend on the grid, the row mapping or the token tile, and x -> 2x doubles every term exactly.
#include "q23_k_device.h"

namespace ghip {

// ---------------------------------------------------------------------------------------------
// block rows -> f32; one thread per four consecutive elements (one sub-block), byte loads and a 16-bit d.
// Q3_K: dl = d * (float)(sc - 32), y = dl * (float)q; Q2_K: dl = d * (float)sc, ml = dmin * (float)m, y = dl *
// (float)q - ml: rounded multiplies and a rounded subtraction, as the reference without contraction
template <bool Q3>
__global__ __launch_bounds__(256) void k_dequantize_q23_K(const uint8_t *__restrict__ wq, int64_t nquads,
                                                           float *__restrict__ w) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= nquads) return;
    const uint8_t *p = wq + (idx >> 6) * Q23<Q3>::BYTES;
    const int t = (int)(idx & 63), n = t >> 5, k = (t >> 3) & 3, i = t & 7;   // elements 128n + 32k + 4i .. + 3
    const int s = 8 * n + 2 * k + (i >> 2);
    const float d = h2f(*reinterpret_cast<const uint16_t *>(p + Q23<Q3>::D));
    float dl, ml = 0.0f;
    if (Q3) {
        const uint8_t *sp = p + Q23<Q3>::SC;
        const uint32_t lo = (uint32_t)sp[s & 7] >> (4 * (s >> 3)) & 0xFu;
        const uint32_t hi = ((uint32_t)sp[8 + (s & 3)] >> (2 * (s >> 2))) & 3u;
        dl = __fmul_rn(d, (float)((int)(lo | (hi << 4)) - 32));
    } else {
        const uint32_t sc = p[s];
        dl = __fmul_rn(d, (float)(sc & 0xFu));
        ml = __fmul_rn(h2f(*reinterpret_cast<const uint16_t *>(p + Q23<Q3>::D + 2)), (float)(sc >> 4));
    }
    float o[4];
#pragma unroll
    for (int e = 0; e < 4; e++) {
        int q = (int)((p[Q23<Q3>::QS + 32 * n + 4 * i + e] >> (2 * k)) & 3u);
        if (Q3) {
            q -= ((p[4 * i + e] >> (4 * n + k)) & 1u) ? 0 : 4;
            o[e] = __fmul_rn(dl, (float)q);
        } else {
            o[e] = __fsub_rn(__fmul_rn(dl, (float)q), ml);
        }
    }
    reinterpret_cast<float4 *>(w)[idx] = make_float4(o[0], o[1], o[2], o[3]);
}

template <bool Q3>
static hipError_t dequantize_q23_K_t(const void *wq, int64_t K, int64_t M, float *w, hipStream_t s) {
    const int64_t nquads = M * K / 4;
    return launch_1d(k_dequantize_q23_K<Q3>, nquads, 256, s, (const uint8_t *)wq, nquads, w);
}

hipError_t dequantize_q23_K(bool q3, const void *wq, int64_t K, int64_t M, float *w, hipStream_t s) {
    return q3 ? dequantize_q23_K_t<true>(wq, K, M, w, s) : dequantize_q23_K_t<false>(wq, K, M, w, s);
}

// ---------------------------------------------------------------------------------------------
// GEMV, NT <= 8 tokens.  Prologue: the workgroup's waves quantize x to q8_K into LDS (the arithmetic of
// k_quantize_q8_K): per (token, superblock) the 64 q8 dwords, d_x and, for Q2_K, the sixteen per-16-element sums of
// the q8 values as int16 (the reference's bsums; |sum| <= 2048).  With int32 sums the K = 16384, NT = 8 image would
// not fit the LDS; with int16 it is 292 bytes per (token, superblock), 149,504 bytes in all (Q3_K: 260 bytes).  The q8
// dwords are stored permuted: the dword of elements 128n + 32k + 4i .. + 3 sits at dword 4 (8n + i) + k, so that the
// main loop's lane reads its four dwords with one 16-byte LDS load.
// Main loop: one wave per weight row, rows strided over the grid; a quarter wave (one DPP row of 16 lanes) per
// superblock, four superblocks per step.  Lane t of the quarter (n = t / 8, i = t % 8) loads qs dword 8n + i, for
// Q3_K also hmask dword i (bits 4n .. 4n + 3 of each byte), and the scales (the same addresses in every lane of the
// quarter).  It owns four groups of four elements, one per k, under scale 8n + 2k + (i >= 4): four v_dot4_i32_i8
// against its q8 dwords; the lane's part sum_k sc_k dot_k is added over the row by DPP into the exact int32 isum_b,
// valid in every lane of the quarter.  Q2_K: lane t also holds m[t] bsums[t], added the same way into msum_b.
// Nothing is converted to fp32 before these sums.  Every lane forms its quarter's t_b (header comment); the four are
// read from lanes 0, 16, 32, 48 and added to the accumulator in superblock order, in every lane.
// The loads of UNROLL steps are issued before the first is used, and two such batches are in flight: with batches
// of two steps a K = 4096 row is exactly the two batches.  Measured on the LLaMA-7B layer shapes (N = 1, weights from
// HBM): batches of one step cost 6-17 % more time, batches of four (whose second batch at K = 4096 is
// the clamped next row, loaded for nothing) 4-11 % more on Q3_K; 512- or 256-thread workgroups 7-50 % more.
static constexpr int GEMV23_THREADS = 1024;
static constexpr int GEMV23_MAX_K = 16384;

template <bool Q3>
struct Gemv23 {
    static constexpr int UNROLL = 2;                                 // steps (of four superblocks) per batch
    static constexpr int LDS_PER_BLOCK = QK_K + 4 + (Q3 ? 0 : 32);   // q8 bytes + d_x (+ sixteen int16 sums)
};

// one step's loads of a lane.  Q3_K: the aligned dword pairs of qs dword 8n + i and hmask dword i, the four aligned
// dwords that hold scales[12], d.  Q2_K: qs dword 8n + i, scales dwords 2n and 2n + 1 (the lane's scales), scales
// dword t / 4 (the lane's min), d | dmin.
template <bool Q3>
struct Gemv23Regs {
    uint32_t a[Gemv23<Q3>::UNROLL][Q3 ? 9 : 5];
};

template <bool Q3, int NT>
__global__ __launch_bounds__(GEMV23_THREADS) void k_gemv_q23_K(const uint8_t *__restrict__ W, int nb, int M,
                                                                const float *__restrict__ x, float *__restrict__ y,
                                                                int64_t ldy) {
    constexpr int BS = Q23<Q3>::BYTES, UNROLL = Gemv23<Q3>::UNROLL;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int K = nb * QK_K;
    uint32_t *xq = reinterpret_cast<uint32_t *>(smem);                                  // [NT nb][64] permuted
    int16_t *xs = reinterpret_cast<int16_t *>(smem + (size_t)NT * K);                   // [NT nb][16], Q2_K only
    float *xd = reinterpret_cast<float *>(smem + (size_t)NT * K + (Q3 ? 0 : (size_t)NT * nb * 32));   // [NT nb]
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int quarter = lane >> 4, t = lane & 15, n4 = t >> 3, i = t & 7, h = i >> 2;
    const int nsteps = (nb + 3) >> 2;
    const int64_t rowbytes = (int64_t)nb * BS;
    const int stride = gridDim.x * (GEMV23_THREADS / 64);
    // (unconditional loads at clamped indices, always inside the matrix: a load under a branch would make the
    // compiler wait for every load in flight, the prefetched batch included, before the first use)
    auto load_batch = [&](int m, int s0, Gemv23Regs<Q3> &r) __attribute__((always_inline)) {
        const uint8_t *row = W + (int64_t)(m < M ? m : M - 1) * rowbytes;
#pragma unroll
        for (int u = 0; u < UNROLL; u++) {
            const int b = 4 * (s0 + u) + quarter;
            // (pointer arithmetic, not an integer round trip: the address stays a global one, no flat load)
            const uint8_t *p = row + (b < nb ? b : nb - 1) * BS;
            if constexpr (Q3) {
                const uint32_t mis = (uint32_t)((uintptr_t)p & 3);           // 0 or 2
                const uint32_t *q = reinterpret_cast<const uint32_t *>(p - mis);
                const int hi = (int)(mis >> 1);
                r.a[u][0] = q[8 + 8 * n4 + i];
                r.a[u][1] = q[8 + 8 * n4 + i + hi];
                r.a[u][2] = q[i];
                r.a[u][3] = q[i + hi];
                r.a[u][4] = q[24];
                r.a[u][5] = q[25];
                r.a[u][6] = q[26];
                r.a[u][7] = q[26 + hi];
                r.a[u][8] = *reinterpret_cast<const uint16_t *>(p + Q23<Q3>::D);
            } else {
                const uint32_t *q = reinterpret_cast<const uint32_t *>(p);
                r.a[u][0] = q[4 + 8 * n4 + i];
                r.a[u][1] = q[2 * n4];
                r.a[u][2] = q[2 * n4 + 1];
                r.a[u][3] = q[t >> 2];
                r.a[u][4] = q[20];
            }
        }
    };
    int m = blockIdx.x * (GEMV23_THREADS / 64) + wave, s0 = 0;
    Gemv23Regs<Q3> cur, nxt;
    {
        // the wave's first x block is requested first and its first weight batch right behind it, so the weights
        // travel while x is quantized; the next x block is requested before the current one is worked on
        const int nblk = NT * nb;
        const float4 *x4 = reinterpret_cast<const float4 *>(x);
        float4 v = x4[(wave < nblk ? wave : nblk - 1) * 64 + lane];
        __builtin_amdgcn_sched_barrier(0);                 // (keeps the x request in front of the weight requests)
        load_batch(m, s0, cur);
        // quantizer lane l holds elements 4l .. 4l + 3: l = 32n + 8k + i
        const int dst = 4 * (8 * (lane >> 5) + (lane & 7)) + ((lane >> 3) & 3);
        // (no branch around the first block, so that its request stays where it is written: a wave beyond the last
        // block repeats the last one and stores the same values again)
        int blk = wave;
        do {
            const int bc = blk < nblk ? blk : nblk - 1, nx = blk + GEMV23_THREADS / 64;
            const float4 vn = x4[(nx < nblk ? nx : nblk - 1) * 64 + lane];
            float d;
            const uint32_t p = q8k_block_lane(v, lane, d);
            xq[bc * 64 + dst] = p;
            if (!Q3) {
                int s16 = __builtin_amdgcn_sdot4((int)p, 0x01010101, 0, false);
                s16 += dpp_i<DPP_QUAD_XOR1>(s16);
                s16 += dpp_i<DPP_QUAD_XOR2>(s16);
                if ((lane & 3) == 0) xs[bc * 16 + (lane >> 2)] = (int16_t)s16;
            }
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
        const bool last = s0 + UNROLL >= nsteps;          // of this row
        const int nm = last ? m + stride : m, ns0 = last ? 0 : s0 + UNROLL;
        load_batch(nm, ns0, nxt);
#pragma unroll
        for (int u = 0; u < UNROLL; u++) {
            // no branch per step: a quarter past the row's end repeats the last block and contributes t_b = +0,
            // which leaves an accumulator that is never -0 unchanged
            const int braw = 4 * (s0 + u) + quarter;
            const bool live = braw < nb;
            const int b = live ? braw : nb - 1;
            const uint32_t *a = cur.a[u];
            uint32_t v[4];
            int sc[4];
            float dw, dmw = 0.0f;
            int mn = 0;
            if constexpr (Q3) {
                // 110 = 2 mod 4: block (m, b) sits at 2 mod 4 exactly when m nb + b is odd
                const uint32_t mis = (uint32_t)(((m & nb) ^ b) & 1) << 1;
                q23_values<Q3>(blk_dword(a[0], a[1], mis), blk_dword(a[2], a[3], mis), n4, v);
                q3_scales(blk_dword(a[4], a[5], mis), blk_dword(a[5], a[6], mis), blk_dword(a[6], a[7], mis), n4, h, sc);
                dw = h2f(a[8]);
            } else {
                q23_values<Q3>(a[0], 0u, n4, v);
                q2_scales(a[1], a[2], h, sc);
                mn = (int)((a[3] >> (8 * (t & 3) + 4)) & 0xFu);
                dw = h2f(a[4] & 0xFFFFu);
                dmw = h2f(a[4] >> 16);
            }
#pragma unroll
            for (int n = 0; n < NT; n++) {
                const int xb = n * nb + b;
                const u32x4 x8 = *reinterpret_cast<const u32x4 *>(xq + xb * 64 + 4 * t);
                int part = sc[0] * __builtin_amdgcn_sdot4((int)v[0], (int)x8.x, 0, false) +
                           sc[1] * __builtin_amdgcn_sdot4((int)v[1], (int)x8.y, 0, false) +
                           sc[2] * __builtin_amdgcn_sdot4((int)v[2], (int)x8.z, 0, false) +
                           sc[3] * __builtin_amdgcn_sdot4((int)v[3], (int)x8.w, 0, false);
                part = row16_sum(part);                                   // isum_b, every lane of the quarter
                const float dx = xd[xb];
                float tb;
                if constexpr (Q3) {
                    tb = __fmul_rn(__fmul_rn(dx, dw), (float)part);
                } else {
                    const int msum = row16_sum(mn * (int)xs[xb * 16 + t]);  // msum_b
                    const float negp = -__fmul_rn(__fmul_rn(dx, dmw), (float)msum);
                    tb = __builtin_fmaf(__fmul_rn(dx, dw), (float)part, negp);
                }
                tb = live ? tb : 0.0f;
                const int tbi = __float_as_int(tb);
                float r = acc[n];
                r = __fadd_rn(r, __int_as_float(__builtin_amdgcn_readlane(tbi, 0)));
                r = __fadd_rn(r, __int_as_float(__builtin_amdgcn_readlane(tbi, 16)));
                r = __fadd_rn(r, __int_as_float(__builtin_amdgcn_readlane(tbi, 32)));
                r = __fadd_rn(r, __int_as_float(__builtin_amdgcn_readlane(tbi, 48)));
                acc[n] = r;
            }
        }
        if (last) {
#pragma unroll
            for (int n = 0; n < NT; n++) {
                if (lane == 0) y[(int64_t)n * ldy + m] = acc[n];
                acc[n] = 0.0f;
            }
        }
        cur = nxt;
        m = nm;
        s0 = ns0;
    }
}

template <bool Q3, int NT>
static hipError_t launch_gemv23(const uint8_t *W, int nb, int M, const float *x, float *y, int64_t ldy, int num_cus,
                                hipStream_t s) {
    const size_t lds = (size_t)NT * (size_t)nb * Gemv23<Q3>::LDS_PER_BLOCK;
    // (the limit for GEMV23_MAX_K, not this launch's lds: it is set once)
    const hipError_t e = raise_dynamic_lds<k_gemv_q23_K<Q3, NT>>(NT * (GEMV23_MAX_K / QK_K) * Gemv23<Q3>::LDS_PER_BLOCK);
    if (e != hipSuccess) return e;
    const int per = GEMV23_THREADS / 64;
    const int64_t want = ((int64_t)M + per - 1) / per;
    // one workgroup per CU; rows beyond the grid are strided (y does not depend on this choice)
    const int64_t cap = (int64_t)(num_cus > 0 ? num_cus : 256);
    (void)hipGetLastError();  // report only this launch's error
    launch_k(k_gemv_q23_K<Q3, NT>, dim3((unsigned)(want < cap ? want : cap)), dim3(GEMV23_THREADS), lds, s, W, nb, M, x, y,
             ldy);
    return hipGetLastError();
}

// any N: column tiles of 8 through the same kernel (each tile is exactly the call on those columns)
template <bool Q3>
static hipError_t gemv_q23_K_t(const void *W, int64_t K, int64_t M, const float *x, int64_t N, float *y, int64_t ldy,
                               const DeviceInfo &dev, hipStream_t s) {
    if (K <= 0 || K % QK_K || K > GEMV23_MAX_K || M < 1 || M >= ((int64_t)1 << 31)) return hipErrorInvalidValue;
    const int nb = (int)(K / QK_K);
    return for_column_tiles(N, 8, [&](int64_t n0, int nt) {
        return with_token_tile(nt, [&](auto NT) {
            return launch_gemv23<Q3, decltype(NT)::value>((const uint8_t *)W, nb, (int)M, x + n0 * K, y + n0 * ldy, ldy,
                                                          dev.num_cus, s);
        });
    });
}

hipError_t gemv_q23_K(bool q3, const void *W, int64_t K, int64_t M, const float *x, int64_t N, float *y, int64_t ldy,
                      const DeviceInfo &dev, hipStream_t s) {
    return q3 ? gemv_q23_K_t<true>(W, K, M, x, N, y, ldy, dev, s) : gemv_q23_K_t<false>(W, K, M, x, N, y, ldy, dev, s);
}

// ---------------------------------------------------------------------------------------------
// Exact mode: y bit-identical to the AVX2 branches of ggml_vec_dot_q3_K_q8_K (k_quants.c:1836-1938) and
// ggml_vec_dot_q2_K_q8_K (1330-1394), fixed fp32 schedules.  Both: per superblock eight int32 lanes, lane L = sum
// over n, k of sc[8n + 2k + (L >= 4)] * sum of q q8 over elements 128n + 32k + 4L .. + 3 (the reference's `is` is
// never advanced: scales[j] selects the half, get_scale_shuffle_q3k(k) puts scale 2k in the low and 2k + 1 in the
// high 128 bits; the int16 steps are exact, |maddubs| <= 1024), then acc_L = fma(d, (float)lane L, acc_L) with d =
// d_x * fp32(d_w), superblocks in order, and hsum_float_8's tree at the end.  Q2_K first adds the mins into the same
// accumulators: prod_L = m[2L] bsums[2L] + m[2L + 1] bsums[2L + 1] (madd_epi16), acc_L = fma(dmin, (float)prod_L,
// acc_L) with dmin = -d_x * fp32(dmin_w).  Eight threads per output run the eight chains; x is the AoS q8_K of
// k_quantize_q8_K.  Idle rows shadow row M - 1 (their shuffles still execute); only live rows store.
static constexpr int EX23_ROWS = 16;

template <bool Q3>
__global__ __launch_bounds__(EX23_ROWS * 8) void k_mm_exact_q23_K(const uint8_t *__restrict__ W, int nb, int M,
                                                                   const uint8_t *__restrict__ xq,
                                                                   float *__restrict__ y, int64_t ldy) {
    constexpr int BS = Q23<Q3>::BYTES;
    const int L = threadIdx.x & 7, r = threadIdx.x >> 3, h = L >> 2;
    const int m = blockIdx.x * EX23_ROWS + r, n = blockIdx.y;
    const bool live = m < M;
    const uint8_t *row = W + (int64_t)(live ? m : M - 1) * nb * BS;
    const uint8_t *xr = xq + (int64_t)n * nb * Q8KB;
    float acc = 0.0f;
    for (int b = 0; b < nb; b++) {
        const uint8_t *p = row + b * BS;
        const uint8_t *xb = xr + b * Q8KB;
        const float dx = *reinterpret_cast<const float *>(xb);
        const uint32_t mis = Q3 ? (uint32_t)((uintptr_t)p & 3) : 0u;
        const uint32_t *q = reinterpret_cast<const uint32_t *>(p - mis);
        const float d = __fmul_rn(dx, h2f(*reinterpret_cast<const uint16_t *>(p + Q23<Q3>::D)));
        uint32_t hm = 0, a0 = 0, a1 = 0, a2 = 0;
        if (Q3) {
            hm = ld_blk_dword(q, mis, L);
            a0 = ld_blk_dword(q, mis, 24);
            a1 = ld_blk_dword(q, mis, 25);
            a2 = ld_blk_dword(q, mis, 26);
        } else {
            const float dmin = __fmul_rn(-dx, h2f(*reinterpret_cast<const uint16_t *>(p + Q23<Q3>::D + 2)));
            const uint32_t mb = (uint32_t)*reinterpret_cast<const uint16_t *>(p + 2 * L);   // scales[2L], [2L + 1]
            const uint32_t bs = *reinterpret_cast<const uint32_t *>(xb + 4 + QK_K + 4 * L);
            const int prod = (int)((mb >> 4) & 0xFu) * (int)(int16_t)(bs & 0xFFFFu) + (int)(mb >> 12) * (int)(int16_t)(bs >> 16);
            acc = __builtin_fmaf(dmin, (float)prod, acc);
        }
        int sumi = 0;
#pragma unroll
        for (int nn = 0; nn < 2; nn++) {
            uint32_t v[4];
            int sc[4];
            q23_values<Q3>(ld_blk_dword(q, mis, Q23<Q3>::QS / 4 + 8 * nn + L), hm, nn, v);
            if (Q3)
                q3_scales(a0, a1, a2, nn, h, sc);
            else
                q2_scales(q[2 * nn], q[2 * nn + 1], h, sc);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t x8 = *reinterpret_cast<const uint32_t *>(xb + 4 + 128 * nn + 32 * k + 4 * L);
                sumi += sc[k] * __builtin_amdgcn_sdot4((int)v[k], (int)x8, 0, false);
            }
        }
        acc = __builtin_fmaf(d, (float)sumi, acc);
    }
    float v = acc;
    v = __fadd_rn(v, __shfl_xor(v, 4, 8));       // r_k = acc_k + acc_{k+4}
    v = __fadd_rn(v, __shfl_xor(v, 2, 8));       // lane 0: r0 + r2, lane 1: r1 + r3
    v = __fadd_rn(v, __shfl_xor(v, 1, 8));       // lane 0: (r0 + r2) + (r1 + r3)
    if (L == 0 && live) y[(int64_t)n * ldy + m] = v;
}

template <bool Q3>
static hipError_t mm_exact_q23_K_t(const void *W, int64_t K, int64_t M, const void *xq8k, int64_t N, float *y,
                                   int64_t ldy, hipStream_t s) {
    if (K <= 0 || K % QK_K || M < 1 || M >= ((int64_t)1 << 31)) return hipErrorInvalidValue;
    return launch_column_chunks(N, [&](int64_t n0, unsigned nn) {
        launch_k(k_mm_exact_q23_K<Q3>, dim3((unsigned)((M + EX23_ROWS - 1) / EX23_ROWS), nn), dim3(EX23_ROWS * 8), 0, s,
                 (const uint8_t *)W, (int)(K / QK_K), (int)M, (const uint8_t *)xq8k + n0 * (K / QK_K) * Q8KB, y + n0 * ldy,
                 ldy);
    });
}

hipError_t mm_exact_q23_K(bool q3, const void *W, int64_t K, int64_t M, const void *xq8k, int64_t N, float *y, int64_t ldy,
                          hipStream_t s) {
    return q3 ? mm_exact_q23_K_t<true>(W, K, M, xq8k, N, y, ldy, s) : mm_exact_q23_K_t<false>(W, K, M, xq8k, N, y, ldy, s);
}

}  // namespace ghip
