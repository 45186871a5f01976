// q5x_w.hip — Q4_1, Q5_0 and Q5_1 WEIGHTS x F32 mul_mat (gfx950, wave64): the layer matrices of the "mostly Q4_1 /
// Q5_0 / Q5_1" files.  One kernel family, templates over <QH, MIN>: QH = the block has a fifth bit plane qh (Q5_0,
// Q5_1), MIN = it has a minimum m and multiplies against q8_1 activations (Q4_1, Q5_1).  Shared device helpers:
// q4_0_device.h and q5x_device.h (a block pair's load and decode, shared with the Q4_1 / Q5_1 prefill GEMM
// q5x_gemm.hip).  What each kernel restates (reference = ggml.c of Fcucgvhhhvjv/llama.cpp-q_4_0):
//   k_dequantize_q5x    dequantize_row_q4_1 / q5_0 / q5_1 ggml.c:1520-1592 (bit-exact: one multiply, one add for MIN)
//   k_quantize_q8_1     quantize_row_q8_1, AVX2 branch ggml.c:1402-1463 (bit-exact: q8_0's bytes, d = amax / 127.f
//                       kept as f32, s = d * (float)sum q)
//   k_gemv_q5x<NT>      mul_mat_q_f32 (ggml.c:11353-11411) for NT <= 8 tokens with the quantization of x fused into
//                       the prologue (LDS, once per workgroup), one wave64 per weight row; y within the parity bound
//   k_mm_exact_q5x      the AVX2 branches of ggml_vec_dot_q4_1_q8_1 / q5_0_q8_0 / q5_1_q8_1 (ggml.c:2680-2713,
//                       2894-2916, 3144-3169), bit for bit
//   k_prep8_w_q5_0      the k_gemm8 weight image (q4_0_gemm.hip) from Q5_0 rows: q - 16 is an int8 and the
//                       activations are q8_0, so the prefill GEMM is gemm8_prep_x + gemm8_run unchanged
//
// Layouts (ggml.c:877-900), 32 weights per block: Q4_1 fp16 d, fp16 m, qs[16] (20 bytes) | Q5_0 fp16 d, qh[4],
// qs[16] (22) | Q5_1 fp16 d, fp16 m, qh[4], qs[16] (24).  Element j < 16 is the low nibble of qs[j], j + 16 the high
// one; bit e of qh is the fifth bit of element e.  K % 64 == 0, so a row is a whole number of block PAIRS of 40 /
// 44 / 48 bytes (10 / 11 / 12 dwords) and every pair is 4-byte aligned and nothing more.  Inside a pair every field
// of Q4_1 and Q5_1 is dword aligned; Q5_0's even block has qh at byte 2 and qs at byte 6 (2 mod 4: re-aligned with
// v_alignbyte_b32), its odd block d at byte 22, qh at 24 and qs at 28.  No load relies on more than 4-byte
// alignment: the vector loads are typed 4-byte aligned, and the exact kernel's words come from the aligned dwords
// that hold them, always inside the block's pair.
//
// Numerics: a block's integer sum is eight v_dot4_i32_i8 on the UNSIGNED 4 / 5-bit values (at most 32 * 31 * 127 <
// 2^17, exact); Q5_0's offset is applied once per block as -16 * sum q_x.
#include "q5x_device.h"

namespace ghip {

// four bytes at a 2-byte aligned address from the aligned dwords that hold them (one dword when p is aligned)
__device__ __forceinline__ uint32_t q5x_ld32(const uint8_t *p) {
    const uint32_t mis = (uint32_t)((uintptr_t)p & 3);
    const uint32_t *q = reinterpret_cast<const uint32_t *>(p - mis);
    return __builtin_amdgcn_alignbyte(q[mis >> 1], q[0], mis);
}

// ---------------------------------------------------------------------------------------------
// rows -> f32; one thread per four consecutive elements
template <bool QH, bool MIN>
__global__ __launch_bounds__(256) void k_dequantize_q5x(const uint8_t *__restrict__ wq, int64_t nquads,
                                                         float *__restrict__ w) {
    using T = Q5x<QH, MIN>;
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= nquads) return;
    const uint8_t *blk = wq + (idx >> 3) * T::BLK;
    const int sub = (int)(idx & 7);
    const float d = h2f(*reinterpret_cast<const uint16_t *>(blk));
    const uint32_t qs = q5x_ld32(blk + T::OFF_QS + 4 * (sub & 3));
    uint32_t q4 = (sub < 4 ? qs : qs >> 4) & 0x0F0F0F0Fu;
    if (QH) q4 |= q5x_spread4(q5x_ld32(blk + T::OFF_QH), 4 * sub);
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int q = (int)((q4 >> (8 * k)) & 0xFFu);
        if (MIN)
            v[k] = __fadd_rn(__fmul_rn((float)q, d), h2f(*reinterpret_cast<const uint16_t *>(blk + 2)));
        else
            v[k] = __fmul_rn((float)(q - 16), d);
    }
    reinterpret_cast<float4 *>(w)[idx] = make_float4(v[0], v[1], v[2], v[3]);
}

hipError_t dequantize_q5x(bool qh, bool mn, const void *wq, int64_t K, int64_t M, float *w, hipStream_t s) {
    const int64_t nquads = M * K / 4;
    if (!mn) return launch_1d(k_dequantize_q5x<true, false>, nquads, 256, s, (const uint8_t *)wq, nquads, w);
    return qh ? launch_1d(k_dequantize_q5x<true, true>, nquads, 256, s, (const uint8_t *)wq, nquads, w)
              : launch_1d(k_dequantize_q5x<false, true>, nquads, 256, s, (const uint8_t *)wq, nquads, w);
}

// ---------------------------------------------------------------------------------------------
// One q8_1 block spread over 8 consecutive lanes, 4 floats each: q8_block_lane's bytes and sum, the scale
// d = amax / 127.f unrounded.
__device__ __forceinline__ uint32_t q81_block_lane(float4 v, float &d, int &qsum) {
    float a = fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w)));
    a = group8_max(a);
    d = a / 127.f;                                     // correctly rounded (no fast-math)
    const float id = (a != 0.0f) ? 127.f / a : 0.0f;
    const int q0 = q8_round_sat(v.x * id), q1 = q8_round_sat(v.y * id);
    const int q2 = q8_round_sat(v.z * id), q3 = q8_round_sat(v.w * id);
    qsum = group8_sum(q0 + q1 + q2 + q3);
    return (uint32_t)(q0 & 0xFF) | ((uint32_t)(q1 & 0xFF) << 8) | ((uint32_t)(q2 & 0xFF) << 16) |
           ((uint32_t)(q3 & 0xFF) << 24);
}

// q8_1 activation quantizer.  One lane per 4 floats, 8 lanes per block.  AOS: block_q8_1 rows (f32 d, f32 s,
// qs[32]: 40 bytes); else qs int8 [N][K], d f32 [N][K / 32], s f32 [N][K / 32]
template <bool AOS>
__global__ __launch_bounds__(256) void k_quantize_q8_1(const float *__restrict__ x, int64_t total8,
                                                        uint8_t *__restrict__ aos, int8_t *__restrict__ qs,
                                                        float *__restrict__ dout, float *__restrict__ sout) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total8) return;                           // total8 % 8 == 0: whole groups exit together
    const int64_t blk = t >> 3;
    const int sub = (int)(t & 7);
    const float4 v = *reinterpret_cast<const float4 *>(x + t * 4);
    float d;
    int qsum;
    const uint32_t packed = q81_block_lane(v, d, qsum);
    const float sx = __fmul_rn(d, (float)qsum);
    if (AOS) {
        uint32_t *o = reinterpret_cast<uint32_t *>(aos + blk * 40);
        o[2 + sub] = packed;
        if (sub == 0) {
            o[0] = __float_as_uint(d);
            o[1] = __float_as_uint(sx);
        }
    } else {
        reinterpret_cast<uint32_t *>(qs)[t] = packed;
        if (sub == 0) {
            dout[blk] = d;
            sout[blk] = sx;
        }
    }
}

hipError_t quantize_q8_1_aos(const float *x, int64_t K, int64_t N, void *xq, hipStream_t s) {
    const int64_t total8 = N * (K / QK) * 8;
    return launch_1d(k_quantize_q8_1<true>, total8, 256, s, x, total8, (uint8_t *)xq, (int8_t *)nullptr, (float *)nullptr,
                     (float *)nullptr);
}

hipError_t quantize_q8_1_soa(const float *x, int64_t K, int64_t N, int8_t *qs, float *d, float *sx, hipStream_t s) {
    const int64_t total8 = N * (K / QK) * 8;
    return launch_1d(k_quantize_q8_1<false>, total8, 256, s, x, total8, (uint8_t *)nullptr, qs, d, sx);
}

// ---------------------------------------------------------------------------------------------
// GEMV, NT <= 8 tokens.  The structure of the Q8_0 GEMV (q8_0_w.hip) on 40 / 44 / 48-byte pairs: lane p of a wave
// owns block pair p of its row's 64-pair chunk (10 / 11 / 12 dwords at clamped lane addresses); the x-waves load x
// and quantize it into LDS in the q4_0 GEMV's chunk-major layout, while the other waves already stream their first
// DEPTH items; after the barrier every wave walks its (row, chunk) items with DEPTH of them in flight.  Beside the
// bytes the LDS holds, per block and token, 8 bytes: for MIN the unrounded f32 d_x and s_x = d_x * (float)sum q; for
// Q5_0 the fp16-rounded d_x as f32 and the integer 16 * sum q.  Per block and token: one exact integer sum and
//   acc = fma((float)isum, d_w * d_x, acc);   MIN: acc = fma(m_w, s_x, acc)   immediately after it,
// which keeps the two large, opposite terms of a block adjacent in the chain; pairs in chunk order; at a row's end
// the DPP tree adds the 64 lanes (fixed order).  A lane's accumulation order depends on nothing but K, so every
// launch policy (grid, row mapping, ring depth) and every token count NT gives bitwise identical y per column.
static constexpr int G5X_WAVES = 16;
static constexpr int G5X_LDS_MAX = 64 * 1024;
static constexpr int G5X_XPRO = 4;            // x float4 loads in flight per x-wave thread
static constexpr int G5X_XBYTES = 40;         // LDS bytes per block and token

__device__ __forceinline__ int q5x_dot(const BlockX &b, const u32x4 xl, const u32x4 xh) {
    int s = 0;
    s = __builtin_amdgcn_sdot4((int)b.q[0], (int)xl.x, s, false);
    s = __builtin_amdgcn_sdot4((int)b.q[1], (int)xl.y, s, false);
    s = __builtin_amdgcn_sdot4((int)b.q[2], (int)xl.z, s, false);
    s = __builtin_amdgcn_sdot4((int)b.q[3], (int)xl.w, s, false);
    s = __builtin_amdgcn_sdot4((int)b.q[4], (int)xh.x, s, false);
    s = __builtin_amdgcn_sdot4((int)b.q[5], (int)xh.y, s, false);
    s = __builtin_amdgcn_sdot4((int)b.q[6], (int)xh.z, s, false);
    s = __builtin_amdgcn_sdot4((int)b.q[7], (int)xh.w, s, false);
    return s;
}

template <bool QH, bool MIN, int NT, int DEPTH>
__global__ __launch_bounds__(G5X_WAVES * 64) void k_gemv_q5x(const float *__restrict__ x, const uint8_t *__restrict__ W,
                                                              int nb, int M, int map, float *__restrict__ y,
                                                              int64_t ldy) {
    using T = Q5x<QH, MIN>;
    typedef PairX<T::DW> Pair;
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    // xq: per token, chunk-major [4][npairs] x 16 B: chunk j = (block & 1) * 2 + word / 4 of pair p = block / 2,
    // so lane p's four ds_read_b128 are lane-contiguous (the q4_0 GEMV's layout)
    uint32_t *xq = lds;                                              // [NT][4][npairs][4] int8x4
    uint32_t *xs = lds + NT * nb * 8;                                // [NT][nb][2]: d_x | s_x or 16 * sum q
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grid = gridDim.x;
    const int npairs = nb >> 1;
    const int nchunk = (npairs + 63) >> 6;
    const int64_t rowbytes = (int64_t)nb * T::BLK;
    // row -> (workgroup b, wave w): 0 strided, 1 interleaved, 2 blocked (as the q4_0 GEMV)
    int row0, rstride, rend;
    if (map == 2) {                                                  // grid * M < 2^32 (launcher)
        row0 = (int)(((uint32_t)blockIdx.x * (uint32_t)M) / (uint32_t)grid) + wave;
        rend = (int)(((uint32_t)(blockIdx.x + 1) * (uint32_t)M) / (uint32_t)grid);
        rstride = G5X_WAVES;
    } else {
        row0 = map == 1 ? wave * grid + (int)blockIdx.x : (int)blockIdx.x * G5X_WAVES + wave;
        rend = M;
        rstride = grid * G5X_WAVES;
    }
    // the issue cursor: (row, chunk) of the next item to load; past the wave's last row every lane loads the
    // matrix's first pair (one shared address, always inside the matrix)
    int irow = row0, ichunk = 0;
    auto issue = [&]() __attribute__((always_inline)) {
        const bool valid = irow < rend;
        const int pp = 64 * ichunk + lane;
        const int pc = valid ? (pp < npairs ? pp : npairs - 1) : 0;
        const Pair v = load_pairx<T::DW>(W + (int64_t)(valid ? irow : 0) * rowbytes + (int64_t)pc * T::PAIR);
        if (++ichunk == nchunk) {
            ichunk = 0;
            irow += rstride;
        }
        return v;
    };

    // ---- INIT: the quantization of the NT activation rows into LDS.  x of the NT tokens is contiguous ([NT][K]
    // f32), so float4 t is at byte 16 t; unconditional buffer loads (out of range -> 0, no traffic)
    const int total = NT * nb * 8;
    const __amdgpu_buffer_rsrc_t xr = make_rsrc(x, (uint32_t)total * 16u);
    auto quantize_into_lds = [&](const u32x4 &raw, int t) __attribute__((always_inline)) {
        if (t < total) {                                             // whole 8-lane groups agree
            const float4 v = make_float4(__uint_as_float(raw.x), __uint_as_float(raw.y), __uint_as_float(raw.z),
                                         __uint_as_float(raw.w));
            float d;
            int qsum;
            const uint32_t packed = q81_block_lane(v, d, qsum);
            const int n = t / (nb * 8), tw = t - n * (nb * 8);       // token, word within token
            const int b = tw >> 3, w = tw & 7;
            xq[n * nb * 8 + ((((b & 1) << 1) | (w >> 2)) * npairs + (b >> 1)) * 4 + (w & 3)] = packed;
            if ((t & 7) == 0) {
                if (MIN) {
                    xs[2 * (t >> 3)] = __float_as_uint(d);
                    xs[2 * (t >> 3) + 1] = __float_as_uint(__fmul_rn(d, (float)qsum));
                } else {
                    xs[2 * (t >> 3)] = __float_as_uint(h2f(f2h(d)));
                    xs[2 * (t >> 3) + 1] = (uint32_t)(16 * qsum);
                }
            }
        }
    };
    Pair buf[DEPTH];
    const int XW0 = (total + 64 * G5X_XPRO - 1) / (64 * G5X_XPRO);
    const int XW = XW0 < G5X_WAVES ? XW0 : G5X_WAVES;
    const int XT = XW * 64;
    if (wave < XW) {
        u32x4 xw[G5X_XPRO];
        for (int base = 0; base < total; base += G5X_XPRO * XT) {
#pragma unroll
            for (int i = 0; i < G5X_XPRO; i++)
                xw[i] = __builtin_amdgcn_raw_buffer_load_b128(xr, 16 * (base + tid + i * XT), 0, 0);
#pragma unroll
            for (int i = 0; i < G5X_XPRO; i++) quantize_into_lds(xw[i], base + tid + i * XT);
        }
        asm volatile("" ::: "memory");                               // weight loads stay behind x
    }
#pragma unroll
    for (int d = 0; d < DEPTH; d++) buf[d] = issue();
    __syncthreads();

    // ---- COMPUTE
    float acc[NT];
#pragma unroll
    for (int n = 0; n < NT; n++) acc[n] = 0.0f;
    int prow = row0, pchunk = 0;
    auto process = [&](const Pair &v) __attribute__((always_inline)) {
        const int p = 64 * pchunk + lane;
        if (p < npairs) {
            BlockX A, B;
            q5x_decode_pair<QH, MIN>(v, A, B);
#pragma unroll
            for (int n = 0; n < NT; n++) {
                const u32x4 sx = *reinterpret_cast<const u32x4 *>(xs + 2 * (n * nb + 2 * p));   // d_A, s_A, d_B, s_B
                const u32x4 *xc = reinterpret_cast<const u32x4 *>(xq + n * nb * 8) + p;
                int sA = q5x_dot(A, xc[0], xc[npairs]);
                int sB = q5x_dot(B, xc[2 * npairs], xc[3 * npairs]);
                if (!MIN) {
                    sA -= (int)sx.y;
                    sB -= (int)sx.w;
                }
                acc[n] = fmaf((float)sA, A.d * __uint_as_float(sx.x), acc[n]);
                if (MIN) acc[n] = fmaf(A.m, __uint_as_float(sx.y), acc[n]);
                acc[n] = fmaf((float)sB, B.d * __uint_as_float(sx.z), acc[n]);
                if (MIN) acc[n] = fmaf(B.m, __uint_as_float(sx.w), acc[n]);
            }
        }
        if (++pchunk == nchunk) {                                    // row complete: reduce + store
            typedef __attribute__((address_space(1))) float gfloat;
            float out = 0.0f;
#pragma unroll
            for (int n = 0; n < NT; n++) {
                const float t = wave_sum_lane63(acc[n]);
                const float tn = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(t), 63));
                out = (lane == n) ? tn : out;
                acc[n] = 0.0f;
            }
            if (lane < NT) ((gfloat *)y)[(int64_t)lane * ldy + prow] = out;
            pchunk = 0;
            prow += rstride;
        }
    };
    while (prow < rend) {                                            // wave-uniform
#pragma unroll
        for (int d = 0; d < DEPTH; d++) {
            if (prow >= rend) break;
            process(buf[d]);
            buf[d] = issue();
        }
    }
}

// launch policy overrides (tests sweep them; every policy gives the same y bitwise): map -1 auto / 0 / 1 / 2,
// depth 0 auto / 1 / 2, workgroups per CU 0 auto
struct Gemv5xPolicy {
    int map, depth, wg_per_cu;
};
static Gemv5xPolicy &gemv5x_policy() {
    static Gemv5xPolicy p = {env_int("GGML_HIP_Q5X_GEMV_MAP", -1), env_int("GGML_HIP_Q5X_GEMV_DEPTH", 0),
                             env_int("GGML_HIP_Q5X_GEMV_WG_PER_CU", 0)};
    return p;
}
void gemv_q5x_set_policy(int map, int depth, int wg_per_cu) { gemv5x_policy() = {map, depth, wg_per_cu}; }

// tokens per launch: the quantized x of NT tokens (40 bytes per block) in 64 KiB of LDS; 0: K too long for the GEMV
int gemv_q5x_max_tokens(int64_t K) {
    const int64_t nb = K / QK;
    if (nb <= 0 || nb >= (1 << 16)) return 0;
    const int64_t nt = G5X_LDS_MAX / (nb * G5X_XBYTES);
    return (int)(nt > 8 ? 8 : nt);
}

template <bool QH, bool MIN, int NT, int DEPTH>
static hipError_t launch_gemv5x(const uint8_t *W, int nb, int64_t M, const float *x, float *y, int64_t ldy, int num_cus,
                                hipStream_t s) {
    const size_t lds = (size_t)NT * nb * G5X_XBYTES;
    const int64_t cus = num_cus > 0 ? num_cus : 256;
    const int64_t need = (M + G5X_WAVES - 1) / G5X_WAVES;
    // the q4_0 GEMV's grid rule: one workgroup per CU while that leaves at most two rows per wave, two above; a
    // multiple of the CU count once there is more than one workgroup's rows per CU
    const int wg_env = gemv5x_policy().wg_per_cu;
    int wg_per_cu = wg_env > 0 ? wg_env : (M <= 2 * cus * G5X_WAVES ? 1 : 2);
    if (wg_per_cu > 2) wg_per_cu = 2;                 // 2048 threads per CU (two 64 KiB LDS blocks always fit)
    const int64_t cap = cus * wg_per_cu;
    const int64_t bal = need <= cus ? need : cus * ((need + cus - 1) / cus);
    const int64_t grid = bal < cap ? bal : cap;
    const int map_env = gemv5x_policy().map;
    int map = map_env >= 0 && map_env <= 2 ? map_env
              : ((M % (grid * G5X_WAVES)) % (cus * G5X_WAVES) == 0 ? 0 : (grid > cus ? 1 : 2));
    if (map == 2 && grid * M >= (int64_t)1 << 32) map = 1;           // the kernel's 32-bit row split
    if (grid * G5X_WAVES + M >= (int64_t)1 << 31) return hipErrorInvalidValue;   // 32-bit row indices
    (void)hipGetLastError();  // report only this launch's error
    launch_k((k_gemv_q5x<QH, MIN, NT, DEPTH>), dim3((unsigned)grid), dim3(G5X_WAVES * 64), lds, s, x, W, nb, (int)M, map, y,
             ldy);
    return hipGetLastError();
}

template <bool QH, bool MIN>
static hipError_t gemv_q5x_t(const void *W, int64_t K, int64_t M, const float *x, int64_t N, float *y, int64_t ldy,
                             const DeviceInfo &dev, hipStream_t s) {
    const int tile = gemv_q5x_max_tokens(K);
    if (K <= 0 || K % 64 || tile < 1 || M < 1 || M >= ((int64_t)1 << 30)) return hipErrorInvalidValue;
    const int nb = (int)(K / QK);
    const bool d1 = gemv5x_policy().depth == 1;       // two items in flight per wave unless forced (as the Q8_0 GEMV)
    return for_column_tiles(N, tile, [&](int64_t n0, int nt) {
        return with_token_tile(nt, [&](auto NT) {
            constexpr int T = decltype(NT)::value;
            return d1 ? launch_gemv5x<QH, MIN, T, 1>((const uint8_t *)W, nb, M, x + n0 * K, y + n0 * ldy, ldy, dev.num_cus, s)
                      : launch_gemv5x<QH, MIN, T, 2>((const uint8_t *)W, nb, M, x + n0 * K, y + n0 * ldy, ldy, dev.num_cus, s);
        });
    });
}

// any N: column tiles of gemv_q5x_max_tokens(K) (8 up to K = 6528) through the same kernel; a column's y does not
// depend on the tile it runs in
hipError_t gemv_q5x(bool qh, bool mn, const void *W, int64_t K, int64_t M, const float *x, int64_t N, float *y,
                    int64_t ldy, const DeviceInfo &dev, hipStream_t s) {
    if (!mn) return gemv_q5x_t<true, false>(W, K, M, x, N, y, ldy, dev, s);
    return qh ? gemv_q5x_t<true, true>(W, K, M, x, N, y, ldy, dev, s) : gemv_q5x_t<false, true>(W, K, M, x, N, y, ldy, dev, s);
}

// ---------------------------------------------------------------------------------------------
// Exact mode: y bit-identical to the AVX2 branch of the type's ggml_vec_dot, a fixed fp32 schedule: per block i,
// lane j = (float)sum_{e = 4j .. 4j + 3} w_e q_e with w the byte vector the reference forms (Q5_0: nibble | (bit ? 0 :
// 0xF0) read as int8 = q - 16; the others the unsigned value; maddubs pairs at most 2 * 31 * 127 < 32767, so exact),
// and acc_j = fma(d, lane j, acc_j) with d = fp32(d_w) * d_x rounded to f32, blocks in order; hsum_float_8's tree at
// the end.  Eight threads per output run the eight chains.  For MIN lane 0 also carries summs += fp32(m) * s, which
// the compiled reference forms as a multiply rounded to f32 and an add (its fixtures reject the fma form), and adds
// it last.  x is the SoA output of the bit-exact quantizers: qs int8 [N][K], d f32 [N][K / 32] (q8_0's fp16-rounded
// scale for Q5_0, q8_1's unrounded one for MIN), s f32 [N][K / 32] (MIN only).
static constexpr int EX5X_ROWS = 16;

template <bool QH, bool MIN>
__global__ __launch_bounds__(EX5X_ROWS * 8) void k_mm_exact_q5x(const uint8_t *__restrict__ W, int nb, int M,
                                                                 const int8_t *__restrict__ xqs,
                                                                 const float *__restrict__ xd,
                                                                 const float *__restrict__ xsum, float *__restrict__ y,
                                                                 int64_t ldy) {
    using T = Q5x<QH, MIN>;
    const int j = threadIdx.x & 7, r = threadIdx.x >> 3;
    const int m = blockIdx.x * EX5X_ROWS + r, n = blockIdx.y;
    const bool live = m < M;
    const uint8_t *row = W + (int64_t)(live ? m : M - 1) * nb * T::BLK;   // idle rows shadow the last one (shuffles)
    const uint32_t *xr = reinterpret_cast<const uint32_t *>(xqs + (int64_t)n * nb * QK) + j;
    const float *dr = xd + (int64_t)n * nb;
    const float *sr = MIN ? xsum + (int64_t)n * nb : nullptr;
    float acc = 0.0f, summs = 0.0f;
    for (int b = 0; b < nb; b++) {
        const uint8_t *blk = row + (int64_t)b * T::BLK;
        const float d = __fmul_rn(h2f(*reinterpret_cast<const uint16_t *>(blk)), dr[b]);
        // the words are at 0 or 2 mod 4: one aligned dword, or two that are both inside the block's pair
        const uint32_t qs = q5x_ld32(blk + T::OFF_QS + 4 * (j & 3));
        uint32_t w4 = (j < 4 ? qs : qs >> 4) & 0x0F0F0F0Fu;
        if (QH) {
            const uint32_t hi = q5x_spread4(q5x_ld32(blk + T::OFF_QH), 4 * j);
            w4 |= MIN ? hi : (~hi & 0x10101010u) * 0xFu;
        }
        const int sum = __builtin_amdgcn_sdot4((int)w4, (int)xr[b * 8], 0, false);
        acc = __builtin_fmaf(d, (float)sum, acc);
        if (MIN && j == 0)
            summs = __fadd_rn(summs, __fmul_rn(h2f(*reinterpret_cast<const uint16_t *>(blk + 2)), sr[b]));
    }
    float v = acc;
    v = v + __shfl_xor(v, 4, 8);       // r_k = acc_k + acc_{k+4}
    v = v + __shfl_xor(v, 2, 8);       // lane 0: r0 + r2, lane 1: r1 + r3
    v = v + __shfl_xor(v, 1, 8);       // lane 0: (r0 + r2) + (r1 + r3)
    if (MIN) v = __fadd_rn(v, summs);
    if (j == 0 && live) y[(int64_t)n * ldy + m] = v;
}

hipError_t mm_exact_q5x(bool qh, bool mn, const void *W, int64_t K, int64_t M, const int8_t *xqs, const float *xd,
                        const float *xsum, int64_t N, float *y, int64_t ldy, hipStream_t s) {
    if (K <= 0 || K % 64 || M < 1 || M >= ((int64_t)1 << 30)) return hipErrorInvalidValue;
    const int nb = (int)(K / QK);
    return launch_column_chunks(N, [&](int64_t n0, unsigned nn) {
        const dim3 grid((unsigned)((M + EX5X_ROWS - 1) / EX5X_ROWS), nn), block(EX5X_ROWS * 8);
        const int8_t *q = xqs + n0 * K;
        const float *d = xd + n0 * nb, *sx = mn ? xsum + n0 * nb : nullptr;
        float *yo = y + n0 * ldy;
        if (!mn)
            launch_k((k_mm_exact_q5x<true, false>), grid, block, 0, s, (const uint8_t *)W, nb, (int)M, q, d, sx, yo, ldy);
        else if (qh)
            launch_k((k_mm_exact_q5x<true, true>), grid, block, 0, s, (const uint8_t *)W, nb, (int)M, q, d, sx, yo, ldy);
        else
            launch_k((k_mm_exact_q5x<false, true>), grid, block, 0, s, (const uint8_t *)W, nb, (int)M, q, d, sx, yo, ldy);
    });
}

// ---------------------------------------------------------------------------------------------
// The k_gemm8 weight image from Q5_0 rows: [M/64][nb][64 rows][32 B] with the 16-byte halves of row r swapped when
// (r >> 3) & 1, + fp16 d_w [M/64][nb][64] (gemm8_w_bytes; the layout k_prep8_w_q8_0 writes).  The bytes are q - 16
// in element order, d is copied verbatim; rows >= M of the last tile are zeros.  One lane per (row, block pair), a
// wave = 64 consecutive rows of one pair.
__global__ __launch_bounds__(256) void k_prep8_w_q5_0(const uint8_t *__restrict__ W, int64_t rowbytes, int nb, int M,
                                                       int8_t *__restrict__ wimg, uint16_t *__restrict__ wd16) {
    using T = Q5x<true, false>;
    const int r = threadIdx.x & 63;
    const int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);     // (row tile, pair)
    const int npair = nb >> 1;
    const int64_t rt = item / npair;
    const int p = (int)(item - rt * npair);
    const int64_t row = rt * 64 + r;
    if (rt * 64 >= M) return;
    const bool live = row < M;
    // a dead row reads the matrix's first pair (inside the matrix) and stores zeros
    const PairX<T::DW> v = load_pairx<T::DW>(W + (live ? row * rowbytes + (int64_t)p * T::PAIR : 0));
    BlockX A, B;
    q5x_decode_pair<true, false>(v, A, B);
    const uint32_t keep = live ? 0xFFFFFFFFu : 0u;
    uint32_t a[8], b[8];
#pragma unroll
    for (int i = 0; i < 8; i++) {                           // q - 16 per byte: bit 4 off, bits 5..7 = !bit 4
        a[i] = ((A.q[i] & 0x0F0F0F0Fu) | ((~A.q[i] & 0x10101010u) * 0xFu)) & keep;
        b[i] = ((B.q[i] & 0x0F0F0F0Fu) | ((~B.q[i] & 0x10101010u) * 0xFu)) & keep;
    }
    const int sw = (r >> 3) & 1;
    const int64_t blk = rt * nb + 2 * p;
    u32x4 *dst = reinterpret_cast<u32x4 *>(wimg + (blk * 64 + r) * 32);
    dst[sw] = u32x4{a[0], a[1], a[2], a[3]};
    dst[sw ^ 1] = u32x4{a[4], a[5], a[6], a[7]};
    wd16[blk * 64 + r] = (uint16_t)(v.w[0] & 0xFFFFu & keep);
    dst = reinterpret_cast<u32x4 *>(wimg + ((blk + 1) * 64 + r) * 32);
    dst[sw] = u32x4{b[0], b[1], b[2], b[3]};
    dst[sw ^ 1] = u32x4{b[4], b[5], b[6], b[7]};
    wd16[(blk + 1) * 64 + r] = (uint16_t)((v.w[5] >> 16) & keep);
}

hipError_t gemm8_prep_w_q5_0(const void *W, int64_t K, int64_t M, void *wws, hipStream_t s) {
    const int nb = (int)(K / QK);
    const int64_t Mt = (M + 63) / 64;
    int8_t *wimg = (int8_t *)wws;
    uint16_t *wd16 = (uint16_t *)((char *)wws + (size_t)Mt * nb * 2048);
    const int64_t items = Mt * (nb / 2);                  // (row tile, pair) items, 4 per 256-thread block
    if ((items + 3) / 4 >= ((int64_t)1 << 31)) return hipErrorInvalidValue;
    (void)hipGetLastError();
    launch_k(k_prep8_w_q5_0, dim3((unsigned)((items + 3) / 4)), dim3(256), 0, s, (const uint8_t *)W, (int64_t)nb * 22, nb,
             (int)M, wimg, wd16);
    return hipGetLastError();
}

}  // namespace ghip
