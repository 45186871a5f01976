// blk32_w.hip — Q8_0, Q4_1, Q5_0 and Q5_1 WEIGHTS x F32 mul_mat (gfx950, wave64): the layer matrices of the "mostly
// Q8_0 / Q4_1 / Q5_0 / Q5_1" files.  The four types are one family: 32 weights per block, an fp16 d in front, K % 64
// == 0, rows made of 4-byte aligned block PAIRS and nothing more.  One kernel of each kind, templates over a traits
// struct that carries only what differs: W8_0, and W5x<QH, MIN> with QH = the block has a fifth bit plane qh (Q5_0,
// Q5_1), MIN = it has a minimum m and multiplies against q8_1 activations (Q4_1, Q5_1).  Shared device helpers:
// q4_0_device.h (the bit-exact q8_0 quantizer of x, q8_block_lane, the DPP trees) and blk32_device.h (a block pair's
// load and decode, shared with the Q4_1 / Q5_1 prefill GEMM q5x_gemm.hip).  What each kernel restates (reference =
// ggml.c of Fcucgvhhhvjv/llama.cpp-q_4_0):
//   k_dequantize_blk32  dequantize_row_q8_0 / q4_1 / q5_0 / q5_1 ggml.c:1520-1610 (bit-exact: one multiply, one add
//                       for MIN)
//   k_quantize_q8_1     quantize_row_q8_1, AVX2 branch ggml.c:1402-1463 (bit-exact: q8_0's bytes, d = amax / 127.f
//                       kept as f32, s = d * (float)sum q)
//   k_gemv_blk32<T, NT> mul_mat_q_f32 (ggml.c:11353-11411) for NT <= 8 tokens with the quantization of x fused into
//                       the prologue (LDS, once per workgroup), one wave64 per weight row; y within the parity bound,
//                       its fp32 order restated in tests/blk32_ref.py
//   k_mm_exact_blk32    the AVX2 branches of ggml_vec_dot_q8_0_q8_0 / q4_1_q8_1 / q5_0_q8_0 / q5_1_q8_1 (ggml.c:
//                       3231-3320, 2680-2713, 2894-2916, 3144-3169), bit for bit
//   k_prep8_w<T>        the k_gemm8 weight image (q4_0_gemm.hip) from q4_0 (nibble - 8), Q8_0 (verbatim) and Q5_0
//                       (q - 16) rows: the values are int8 and the activations q8_0, so the prefill GEMM is
//                       gemm8_prep_x + gemm8_run unchanged
//
// Layouts (ggml.c:877-915): Q8_0 fp16 d, int8 qs[32] (34 bytes) | Q4_1 fp16 d, fp16 m, qs[16] (20) | Q5_0 fp16 d,
// qh[4], qs[16] (22) | Q5_1 fp16 d, fp16 m, qh[4], qs[16] (24).  In the nibble types element j < 16 is the low nibble
// of qs[j], j + 16 the high one; bit e of qh is the fifth bit of element e.  K % 64 == 0, so a row is a whole number
// of block PAIRS of 68 / 40 / 44 / 48 bytes (17 / 10 / 11 / 12 dwords) and every pair is 4-byte aligned and nothing
// more (Q8_0: row stride 68 B at K = 64, 4420 B at K = 4160).  Inside a pair every field of Q4_1 and Q5_1 is dword
// aligned.  Q8_0: d_A at byte 0, qs_A at bytes 2..33 (2 mod 4: re-aligned with v_alignbyte_b32), d_B at byte 34, qs_B
// at bytes 36..67 (aligned); 64 lanes x 68 B = one K = 4096 row per wave load.  Q5_0: the even block has qh at byte 2
// and qs at byte 6 (2 mod 4: re-aligned), the odd block d at byte 22, qh at 24 and qs at 28.  No load relies on more
// than 4-byte alignment: the vector loads are typed 4-byte aligned (global_load_dwordx4 on gfx950 needs dword
// alignment only, as the q4_0 GEMV's 36-byte pairs already rely on), and the exact kernel's words come from the
// aligned dwords that hold them, always inside the block's pair.
//
// Numerics: a block's integer sum is eight v_dot4_i32_i8.  Q8_0: on the SIGNED weights (no offset term; the weight
// byte -128 is legal, the quantizer's activations never hold it): |isum| <= 32 * 128 * 127 < 2^19.  The nibble types:
// on the UNSIGNED 4 / 5-bit values (at most 32 * 31 * 127 < 2^17); Q5_0's offset is applied once per block as -16 *
// sum q_x.  All exact as int32 and as f32.
#include "blk32_device.h"

namespace ghip {

// launch policy overrides of a GEMV (tests sweep them; every policy gives the same y bitwise): map -1 auto / 0 / 1 /
// 2, depth 0 auto / 1 / 2, workgroups per CU 0 auto.  Two instances: Q8_0's, and one for Q4_1 / Q5_0 / Q5_1.
struct GemvPolicy {
    int map, depth, wg_per_cu;
};
static GemvPolicy &policy_q8_0() {
    static GemvPolicy p = {env_int("GGML_HIP_Q8_0_GEMV_MAP", -1), env_int("GGML_HIP_Q8_0_GEMV_DEPTH", 0),
                           env_int("GGML_HIP_Q8_0_GEMV_WG_PER_CU", 0)};
    return p;
}
static GemvPolicy &policy_q5x() {
    static GemvPolicy p = {env_int("GGML_HIP_Q5X_GEMV_MAP", -1), env_int("GGML_HIP_Q5X_GEMV_DEPTH", 0),
                           env_int("GGML_HIP_Q5X_GEMV_WG_PER_CU", 0)};
    return p;
}
void gemv_q8_0w_set_policy(int map, int depth, int wg_per_cu) { policy_q8_0() = {map, depth, wg_per_cu}; }
void gemv_q5x_set_policy(int map, int depth, int wg_per_cu) { policy_q5x() = {map, depth, wg_per_cu}; }

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

// q - 16 per byte of the 5-bit values: bit 4 off, bits 5..7 = !bit 4
__device__ __forceinline__ uint32_t q5_to_i8x4(uint32_t q) { return (q & 0x0F0F0F0Fu) | ((~q & 0x10101010u) * 0xFu); }

// ---------------------------------------------------------------------------------------------
// The traits.  What the kernels below ask of a type T:
//   BLK, PAIR          bytes of a block and of a block pair
//   Pair, load()       a pair in registers and its load at a 4-byte aligned address
//   decode()           a pair -> two BlockX (eight dwords in element order, d, m)
//   MIN                the block has a minimum (the exact kernel's summs chain, the dequantizer's add)
//   XS_DW              dwords per block and token the GEMV keeps in the LDS beside the 32 bytes of q: XBYTES = 32 + 4
//                      XS_DW is 36 for Q8_0 and 40 for the other three (gemv_*_max_tokens depend on it)
//   quantize_x()       the GEMV's x side: one block over 8 lanes -> this lane's packed bytes, the block's scale (raw)
//                      and sum q
//   store_xs()         the block's XS_DW dwords from them (the group's first lane)
//   XScale             a pair's 2 XS_DW dwords as the LDS read that fetches them
//   accumulate()       the GEMV's step per pair and token on the two exact block sums and the pair's XScale
//   exact_word()       the exact kernel's byte vector of elements 4j .. 4j + 3 of a block, as the reference forms it
//   dequant4()         elements 4 sub .. 4 sub + 3 of a block as f32
//   image()            the k_gemm8 image of a pair: the int8 values in element order and the raw fp16 d (the types
//                      k_gemm8 takes only); ZERO_IMAGE: a pair of zero bytes gives an image of zeros
struct W8_0 {
    static constexpr int BLK = Q8B, PAIR = 2 * Q8B, XS_DW = 1;
    static constexpr bool MIN = false, ZERO_IMAGE = true;
    typedef Pair8 Pair;
    static GemvPolicy &policy() { return policy_q8_0(); }
    static __device__ __forceinline__ Pair load(const uint8_t *p) { return load_pair8(p); }
    static __device__ __forceinline__ void decode(const Pair &v, BlockX &A, BlockX &B) { q8_0_decode_pair(v, A, B); }
    // d_x = the fp16-rounded scale as f32
    static __device__ __forceinline__ uint32_t quantize_x(float4 v, uint32_t &d, int &qsum) { return q8_block_lane(v, d, qsum); }
    static __device__ __forceinline__ void store_xs(uint32_t *xs, uint32_t d16, int) { xs[0] = __float_as_uint(h2f(d16)); }
    typedef float2 XScale;                                                                // d_A, d_B
    static __device__ __forceinline__ float accumulate(float acc, const BlockX &A, const BlockX &B, int sA, int sB,
                                                       const XScale dx) {
        acc = fmaf((float)sA, A.d * dx.x, acc);
        return fmaf((float)sB, B.d * dx.y, acc);
    }
    // the word at blk + 2 + 4 j: aligned in odd blocks (one dword: nothing past the block is read), at 2 mod 4 in
    // even ones (two aligned dwords, both inside the pair)
    static __device__ __forceinline__ uint32_t exact_word(const uint8_t *blk, int j) { return blk32_ld32(blk + 2 + 4 * j); }
    static __device__ __forceinline__ float4 dequant4(const uint8_t *blk, int sub, float d) {
        const int8_t *q = reinterpret_cast<const int8_t *>(blk + 2 + 4 * sub);
        return make_float4(__fmul_rn((float)q[0], d), __fmul_rn((float)q[1], d), __fmul_rn((float)q[2], d),
                           __fmul_rn((float)q[3], d));
    }
    static __device__ __forceinline__ void image(const Pair &v, uint32_t *a, uint32_t *b, uint32_t &dA, uint32_t &dB) {
        BlockX A, B;
        q8_0_decode_pair(v, A, B);
#pragma unroll
        for (int i = 0; i < 8; i++) {
            a[i] = A.q[i];
            b[i] = B.q[i];
        }
        dA = v.a.x & 0xFFFFu;
        dB = v.c.x >> 16;
    }
};

template <bool QH, bool MN>
struct W5x : Q5x<QH, MN> {
    using G = Q5x<QH, MN>;
    static constexpr int XS_DW = 2;
    static constexpr bool MIN = MN, ZERO_IMAGE = false;     // q = 0 is -16 in the image
    typedef PairX<G::DW> Pair;
    static GemvPolicy &policy() { return policy_q5x(); }
    static __device__ __forceinline__ Pair load(const uint8_t *p) { return load_pairx<G::DW>(p); }
    static __device__ __forceinline__ void decode(const Pair &v, BlockX &A, BlockX &B) { q5x_decode_pair<QH, MN>(v, A, B); }
    // MIN: the unrounded f32 d_x and s_x = d_x * (float)sum q; Q5_0: the fp16-rounded d_x as f32 and the integer 16 *
    // sum q
    static __device__ __forceinline__ uint32_t quantize_x(float4 v, uint32_t &d, int &qsum) {
        float df;
        const uint32_t packed = q81_block_lane(v, df, qsum);
        d = __float_as_uint(df);
        return packed;
    }
    static __device__ __forceinline__ void store_xs(uint32_t *xs, uint32_t d, int qsum) {
        if (MN) {
            xs[0] = d;
            xs[1] = __float_as_uint(__fmul_rn(__uint_as_float(d), (float)qsum));
        } else {
            xs[0] = __float_as_uint(h2f(f2h(__uint_as_float(d))));
            xs[1] = (uint32_t)(16 * qsum);
        }
    }
    // acc = fma((float)isum, d_w * d_x, acc);   MIN: acc = fma(m_w, s_x, acc)   immediately after it, which keeps the
    // two large, opposite terms of a block adjacent in the chain
    typedef u32x4 XScale;                                                                 // d_A, s_A, d_B, s_B
    static __device__ __forceinline__ float accumulate(float acc, const BlockX &A, const BlockX &B, int sA, int sB,
                                                       const XScale sx) {
        if (!MN) {
            sA -= (int)sx.y;
            sB -= (int)sx.w;
        }
        acc = fmaf((float)sA, A.d * __uint_as_float(sx.x), acc);
        if (MN) acc = fmaf(A.m, __uint_as_float(sx.y), acc);
        acc = fmaf((float)sB, B.d * __uint_as_float(sx.z), acc);
        if (MN) acc = fmaf(B.m, __uint_as_float(sx.w), acc);
        return acc;
    }
    // Q5_0: nibble | (bit ? 0 : 0xF0) read as int8 = q - 16; the others the unsigned value.  The words are at 0 or 2
    // mod 4: one aligned dword, or two that are both inside the block's pair
    static __device__ __forceinline__ uint32_t exact_word(const uint8_t *blk, int j) {
        const uint32_t qs = blk32_ld32(blk + G::OFF_QS + 4 * (j & 3));
        uint32_t w4 = (j < 4 ? qs : qs >> 4) & 0x0F0F0F0Fu;
        if (QH) {
            const uint32_t hi = q5x_spread4(blk32_ld32(blk + G::OFF_QH), 4 * j);
            w4 |= MN ? hi : (~hi & 0x10101010u) * 0xFu;
        }
        return w4;
    }
    static __device__ __forceinline__ float4 dequant4(const uint8_t *blk, int sub, float d) {
        const uint32_t qs = blk32_ld32(blk + G::OFF_QS + 4 * (sub & 3));
        uint32_t q4 = (sub < 4 ? qs : qs >> 4) & 0x0F0F0F0Fu;
        if (QH) q4 |= q5x_spread4(blk32_ld32(blk + G::OFF_QH), 4 * sub);
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int q = (int)((q4 >> (8 * k)) & 0xFFu);
            if (MN)
                v[k] = __fadd_rn(__fmul_rn((float)q, d), h2f(*reinterpret_cast<const uint16_t *>(blk + 2)));
            else
                v[k] = __fmul_rn((float)(q - 16), d);
        }
        return make_float4(v[0], v[1], v[2], v[3]);
    }
    static __device__ __forceinline__ void image(const Pair &v, uint32_t *a, uint32_t *b, uint32_t &dA, uint32_t &dB) {
        static_assert(QH && !MN, "k_gemm8 takes Q5_0 only: one term per block, q8_0 activations");
        BlockX A, B;
        q5x_decode_pair<true, false>(v, A, B);
#pragma unroll
        for (int i = 0; i < 8; i++) {
            a[i] = q5_to_i8x4(A.q[i]);
            b[i] = q5_to_i8x4(B.q[i]);
        }
        dA = v.w[0] & 0xFFFFu;
        dB = v.w[5] >> 16;
    }
};

// q4_0 (fp16 d, qs[16]: 18 bytes, 36-byte pairs) has kernels of its own (q4_0_gemv.hip, q4_0_exact.hip); here it is
// a source of the k_gemm8 image only.  Block 2p: d = w0[15:0], qs = bytes 2..17; block 2p + 1: d = w4[31:16], qs = w5
// .. w8
struct W4_0 {
    static constexpr int BLK = Q4B, PAIR = 2 * Q4B;
    static constexpr bool ZERO_IMAGE = false;               // the nibble 0 is -8 in the image
    typedef PairX<9> Pair;
    static __device__ __forceinline__ Pair load(const uint8_t *p) { return load_pairx<9>(p); }
    static __device__ __forceinline__ void image(const Pair &v, uint32_t *a, uint32_t *b, uint32_t &dA, uint32_t &dB) {
        const uint32_t *w = v.w;
        const uint32_t e[4] = {__builtin_amdgcn_alignbyte(w[1], w[0], 2), __builtin_amdgcn_alignbyte(w[2], w[1], 2),
                               __builtin_amdgcn_alignbyte(w[3], w[2], 2), __builtin_amdgcn_alignbyte(w[4], w[3], 2)};
#pragma unroll
        for (int i = 0; i < 4; i++) {                       // elements 0..15 (low nibbles), 16..31 (high)
            a[i] = nib_to_i8x4(e[i], 0);
            a[4 + i] = nib_to_i8x4(e[i], 4);
            b[i] = nib_to_i8x4(w[5 + i], 0);
            b[4 + i] = nib_to_i8x4(w[5 + i], 4);
        }
        dA = w[0] & 0xFFFFu;
        dB = w[4] >> 16;
    }
};

// ---------------------------------------------------------------------------------------------
// rows -> f32; one thread per four consecutive elements
template <class T>
__global__ __launch_bounds__(256) void k_dequantize_blk32(const uint8_t *__restrict__ wq, int64_t nquads,
                                                           float *__restrict__ w) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= nquads) return;
    const uint8_t *blk = wq + (idx >> 3) * T::BLK;
    const float d = h2f(*reinterpret_cast<const uint16_t *>(blk));
    reinterpret_cast<float4 *>(w)[idx] = T::dequant4(blk, (int)(idx & 7), d);
}

template <class T>
static hipError_t dequantize_blk32(const void *wq, int64_t K, int64_t M, float *w, hipStream_t s) {
    const int64_t nquads = M * K / 4;
    return launch_1d(k_dequantize_blk32<T>, nquads, 256, s, (const uint8_t *)wq, nquads, w);
}

hipError_t dequantize_q8_0(const void *wq, int64_t K, int64_t M, float *w, hipStream_t s) {
    return dequantize_blk32<W8_0>(wq, K, M, w, s);
}

hipError_t dequantize_q5x(bool qh, bool mn, const void *wq, int64_t K, int64_t M, float *w, hipStream_t s) {
    if (!mn) return dequantize_blk32<W5x<true, false>>(wq, K, M, w, s);
    return qh ? dequantize_blk32<W5x<true, true>>(wq, K, M, w, s) : dequantize_blk32<W5x<false, true>>(wq, K, M, w, s);
}

// ---------------------------------------------------------------------------------------------
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
// GEMV, NT <= 8 tokens.  The structure of the q4_0 GEMV (q4_0_gemv.hip) on 68 / 40 / 44 / 48-byte pairs: lane p of a
// wave owns block pair p of its row's 64-pair chunk (17 / 10 / 11 / 12 dwords at clamped lane addresses); the x-waves
// (the first ceil(NT K / 1024) waves) load x and quantize it into LDS (T::quantize_x), in the q4_0 GEMV's chunk-major
// layout, while the other waves already stream their first DEPTH items; after the barrier every wave walks its (row,
// chunk) items with DEPTH of them in flight.  Beside the bytes the LDS holds T::XS_DW dwords per block and token.  Per
// pair and token: two exact block sums (8 v_dot4_i32_i8 each) and T::accumulate, pairs in chunk order; at a row's end
// the DPP tree adds the 64 lanes (fixed order).  A lane's accumulation order depends on nothing but K, so every
// launch policy (grid, row mapping, ring depth) and every token count NT gives bitwise identical y per column.
static constexpr int GB_WAVES = 16;
static constexpr int GB_LDS_MAX = 64 * 1024;
static constexpr int GB_XPRO = 4;             // x float4 loads in flight per x-wave thread

__device__ __forceinline__ int blk32_dot(const BlockX &b, const u32x4 xl, const u32x4 xh) {
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

template <class T, int NT, int DEPTH>
__global__ __launch_bounds__(GB_WAVES * 64) void k_gemv_blk32(const float *__restrict__ x, const uint8_t *__restrict__ W,
                                                               int nb, int M, int map, float *__restrict__ y,
                                                               int64_t ldy) {
    typedef typename T::Pair Pair;
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    // xq: per token, chunk-major [4][npairs] x 16 B: chunk j = (block & 1) * 2 + word / 4 of pair p = block / 2,
    // so lane p's four ds_read_b128 are lane-contiguous (the q4_0 GEMV's layout)
    uint32_t *xq = lds;                                              // [NT][4][npairs][4] int8x4
    uint32_t *xs = lds + NT * nb * 8;                                // [NT][nb][XS_DW]
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
        rstride = GB_WAVES;
    } else {
        row0 = map == 1 ? wave * grid + (int)blockIdx.x : (int)blockIdx.x * GB_WAVES + wave;
        rend = M;
        rstride = grid * GB_WAVES;
    }
    // the issue cursor: (row, chunk) of the next item to load; past the wave's last row every lane loads the
    // matrix's first pair (one shared address, always inside the matrix)
    int irow = row0, ichunk = 0;
    auto issue = [&]() __attribute__((always_inline)) {
        const bool valid = irow < rend;
        const int pp = 64 * ichunk + lane;
        const int pc = valid ? (pp < npairs ? pp : npairs - 1) : 0;
        const Pair v = T::load(W + (int64_t)(valid ? irow : 0) * rowbytes + (int64_t)pc * T::PAIR);
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
            uint32_t d;
            int qsum;
            const uint32_t packed = T::quantize_x(v, d, qsum);
            const int n = t / (nb * 8), tw = t - n * (nb * 8);       // token, word within token
            const int b = tw >> 3, w = tw & 7;
            xq[n * nb * 8 + ((((b & 1) << 1) | (w >> 2)) * npairs + (b >> 1)) * 4 + (w & 3)] = packed;
            if ((t & 7) == 0) T::store_xs(xs + T::XS_DW * (t >> 3), d, qsum);
        }
    };
    Pair buf[DEPTH];
    const int XW0 = (total + 64 * GB_XPRO - 1) / (64 * GB_XPRO);
    const int XW = XW0 < GB_WAVES ? XW0 : GB_WAVES;
    const int XT = XW * 64;
    if (wave < XW) {
        u32x4 xw[GB_XPRO];
        for (int base = 0; base < total; base += GB_XPRO * XT) {
#pragma unroll
            for (int i = 0; i < GB_XPRO; i++)
                xw[i] = __builtin_amdgcn_raw_buffer_load_b128(xr, 16 * (base + tid + i * XT), 0, 0);
#pragma unroll
            for (int i = 0; i < GB_XPRO; i++) quantize_into_lds(xw[i], base + tid + i * XT);
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
            T::decode(v, A, B);
#pragma unroll
            for (int n = 0; n < NT; n++) {
                const typename T::XScale sx = *reinterpret_cast<const typename T::XScale *>(xs + T::XS_DW * (n * nb) + T::XS_DW * (2 * p));
                const u32x4 *xc = reinterpret_cast<const u32x4 *>(xq + n * nb * 8) + p;
                const int sA = blk32_dot(A, xc[0], xc[npairs]);
                const int sB = blk32_dot(B, xc[2 * npairs], xc[3 * npairs]);
                acc[n] = T::accumulate(acc[n], A, B, sA, sB, sx);
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

// tokens per launch: the quantized x of NT tokens (36 bytes per block for Q8_0, 40 for the others) in 64 KiB of LDS; 0:
// K too long for the GEMV
template <class T>
static int gemv_max_tokens_blk32(int64_t K) {
    const int64_t nb = K / QK;
    if (nb <= 0 || nb >= (1 << 16)) return 0;
    const int64_t nt = GB_LDS_MAX / (nb * (32 + 4 * T::XS_DW));
    return (int)(nt > 8 ? 8 : nt);
}
int gemv_q8_0w_max_tokens(int64_t K) { return gemv_max_tokens_blk32<W8_0>(K); }
int gemv_q5x_max_tokens(int64_t K) { return gemv_max_tokens_blk32<W5x<true, true>>(K); }

template <class T, int NT, int DEPTH>
static hipError_t launch_gemv_blk32(const uint8_t *W, int nb, int64_t M, const float *x, float *y, int64_t ldy, int num_cus,
                                    hipStream_t s) {
    const size_t lds = (size_t)NT * nb * (32 + 4 * T::XS_DW);
    const int64_t cus = num_cus > 0 ? num_cus : 256;
    const int64_t need = (M + GB_WAVES - 1) / GB_WAVES;
    // the q4_0 GEMV's grid rule: one workgroup per CU while that leaves at most two rows per wave, two above; a
    // multiple of the CU count once there is more than one workgroup's rows per CU
    const int wg_env = T::policy().wg_per_cu;
    int wg_per_cu = wg_env > 0 ? wg_env : (M <= 2 * cus * GB_WAVES ? 1 : 2);
    if (wg_per_cu > 2) wg_per_cu = 2;                 // 2048 threads per CU (two 64 KiB LDS blocks always fit)
    const int64_t cap = cus * wg_per_cu;
    const int64_t bal = need <= cus ? need : cus * ((need + cus - 1) / cus);
    const int64_t grid = bal < cap ? bal : cap;
    const int map_env = T::policy().map;
    int map = map_env >= 0 && map_env <= 2 ? map_env
              : ((M % (grid * GB_WAVES)) % (cus * GB_WAVES) == 0 ? 0 : (grid > cus ? 1 : 2));
    if (map == 2 && grid * M >= (int64_t)1 << 32) map = 1;           // the kernel's 32-bit row split
    if (grid * GB_WAVES + M >= (int64_t)1 << 31) return hipErrorInvalidValue;   // 32-bit row indices
    (void)hipGetLastError();  // report only this launch's error
    launch_k((k_gemv_blk32<T, NT, DEPTH>), dim3((unsigned)grid), dim3(GB_WAVES * 64), lds, s, x, W, nb, (int)M, map, y, ldy);
    return hipGetLastError();
}

// any N: column tiles of the type's max tokens (8 up to K = 7232 for Q8_0, 6528 for the others) through the same
// kernel; a column's y does not depend on the tile it runs in
template <class T>
static hipError_t gemv_blk32(const void *W, int64_t K, int64_t M, const float *x, int64_t N, float *y, int64_t ldy,
                             const DeviceInfo &dev, hipStream_t s) {
    const int tile = gemv_max_tokens_blk32<T>(K);
    if (K <= 0 || K % 64 || tile < 1 || M < 1 || M >= ((int64_t)1 << 30)) return hipErrorInvalidValue;
    const int nb = (int)(K / QK);
    // two items in flight per wave unless forced: a LLaMA-7B layer's seven Q8_0 N = 1 launches take 59.4 us against
    // 63.8 us at depth 1 (tools/q8_0_bench.py under GGML_HIP_Q8_0_GEMV_DEPTH; 11008 -> 4096: 12.4 against 14.4 us);
    // one or two workgroups per CU measured the same
    const bool d1 = T::policy().depth == 1;
    return for_column_tiles(N, tile, [&](int64_t n0, int nt) {
        return with_token_tile(nt, [&](auto NT) {
            constexpr int NTV = decltype(NT)::value;
            return d1 ? launch_gemv_blk32<T, NTV, 1>((const uint8_t *)W, nb, M, x + n0 * K, y + n0 * ldy, ldy, dev.num_cus, s)
                      : launch_gemv_blk32<T, NTV, 2>((const uint8_t *)W, nb, M, x + n0 * K, y + n0 * ldy, ldy, dev.num_cus, s);
        });
    });
}

hipError_t gemv_q8_0w(const void *W, int64_t K, int64_t M, const float *x, int64_t N, float *y, int64_t ldy,
                      const DeviceInfo &dev, hipStream_t s) {
    return gemv_blk32<W8_0>(W, K, M, x, N, y, ldy, dev, s);
}

hipError_t gemv_q5x(bool qh, bool mn, const void *W, int64_t K, int64_t M, const float *x, int64_t N, float *y,
                    int64_t ldy, const DeviceInfo &dev, hipStream_t s) {
    if (!mn) return gemv_blk32<W5x<true, false>>(W, K, M, x, N, y, ldy, dev, s);
    return qh ? gemv_blk32<W5x<true, true>>(W, K, M, x, N, y, ldy, dev, s)
              : gemv_blk32<W5x<false, true>>(W, K, M, x, N, y, ldy, dev, s);
}

// ---------------------------------------------------------------------------------------------
// Exact mode: y bit-identical to the AVX2 branch of the type's ggml_vec_dot, a fixed fp32 schedule: per block i,
// lane j = (float)sum_{e = 4j .. 4j + 3} w_e q_e with w the byte vector the reference forms (T::exact_word; maddubs
// pairs at most 2 * 128 * 127 < 32767, so exact; then madd with ones), and acc_j = fma(d, lane j, acc_j) with d =
// fp32(d_w) * d_x rounded to f32, blocks in order; hsum_float_8's tree at the end.  Eight threads per output run the
// eight chains.  For MIN lane 0 also carries summs += fp32(m) * s, which the compiled reference forms as a multiply
// rounded to f32 and an add (its fixtures reject the fma form), and adds it last.  x is the SoA output of the
// bit-exact quantizers: qs int8 [N][K], d f32 [N][K / 32] (q8_0's fp16-rounded scale as f32 for Q8_0 and Q5_0, q8_1's
// unrounded one for MIN), s f32 [N][K / 32] (MIN only).
static constexpr int EXB_ROWS = 16;

template <class T>
__global__ __launch_bounds__(EXB_ROWS * 8) void k_mm_exact_blk32(const uint8_t *__restrict__ W, int nb, int M,
                                                                  const int8_t *__restrict__ xqs,
                                                                  const float *__restrict__ xd,
                                                                  const float *__restrict__ xsum, float *__restrict__ y,
                                                                  int64_t ldy) {
    const int j = threadIdx.x & 7, r = threadIdx.x >> 3;
    const int m = blockIdx.x * EXB_ROWS + r, n = blockIdx.y;
    const bool live = m < M;
    const uint8_t *row = W + (int64_t)(live ? m : M - 1) * nb * T::BLK;   // idle rows shadow the last one (shuffles)
    const uint32_t *xr = reinterpret_cast<const uint32_t *>(xqs + (int64_t)n * nb * QK) + j;
    const float *dr = xd + (int64_t)n * nb;
    const float *sr = T::MIN ? xsum + (int64_t)n * nb : nullptr;
    float acc = 0.0f, summs = 0.0f;
    for (int b = 0; b < nb; b++) {
        const uint8_t *blk = row + (int64_t)b * T::BLK;
        const float d = __fmul_rn(h2f(*reinterpret_cast<const uint16_t *>(blk)), dr[b]);
        const int sum = __builtin_amdgcn_sdot4((int)T::exact_word(blk, j), (int)xr[b * 8], 0, false);
        acc = __builtin_fmaf(d, (float)sum, acc);
        if (T::MIN && j == 0)
            summs = __fadd_rn(summs, __fmul_rn(h2f(*reinterpret_cast<const uint16_t *>(blk + 2)), sr[b]));
    }
    float v = acc;
    v = v + __shfl_xor(v, 4, 8);       // r_k = acc_k + acc_{k+4}
    v = v + __shfl_xor(v, 2, 8);       // lane 0: r0 + r2, lane 1: r1 + r3
    v = v + __shfl_xor(v, 1, 8);       // lane 0: (r0 + r2) + (r1 + r3)
    if (T::MIN) v = __fadd_rn(v, summs);
    if (j == 0 && live) y[(int64_t)n * ldy + m] = v;
}

template <class T>
static hipError_t mm_exact_blk32(const void *W, int64_t K, int64_t M, const int8_t *xqs, const float *xd, const float *xsum,
                                 int64_t N, float *y, int64_t ldy, hipStream_t s) {
    if (K <= 0 || K % 64 || M < 1 || M >= ((int64_t)1 << 30)) return hipErrorInvalidValue;
    const int nb = (int)(K / QK);
    return launch_column_chunks(N, [&](int64_t n0, unsigned nn) {
        launch_k(k_mm_exact_blk32<T>, dim3((unsigned)((M + EXB_ROWS - 1) / EXB_ROWS), nn), dim3(EXB_ROWS * 8), 0, s,
                 (const uint8_t *)W, nb, (int)M, xqs + n0 * K, xd + n0 * nb, T::MIN ? xsum + n0 * nb : nullptr,
                 y + n0 * ldy, ldy);
    });
}

hipError_t mm_exact_q8_0w(const void *W, int64_t K, int64_t M, const int8_t *xqs, const float *xd, int64_t N, float *y,
                          int64_t ldy, hipStream_t s) {
    return mm_exact_blk32<W8_0>(W, K, M, xqs, xd, nullptr, N, y, ldy, s);
}

hipError_t mm_exact_q5x(bool qh, bool mn, const void *W, int64_t K, int64_t M, const int8_t *xqs, const float *xd,
                        const float *xsum, int64_t N, float *y, int64_t ldy, hipStream_t s) {
    if (!mn) return mm_exact_blk32<W5x<true, false>>(W, K, M, xqs, xd, xsum, N, y, ldy, s);
    return qh ? mm_exact_blk32<W5x<true, true>>(W, K, M, xqs, xd, xsum, N, y, ldy, s)
              : mm_exact_blk32<W5x<false, true>>(W, K, M, xqs, xd, xsum, N, y, ldy, s);
}

// ---------------------------------------------------------------------------------------------
// The k_gemm8 weight image: [M/64][nb][64 rows][32 B] with the 16-byte halves of row r swapped when (r >> 3) & 1, so
// that a 1 KiB DMA lands 32 rows of one block in the conflict-free operand layout, + fp16 d_w [M/64][nb][64]
// (gemm8_w_bytes).  The bytes are the block's int8 values in element order (T::image), d is copied verbatim; rows >= M
// of the last tile are zeros (d = 0).  One lane per (row, block pair), a wave = 64 consecutive rows of one pair
// (coalesced 2 KiB image stores per block).
template <class T>
__global__ __launch_bounds__(256) void k_prep8_w(const uint8_t *__restrict__ W, int64_t rowbytes, int nb, int M,
                                                  int8_t *__restrict__ wimg, uint16_t *__restrict__ wd16) {
    const int r = threadIdx.x & 63;
    const int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);     // (row tile, pair)
    const int npair = nb >> 1;
    const int64_t rt = item / npair;
    const int p = (int)(item - rt * npair);
    const int64_t row = rt * 64 + r;
    if (rt * 64 >= M) return;
    const bool live = row < M;
    // a dead row stores zeros: where the image of a pair of zeros is zeros (Q8_0) it skips the load; elsewhere it reads
    // the matrix's first pair (inside the matrix) and masks the result
    typename T::Pair v = {};
    uint32_t keep = 0xFFFFFFFFu;
    if constexpr (T::ZERO_IMAGE) {
        if (live) v = T::load(W + row * rowbytes + (int64_t)p * T::PAIR);
    } else {
        v = T::load(W + (live ? row * rowbytes + (int64_t)p * T::PAIR : 0));
        keep = live ? 0xFFFFFFFFu : 0u;
    }
    uint32_t a[8], b[8], dA, dB;
    T::image(v, a, b, dA, dB);
#pragma unroll
    for (int i = 0; i < 8; i++) {
        a[i] &= keep;
        b[i] &= keep;
    }
    const int sw = (r >> 3) & 1;
    const int64_t blk = rt * nb + 2 * p;
    u32x4 *dst = reinterpret_cast<u32x4 *>(wimg + (blk * 64 + r) * 32);
    dst[sw] = u32x4{a[0], a[1], a[2], a[3]};
    dst[sw ^ 1] = u32x4{a[4], a[5], a[6], a[7]};
    wd16[blk * 64 + r] = (uint16_t)(dA & keep);
    dst = reinterpret_cast<u32x4 *>(wimg + ((blk + 1) * 64 + r) * 32);
    dst[sw] = u32x4{b[0], b[1], b[2], b[3]};
    dst[sw ^ 1] = u32x4{b[4], b[5], b[6], b[7]};
    wd16[(blk + 1) * 64 + r] = (uint16_t)(dB & keep);
}

template <class T>
static hipError_t prep8_w(const void *W, int64_t K, int64_t M, void *wws, hipStream_t s) {
    const int nb = (int)(K / QK);
    const int64_t Mt = (M + 63) / 64;
    int8_t *wimg = (int8_t *)wws;
    uint16_t *wd16 = (uint16_t *)((char *)wws + (size_t)Mt * nb * 2048);
    const int64_t items = Mt * (nb / 2);                  // (row tile, pair) items, 4 per 256-thread block
    if ((items + 3) / 4 >= ((int64_t)1 << 31)) return hipErrorInvalidValue;
    (void)hipGetLastError();
    launch_k(k_prep8_w<T>, dim3((unsigned)((items + 3) / 4)), dim3(256), 0, s, (const uint8_t *)W, (int64_t)nb * T::BLK, nb,
             (int)M, wimg, wd16);
    return hipGetLastError();
}

hipError_t gemm8_prep_w(const void *W, int64_t K, int64_t M, void *wws, hipStream_t s) { return prep8_w<W4_0>(W, K, M, wws, s); }
hipError_t gemm8_prep_w_q8_0(const void *W, int64_t K, int64_t M, void *wws, hipStream_t s) {
    return prep8_w<W8_0>(W, K, M, wws, s);
}
hipError_t gemm8_prep_w_q5_0(const void *W, int64_t K, int64_t M, void *wws, hipStream_t s) {
    return prep8_w<W5x<true, false>>(W, K, M, wws, s);
}

}  // namespace ghip
