// q8_0_w.hip — Q8_0 WEIGHTS x F32 mul_mat (gfx950, wave64): the layer matrices of a "mostly Q8_0" file.
// Shared device helpers: q4_0_device.h (the bit-exact q8_0 quantizer of x, q8_block_lane, the DPP trees).  What
// each kernel restates (reference = ggml.c of Fcucgvhhhvjv/llama.cpp-q_4_0):
//   k_dequantize_q8_0   dequantize_row_q8_0 ggml.c:1594-1610 (bit-exact: (float)q * fp32(d), one multiply)
//   k_gemv_q8_0w<NT>    mul_mat_q_f32 (ggml.c:11353-11411) for NT <= 8 tokens with the q8_0 quantization of x
//                       fused into the prologue (LDS, once per workgroup), COMPUTE = ggml_vec_dot_q8_0_q8_0
//                       with one wave64 per weight row; y within the parity bound
//   k_mm_exact_q8_0w    the AVX2 branch of ggml_vec_dot_q8_0_q8_0 (ggml.c:3231-3320), bit for bit
//   k_prep8_w_q8_0      the k_gemm8 weight image (q4_0_gemm.hip) from Q8_0 rows, so that the prefill GEMM is
//                       gemm8_prep_x + gemm8_run unchanged
//
// Layout: block_q8_0 = fp16 d | int8 qs[32] (34 bytes); a row is 34 K / 32 bytes with K % 64 == 0, so a row and
// every block PAIR (68 bytes, 17 dwords) is 4-byte aligned and nothing more (row stride 68 B at K = 64, 4420 B
// at K = 4160).  Inside a pair: d_A at byte 0, qs_A at bytes 2..33 (2 mod 4: re-aligned with v_alignbyte_b32),
// d_B at byte 34, qs_B at bytes 36..67 (aligned).  64 lanes x 68 B = 4352 B = one K = 4096 row per wave load.
// No load relies on more than 4-byte alignment: the vector loads are typed 4-byte aligned (global_load_dwordx4
// on gfx950 needs dword alignment only, as the q4_0 GEMV's 36-byte pairs already rely on), and the exact
// kernel's words come from the aligned dwords that hold them, always inside the block's pair.
//
// Numerics: a block's integer sum is v_dot4_i32_i8 on SIGNED weights (no offset term; the weight byte -128 is
// legal, the quantizer's activations never hold it): |isum| <= 32 * 128 * 127 < 2^19, exact as int32 and as f32.
#include "q4_0_device.h"

namespace ghip {

static constexpr int Q8W_PAIR = 2 * Q8B;      // 68 bytes

// ---------------------------------------------------------------------------------------------
// block_q8_0 rows -> f32; one thread per four consecutive elements
__global__ __launch_bounds__(256) void k_dequantize_q8_0(const uint8_t *__restrict__ wq, int64_t nquads,
                                                          float *__restrict__ w) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= nquads) return;
    const uint8_t *blk = wq + (idx >> 3) * Q8B;
    const float d = h2f(*reinterpret_cast<const uint16_t *>(blk));
    const int8_t *q = reinterpret_cast<const int8_t *>(blk + 2 + 4 * (idx & 7));
    reinterpret_cast<float4 *>(w)[idx] = make_float4(__fmul_rn((float)q[0], d), __fmul_rn((float)q[1], d),
                                                     __fmul_rn((float)q[2], d), __fmul_rn((float)q[3], d));
}

hipError_t dequantize_q8_0(const void *wq, int64_t K, int64_t M, float *w, hipStream_t s) {
    const int64_t nquads = M * K / 4;
    return launch_1d(k_dequantize_q8_0, nquads, 256, s, (const uint8_t *)wq, nquads, w);
}

// ---------------------------------------------------------------------------------------------
// GEMV, NT <= 8 tokens.  The structure of the q4_0 GEMV (q4_0_gemv.hip) on 68-byte pairs: lane p of a wave owns
// block pair p of its row's 64-pair chunk (17 dwords: four dwordx4 and one dword load at clamped lane
// addresses); the x-waves (the first ceil(NT K / 1024) waves) load x and quantize it to q8_0 into LDS with
// q8_block_lane, in the q4_0 GEMV's chunk-major layout, while the other waves already stream their first DEPTH
// items; after the barrier every wave walks its (row, chunk) items with DEPTH of them in flight.  Per pair and
// token: two exact block sums (8 v_dot4_i32_i8 each) and acc = fma((float)isum, d_w * d_x, acc), pairs in chunk
// order; at a row's end the DPP tree adds the 64 lanes (fixed order).  A lane's accumulation order depends on
// nothing but K, so every launch policy (grid, row mapping, ring depth) and every token count NT gives bitwise
// identical y per column.
static constexpr int G8W_WAVES = 16;
static constexpr int G8W_LDS_MAX = 64 * 1024;
static constexpr int G8W_XPRO = 4;            // x float4 loads in flight per x-wave thread

typedef u32x4 u32x4_a4 __attribute__((aligned(4)));
typedef __attribute__((address_space(1))) const u32x4_a4 g8w_u32x4;
typedef __attribute__((address_space(1))) const uint32_t g8w_u32;

struct Pair8 {
    u32x4 a, b, c, d;
    uint32_t e;
};

__device__ __forceinline__ Pair8 load_pair8(const uint8_t *p68) {
    Pair8 v;
    v.a = *(g8w_u32x4 *)(p68);
    v.b = *(g8w_u32x4 *)(p68 + 16);
    v.c = *(g8w_u32x4 *)(p68 + 32);
    v.d = *(g8w_u32x4 *)(p68 + 48);
    v.e = *(g8w_u32 *)(p68 + 64);
    return v;
}

__device__ __forceinline__ int dot_q8_q8(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t w4, uint32_t w5,
                                         uint32_t w6, uint32_t w7, const u32x4 xl, const u32x4 xh) {
    int s = 0;
    s = __builtin_amdgcn_sdot4((int)w0, (int)xl.x, s, false);
    s = __builtin_amdgcn_sdot4((int)w1, (int)xl.y, s, false);
    s = __builtin_amdgcn_sdot4((int)w2, (int)xl.z, s, false);
    s = __builtin_amdgcn_sdot4((int)w3, (int)xl.w, s, false);
    s = __builtin_amdgcn_sdot4((int)w4, (int)xh.x, s, false);
    s = __builtin_amdgcn_sdot4((int)w5, (int)xh.y, s, false);
    s = __builtin_amdgcn_sdot4((int)w6, (int)xh.z, s, false);
    s = __builtin_amdgcn_sdot4((int)w7, (int)xh.w, s, false);
    return s;
}

template <int NT, int DEPTH>
__global__ __launch_bounds__(G8W_WAVES * 64) void k_gemv_q8_0w(const float *__restrict__ x, const uint8_t *__restrict__ W,
                                                                int nb, int M, int map, float *__restrict__ y,
                                                                int64_t ldy) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    // xq: per token, chunk-major [4][npairs] x 16 B: chunk j = (block & 1) * 2 + word / 4 of pair p = block / 2,
    // so lane p's four ds_read_b128 are lane-contiguous (the q4_0 GEMV's layout)
    uint32_t *xq = lds;                                              // [NT][4][npairs][4] int8x4
    float *xd = reinterpret_cast<float *>(lds + NT * nb * 8);        // [NT][nb]
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grid = gridDim.x;
    const int npairs = nb >> 1;
    const int nchunk = (npairs + 63) >> 6;
    const int64_t rowbytes = (int64_t)nb * Q8B;
    // row -> (workgroup b, wave w): 0 strided, 1 interleaved, 2 blocked (as the q4_0 GEMV)
    int row0, rstride, rend;
    if (map == 2) {                                                  // grid * M < 2^32 (launcher)
        row0 = (int)(((uint32_t)blockIdx.x * (uint32_t)M) / (uint32_t)grid) + wave;
        rend = (int)(((uint32_t)(blockIdx.x + 1) * (uint32_t)M) / (uint32_t)grid);
        rstride = G8W_WAVES;
    } else {
        row0 = map == 1 ? wave * grid + (int)blockIdx.x : (int)blockIdx.x * G8W_WAVES + wave;
        rend = M;
        rstride = grid * G8W_WAVES;
    }
    // the issue cursor: (row, chunk) of the next item to load; past the wave's last row every lane loads the
    // matrix's first pair (one shared address, always inside the matrix)
    int irow = row0, ichunk = 0;
    auto issue = [&]() __attribute__((always_inline)) {
        const bool valid = irow < rend;
        const int pp = 64 * ichunk + lane;
        const int pc = valid ? (pp < npairs ? pp : npairs - 1) : 0;
        const Pair8 v = load_pair8(W + (int64_t)(valid ? irow : 0) * rowbytes + (int64_t)pc * Q8W_PAIR);
        if (++ichunk == nchunk) {
            ichunk = 0;
            irow += rstride;
        }
        return v;
    };

    // ---- INIT: q8_0 of the NT activation rows into LDS.  x of the NT tokens is contiguous ([NT][K] f32), so
    // float4 t is at byte 16 t; unconditional buffer loads (out of range -> 0, no traffic)
    const int total = NT * nb * 8;
    const __amdgpu_buffer_rsrc_t xr = make_rsrc(x, (uint32_t)total * 16u);
    auto quantize_into_lds = [&](const u32x4 &raw, int t) __attribute__((always_inline)) {
        if (t < total) {                                             // whole 8-lane groups agree
            const float4 v = make_float4(__uint_as_float(raw.x), __uint_as_float(raw.y), __uint_as_float(raw.z),
                                         __uint_as_float(raw.w));
            uint32_t d16;
            int qsum;
            const uint32_t packed = q8_block_lane(v, d16, qsum);
            const int n = t / (nb * 8), tw = t - n * (nb * 8);       // token, word within token
            const int b = tw >> 3, w = tw & 7;
            xq[n * nb * 8 + ((((b & 1) << 1) | (w >> 2)) * npairs + (b >> 1)) * 4 + (w & 3)] = packed;
            if ((t & 7) == 0) xd[t >> 3] = h2f(d16);
        }
    };
    Pair8 buf[DEPTH];
    const int XW0 = (total + 64 * G8W_XPRO - 1) / (64 * G8W_XPRO);
    const int XW = XW0 < G8W_WAVES ? XW0 : G8W_WAVES;
    const int XT = XW * 64;
    if (wave < XW) {
        u32x4 xw[G8W_XPRO];
        for (int base = 0; base < total; base += G8W_XPRO * XT) {
#pragma unroll
            for (int i = 0; i < G8W_XPRO; i++)
                xw[i] = __builtin_amdgcn_raw_buffer_load_b128(xr, 16 * (base + tid + i * XT), 0, 0);
#pragma unroll
            for (int i = 0; i < G8W_XPRO; i++) quantize_into_lds(xw[i], base + tid + i * XT);
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
    auto process = [&](const Pair8 &v) __attribute__((always_inline)) {
        const int p = 64 * pchunk + lane;
        if (p < npairs) {
            // even block: d = a.x[15:0], qs = bytes 2..33; odd block: d = c.x[31:16], qs = c.y .. e
            const float dA = h2f(v.a.x & 0xFFFFu);
            const float dB = h2f(v.c.x >> 16);
            const uint32_t a0 = __builtin_amdgcn_alignbyte(v.a.y, v.a.x, 2), a1 = __builtin_amdgcn_alignbyte(v.a.z, v.a.y, 2);
            const uint32_t a2 = __builtin_amdgcn_alignbyte(v.a.w, v.a.z, 2), a3 = __builtin_amdgcn_alignbyte(v.b.x, v.a.w, 2);
            const uint32_t a4 = __builtin_amdgcn_alignbyte(v.b.y, v.b.x, 2), a5 = __builtin_amdgcn_alignbyte(v.b.z, v.b.y, 2);
            const uint32_t a6 = __builtin_amdgcn_alignbyte(v.b.w, v.b.z, 2), a7 = __builtin_amdgcn_alignbyte(v.c.x, v.b.w, 2);
#pragma unroll
            for (int n = 0; n < NT; n++) {
                const float2 dx = *reinterpret_cast<const float2 *>(xd + n * nb + 2 * p);
                const u32x4 *xc = reinterpret_cast<const u32x4 *>(xq + n * nb * 8) + p;
                const int sA = dot_q8_q8(a0, a1, a2, a3, a4, a5, a6, a7, xc[0], xc[npairs]);
                const int sB = dot_q8_q8(v.c.y, v.c.z, v.c.w, v.d.x, v.d.y, v.d.z, v.d.w, v.e, xc[2 * npairs], xc[3 * npairs]);
                acc[n] = fmaf((float)sA, dA * dx.x, acc[n]);
                acc[n] = fmaf((float)sB, dB * dx.y, acc[n]);
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
struct Gemv8wPolicy {
    int map, depth, wg_per_cu;
};
static Gemv8wPolicy &gemv8w_policy() {
    static Gemv8wPolicy p = {env_int("GGML_HIP_Q8_0_GEMV_MAP", -1), env_int("GGML_HIP_Q8_0_GEMV_DEPTH", 0),
                             env_int("GGML_HIP_Q8_0_GEMV_WG_PER_CU", 0)};
    return p;
}
void gemv_q8_0w_set_policy(int map, int depth, int wg_per_cu) { gemv8w_policy() = {map, depth, wg_per_cu}; }

// tokens per launch: the q8_0 of NT tokens (36 bytes per block) in 64 KiB of LDS; 0: K too long for the GEMV
int gemv_q8_0w_max_tokens(int64_t K) {
    const int64_t nb = K / QK;
    if (nb <= 0 || nb >= (1 << 16)) return 0;
    const int64_t nt = G8W_LDS_MAX / (nb * 36);
    return (int)(nt > 8 ? 8 : nt);
}

template <int NT, int DEPTH>
static hipError_t launch_gemv8w(const uint8_t *W, int nb, int64_t M, const float *x, float *y, int64_t ldy, int num_cus,
                                hipStream_t s) {
    const size_t lds = (size_t)NT * nb * 36;
    const int64_t cus = num_cus > 0 ? num_cus : 256;
    const int64_t need = (M + G8W_WAVES - 1) / G8W_WAVES;
    // the q4_0 GEMV's grid rule: one workgroup per CU while that leaves at most two rows per wave, two above; a
    // multiple of the CU count once there is more than one workgroup's rows per CU
    const int wg_env = gemv8w_policy().wg_per_cu;
    int wg_per_cu = wg_env > 0 ? wg_env : (M <= 2 * cus * G8W_WAVES ? 1 : 2);
    if (wg_per_cu > 2) wg_per_cu = 2;                 // 2048 threads per CU (two 64 KiB LDS blocks always fit)
    const int64_t cap = cus * wg_per_cu;
    const int64_t bal = need <= cus ? need : cus * ((need + cus - 1) / cus);
    const int64_t grid = bal < cap ? bal : cap;
    const int map_env = gemv8w_policy().map;
    int map = map_env >= 0 && map_env <= 2 ? map_env
              : ((M % (grid * G8W_WAVES)) % (cus * G8W_WAVES) == 0 ? 0 : (grid > cus ? 1 : 2));
    if (map == 2 && grid * M >= (int64_t)1 << 32) map = 1;           // the kernel's 32-bit row split
    if (grid * G8W_WAVES + M >= (int64_t)1 << 31) return hipErrorInvalidValue;   // 32-bit row indices
    (void)hipGetLastError();  // report only this launch's error
    launch_k((k_gemv_q8_0w<NT, DEPTH>), dim3((unsigned)grid), dim3(G8W_WAVES * 64), lds, s, x, W, nb, (int)M, map, y, ldy);
    return hipGetLastError();
}

template <int NT>
static hipError_t launch_gemv8w_d(const uint8_t *W, int nb, int64_t M, const float *x, float *y, int64_t ldy, int num_cus,
                                  hipStream_t s) {
    // two items in flight per wave: a LLaMA-7B layer's seven N = 1 launches take 59.4 us against 63.8 us at depth 1
    // (tools/q8_0_bench.py under GGML_HIP_Q8_0_GEMV_DEPTH; 11008 -> 4096: 12.4 against 14.4 us); one or two
    // workgroups per CU measured the same
    const int depth = gemv8w_policy().depth;
    return depth == 1 ? launch_gemv8w<NT, 1>(W, nb, M, x, y, ldy, num_cus, s)
                      : launch_gemv8w<NT, 2>(W, nb, M, x, y, ldy, num_cus, s);
}

// any N: column tiles of gemv_q8_0w_max_tokens(K) (8 up to K = 7232) through the same kernel; a column's y does
// not depend on the tile it runs in
hipError_t gemv_q8_0w(const void *W, int64_t K, int64_t M, const float *x, int64_t N, float *y, int64_t ldy,
                      const DeviceInfo &dev, hipStream_t s) {
    const int tile = gemv_q8_0w_max_tokens(K);
    if (K <= 0 || K % 64 || tile < 1 || M < 1 || M >= ((int64_t)1 << 30)) return hipErrorInvalidValue;
    const int nb = (int)(K / QK);
    return for_column_tiles(N, tile, [&](int64_t n0, int nt) {
        return with_token_tile(nt, [&](auto NT) {
            return launch_gemv8w_d<decltype(NT)::value>((const uint8_t *)W, nb, M, x + n0 * K, y + n0 * ldy, ldy, dev.num_cus,
                                                        s);
        });
    });
}

// ---------------------------------------------------------------------------------------------
// Exact mode: y bit-identical to the AVX2 branch of ggml_vec_dot_q8_0_q8_0 (ggml.c:3231-3320), a fixed fp32
// schedule: per block i, lane j = (float)sum_{e = 4j .. 4j + 3} w_e q_e (mul_sum_i8_pairs_float: maddubs of
// |w| with sign-transferred q, pairs at most 2 * 128 * 127 < 32767, so exact; then madd with ones), and
// acc_j = fma(d, lane j, acc_j) with d = fp32(d_w) * fp32(d_x) rounded to f32, blocks in order; hsum_float_8's
// tree at the end.  Eight threads per output run the eight chains.  x is the SoA output of the bit-exact q8_0
// quantizer (qs int8 [N][K], d f32 [N][K / 32] = the fp16-rounded scale as f32).
static constexpr int EX8_ROWS = 16;

__global__ __launch_bounds__(EX8_ROWS * 8) void k_mm_exact_q8_0w(const uint8_t *__restrict__ W, int nb, int M,
                                                                  const int8_t *__restrict__ xqs,
                                                                  const float *__restrict__ xd, float *__restrict__ y,
                                                                  int64_t ldy) {
    const int j = threadIdx.x & 7, r = threadIdx.x >> 3;
    const int m = blockIdx.x * EX8_ROWS + r, n = blockIdx.y;
    const bool live = m < M;
    const uint8_t *row = W + (int64_t)(live ? m : M - 1) * nb * Q8B;      // idle rows shadow the last one (shuffles)
    const uint32_t *xr = reinterpret_cast<const uint32_t *>(xqs + (int64_t)n * nb * QK) + j;
    const float *dr = xd + (int64_t)n * nb;
    float acc = 0.0f;
    for (int b = 0; b < nb; b++) {
        const uint8_t *blk = row + (int64_t)b * Q8B;
        const float d = __fmul_rn(h2f(*reinterpret_cast<const uint16_t *>(blk)), dr[b]);
        // the word at blk + 2 + 4 j: aligned in odd blocks (one dword: nothing past the block is read), at 2 mod 4
        // in even ones (two aligned dwords, both inside the pair)
        const uint8_t *p = blk + 2 + 4 * j;
        const uint32_t mis = (uint32_t)((uintptr_t)p & 3);
        const uint32_t *q = reinterpret_cast<const uint32_t *>(p - mis);   // (pointer arithmetic: stays a global address)
        const uint32_t w4 = __builtin_amdgcn_alignbyte(q[mis >> 1], q[0], mis);
        const int sum = __builtin_amdgcn_sdot4((int)w4, (int)xr[b * 8], 0, false);
        acc = __builtin_fmaf(d, (float)sum, acc);
    }
    float v = acc;
    v = v + __shfl_xor(v, 4, 8);       // r_k = acc_k + acc_{k+4}
    v = v + __shfl_xor(v, 2, 8);       // lane 0: r0 + r2, lane 1: r1 + r3
    v = v + __shfl_xor(v, 1, 8);       // lane 0: (r0 + r2) + (r1 + r3)
    if (j == 0 && live) y[(int64_t)n * ldy + m] = v;
}

hipError_t mm_exact_q8_0w(const void *W, int64_t K, int64_t M, const int8_t *xqs, const float *xd, int64_t N, float *y,
                          int64_t ldy, hipStream_t s) {
    if (K <= 0 || K % 64 || M < 1 || M >= ((int64_t)1 << 30)) return hipErrorInvalidValue;
    return launch_column_chunks(N, [&](int64_t n0, unsigned nn) {
        launch_k(k_mm_exact_q8_0w, dim3((unsigned)((M + EX8_ROWS - 1) / EX8_ROWS), nn), dim3(EX8_ROWS * 8), 0, s,
                 (const uint8_t *)W, (int)(K / QK), (int)M, xqs + n0 * K, xd + n0 * (K / QK), y + n0 * ldy, ldy);
    });
}

// ---------------------------------------------------------------------------------------------
// The k_gemm8 weight image from Q8_0 rows: [M/64][nb][64 rows][32 B] with the 16-byte halves of row r swapped
// when (r >> 3) & 1, + fp16 d_w [M/64][nb][64] (gemm8_w_bytes; the layout k_prep8_w writes from q4_0 rows).  qs
// and d are copied verbatim; rows >= M of the last tile are zeros.  One lane per (row, block pair), a wave = 64
// consecutive rows of one pair (coalesced 2 KiB image stores per block).
__global__ __launch_bounds__(256) void k_prep8_w_q8_0(const uint8_t *__restrict__ W, int64_t rowbytes, int nb, int M,
                                                       int8_t *__restrict__ wimg, uint16_t *__restrict__ wd16) {
    const int r = threadIdx.x & 63;
    const int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);     // (row tile, pair)
    const int npair = nb >> 1;
    const int64_t rt = item / npair;
    const int p = (int)(item - rt * npair);
    const int64_t row = rt * 64 + r;
    if (rt * 64 >= M) return;
    Pair8 v;
    v.a = v.b = v.c = v.d = u32x4{0u, 0u, 0u, 0u};
    v.e = 0u;
    if (row < M) v = load_pair8(W + row * rowbytes + (int64_t)p * Q8W_PAIR);
    const u32x4 e_lo = {__builtin_amdgcn_alignbyte(v.a.y, v.a.x, 2), __builtin_amdgcn_alignbyte(v.a.z, v.a.y, 2),
                        __builtin_amdgcn_alignbyte(v.a.w, v.a.z, 2), __builtin_amdgcn_alignbyte(v.b.x, v.a.w, 2)};
    const u32x4 e_hi = {__builtin_amdgcn_alignbyte(v.b.y, v.b.x, 2), __builtin_amdgcn_alignbyte(v.b.z, v.b.y, 2),
                        __builtin_amdgcn_alignbyte(v.b.w, v.b.z, 2), __builtin_amdgcn_alignbyte(v.c.x, v.b.w, 2)};
    const u32x4 o_lo = {v.c.y, v.c.z, v.c.w, v.d.x};
    const u32x4 o_hi = {v.d.y, v.d.z, v.d.w, v.e};
    const int sw = (r >> 3) & 1;
    const int64_t blk = rt * nb + 2 * p;
    u32x4 *dst = reinterpret_cast<u32x4 *>(wimg + (blk * 64 + r) * 32);
    dst[sw] = e_lo;
    dst[sw ^ 1] = e_hi;
    wd16[blk * 64 + r] = (uint16_t)(v.a.x & 0xFFFFu);
    dst = reinterpret_cast<u32x4 *>(wimg + ((blk + 1) * 64 + r) * 32);
    dst[sw] = o_lo;
    dst[sw ^ 1] = o_hi;
    wd16[(blk + 1) * 64 + r] = (uint16_t)(v.c.x >> 16);
}

hipError_t gemm8_prep_w_q8_0(const void *W, int64_t K, int64_t M, void *wws, hipStream_t s) {
    const int nb = (int)(K / QK);
    const int64_t Mt = (M + 63) / 64;
    int8_t *wimg = (int8_t *)wws;
    uint16_t *wd16 = (uint16_t *)((char *)wws + (size_t)Mt * nb * 2048);
    const int64_t items = Mt * (nb / 2);                  // (row tile, pair) items, 4 per 256-thread block
    if ((items + 3) / 4 >= ((int64_t)1 << 31)) return hipErrorInvalidValue;
    (void)hipGetLastError();
    launch_k(k_prep8_w_q8_0, dim3((unsigned)((items + 3) / 4)), dim3(256), 0, s, (const uint8_t *)W, (int64_t)nb * Q8B, nb,
             (int)M, wimg, wd16);
    return hipGetLastError();
}

}  // namespace ghip
