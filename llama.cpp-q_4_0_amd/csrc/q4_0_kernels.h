// q4_0_kernels.h — launchers for the gfx950 q4_0 x q8_0 kernels (internal to libggml_hip.so).
//
// Data layouts in HBM:
//   W   : ggml block_q4_0 rows, verbatim (ggml.c:870-875): row m at W + m*rowbytes,
//         rowbytes = 18*K/32; block = fp16 d + 16 bytes of nibbles (elem j: low nibble
//         of qs[j], elem j+16: high nibble).  Never repacked.
//   x   : f32 [N][K] (ggml src1, nb10 == 4).
//   y   : f32 [N][ldy] (ggml dst, y[n*ldy + m]).
//   xq8 : ggml block_q8_0 rows (ggml.c:902-907), AoS, 34*K/32 bytes per token — the
//         reference's INIT wdata layout; produced by quantize_q8_0_aos.
//   xs  : internal GEMM operand: int8 qs [N][K] + f32 d [N][K/32] (fp32 value of the
//         fp16-rounded scale), produced by quantize_q8_0_soa from the same device
//         quantizer; bit-identical q8_0 values.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ghip {

struct DeviceInfo {
    int num_cus;
};

// A5 (AVX2 branch semantics, bit-exact): x f32 [N][K] -> block_q8_0 AoS [N][K/32].
hipError_t quantize_q8_0_aos(const float *x, int64_t K, int64_t N, void *xq8, hipStream_t s);
// Same quantizer, GEMM operand layout.
hipError_t quantize_q8_0_soa(const float *x, int64_t K, int64_t N, int8_t *qs, float *d, hipStream_t s,
                             uint16_t *d16 = nullptr);   // d16: optional fp16 copy of d, block-major [K/32][N]
// A3 (quantize_row_q4_0_reference semantics, bit-exact): w f32 [M][K] -> block_q4_0 rows.
hipError_t quantize_q4_0(const float *w, int64_t K, int64_t M, void *wq, hipStream_t s);
// A4: block_q4_0 rows -> f32 [M][K].
hipError_t dequantize_q4_0(const void *wq, int64_t K, int64_t M, float *w, hipStream_t s);

// Decode / small-batch path: fused q8_0 quantize of x (in LDS) + q4_0.q8_0 GEMV.
// N <= gemv_max_tokens(K).
int gemv_max_tokens(int64_t K);
hipError_t gemv_q4_0(const void *W, int64_t K, int64_t M, const float *x, int64_t N,
                     float *y, int64_t ldy, const DeviceInfo &dev, hipStream_t s);

// Sibling mul_mats sharing x (e.g. wq/wk/wv): up to 4 matrices of the same K in one launch.
constexpr int GEMV_MULTI_MAX = 4;
hipError_t gemv_q4_0_multi(int nmat, const void *const *W, const int64_t *M, int64_t K, const float *x, int64_t N,
                           float *const *y, const int64_t *ldy, const DeviceInfo &dev, hipStream_t s);

// The same for N = 1 with the chain that produces x folded into the x prologue, at the widths
// gemv_norm_supported(kind, K) accepts (K % 64 == 0; kind 1: K <= 8192, one round of 16 x-waves with the
// default GEMV_XPRO_N holds the row; kind 2: K <= 12288, the row-item forms of at most 3 pairs per lane); the
// GEMVs consume x, and workgroup 0 also stores the chain's tensors (each may be null) bit for bit as
// the unfused launches:
//   kind 1, ggml's [add ->] rms_norm -> mul(norm weight row): x = (a ? a + b : b) -> sum,
//           x *= 1/sqrt(mean(x*x) + 1e-6) (double sum, as ggml_ops.hip's k_row_norm4) -> norm,
//           x *= w -> out;
//   kind 2, silu -> mul: u = fp16 table[fp16(a)] (ggml's GGML_SILU_FP16) -> norm, x = u * b -> out.
struct GemvNorm {
    const float *a, *w;
    float *sum, *norm, *out;
    int kind = 1;
    const uint16_t *table = nullptr;     // kind 2: ggml's silu table (65536 fp16 bit patterns)
};
// Decode epilogue of a sibling GEMV (hook path, one token): the elementwise nodes ggml emits right after the
// q|k|v mul_mats (rope mode 0 of K and Q in place, K into the K cache, V into the transposed V cache) done by
// the GEMV on its own output element e of matrix i, with the arithmetic of k_elem_batch (ggml_ops.hip) bit
// for bit.  kind 0: y[e] = v; 1: d[e] = rope(v, partner e ^ 1) with (cos, sin) cs[(e % ne0) / 2] (and
// y[e] = v unless d is y), then the copy of d[e]; 2: y[e] = v, then the copy of v.  The copy writes
// linear element e of its target view (ne10, ne11, strides in bytes) as F16 or F32 when c != nullptr.
//   glu != 0 instead (two matrices of M rows, gate then up, launched as 2M interleaved rows): the silu -> mul
// that follows w1 | w3, d[0][e] = silu(gate[e]) and d[1][e] = d[0][e] * up[e] as k_silu_mul computes them
// (table: table_silu_f16 as the kernels take it), beside the two outputs
struct GemvEpi {
    int glu;
    const uint16_t *table;
    float *d[GEMV_MULTI_MAX];
    const float2 *cs[GEMV_MULTI_MAX];
    char *c[GEMV_MULTI_MAX];
    int kind[GEMV_MULTI_MAX], f16[GEMV_MULTI_MAX], ne0[GEMV_MULTI_MAX];
    int ne10[GEMV_MULTI_MAX], ne11[GEMV_MULTI_MAX], nb10[GEMV_MULTI_MAX], nb11[GEMV_MULTI_MAX], nb12[GEMV_MULTI_MAX];
};
// the kinds and widths gemv_q4_0_multi_norm launches (everything else: hipErrorInvalidValue, nothing launched);
// the hook scheduler holds a chain for the prologue only where this is true
bool gemv_norm_supported(int kind, int64_t K);
// epi: nullptr, or the epilogue of every matrix (strided row mapping; returns hipErrorInvalidValue where the
// launch shape cannot pair rows e and e ^ 1 inside one workgroup)
hipError_t gemv_q4_0_multi_norm(int nmat, const void *const *W, const int64_t *M, int64_t K, const float *b,
                                const GemvNorm &nrm, float *const *y, const int64_t *ldy, const DeviceInfo &dev,
                                hipStream_t s, const GemvEpi *epi = nullptr);

// test hook: force the GEMV launch policy (row mapping 0/1/2, ring depth 1/2, row items 0/1,
// workgroups per CU); -1 / 0 = automatic
void gemv_set_policy(int map, int depth, int rowitems, int wg_per_cu);
void gemv_set_bal(int bal);   // -1 auto, 0 off, 1 every chunked decode launch (K > 12288)


// Prefill path: int8 MFMA (v_mfma_i32_32x32x32_i8, K=32 = one q4_0 block) GEMM on the
// pre-quantized activations xs (quantize_q8_0_soa).
// xd16: the same d_x as fp16 bits, block-major [K/32][N] (quantize_q8_0_soa's d16 copy; the default
// LDS GEMM DMAs it straight into its operand layout)
hipError_t gemm_q4_0(const void *W, int64_t K, int64_t M, const int8_t *xqs, const float *xd,
                     int64_t N, float *y, int64_t ldy, hipStream_t s, const uint16_t *xd16);

// Prefill GEMM v8 (default for the LDS GEMM path): x as a block-major int8 image + fp16 d_x
// (gemm8_prep_x, bit-exact q8_0 values), the q4_0 weights converted per call into an int8 image
// (w = nibble - 8, fp16 d verbatim) in the workspace wws, then the MFMA GEMM over both images.
int64_t gemm8_np(int64_t N);
size_t gemm8_x_bytes(int64_t K, int64_t N);       // x image + d_x
size_t gemm8_w_bytes(int64_t K, int64_t M);       // weight image + d_w
hipError_t gemm8_prep_x(const float *x, int64_t K, int64_t N, void *xws, hipStream_t s);
hipError_t gemm8_prep_w(const void *W, int64_t K, int64_t M, void *wws, hipStream_t s);
hipError_t gemm8_run(const void *wws, int64_t K, int64_t M, const void *xws, int64_t N, float *y, int64_t ldy,
                     hipStream_t s);
// Prefill GEMM v9: the same block sums on the block-scaled fp6 MFMA (e2m3 images: weights w/2,
// x split into (q >> 4)/2 and (q & 15)/2; 26 B per 32 weights, 50 B per 32 activations), bitwise
// equal to v8.
int64_t gemm9_np(int64_t N);
size_t gemm9_x_bytes(int64_t K, int64_t N);
size_t gemm9_w_bytes(int64_t K, int64_t M);
hipError_t gemm9_prep_x(const float *x, int64_t K, int64_t N, void *xws, hipStream_t s);
hipError_t gemm9_prep_w(const void *W, int64_t K, int64_t M, void *wws, hipStream_t s);
// one launch over the row tiles of n (1..4) sibling weight images that share the x image; xo (optional, per
// matrix, null entries allowed): the epilogue also writes matrix i's y as the x image of a next launch (K = M[i],
// same N; bitwise gemm9_prep_x of y; gemm9_xo_ok(M[i], N), ldy[i] == M[i], gemm9_x_bytes(M[i], N) bytes)
bool gemm9_xo_ok(int64_t M, int64_t N);
hipError_t gemm9_run_multi(int n, const void *const *wws, const int64_t *M, int64_t K, const void *xws, int64_t N,
                           float *const *y, const int64_t *ldy, hipStream_t s, uint8_t *const *xo = nullptr);
hipError_t gemm9_run(const void *wws, int64_t K, int64_t M, const void *xws, int64_t N, float *y, int64_t ldy,
                     hipStream_t s);
// the 128 x 128 tile (k_gemm9w): -1 auto by rounds of CUs (GGML_HIP_GEMM9_WIDE overrides), 0 never, 1 always
void gemm9_set_wide(int mode);

// Small / medium N (split-K over the waves of a 32x32-tile workgroup, operands straight to registers).
hipError_t gemm_sk_q4_0(const void *W, int64_t K, int64_t M, const int8_t *xqs, const float *xd, int64_t N,
                        float *y, int64_t ldy, int num_cus, hipStream_t s);

// Exact mode: y bit-identical to the reference's AVX2+FMA ggml_vec_dot_q4_0_q8_0 (ggml.c:2412-2435),
// per-lane sequential fma chains in block order; any N.
hipError_t mm_exact_q4_0(const void *W, int64_t K, int64_t M, const int8_t *xqs, const float *xd, int64_t N,
                         float *y, int64_t ldy, hipStream_t s);
// the same for up to 4 matrices of the same K sharing x, one launch (sibling groups in exact mode)
hipError_t mm_exact_q4_0_multi(int n, const void *const *W, const int64_t *M, int64_t K, const int8_t *xqs,
                               const float *xd, int64_t N, float *const *y, const int64_t *ldy, hipStream_t s);

// Q6_K (q6_k.hip): the output.weight of a k-quants q4_0 model.  W: ggml block_q6_K rows, verbatim
// (210 bytes per 256 weights, rows only 2-byte aligned); xq8k: ggml block_q8_K rows (292 bytes per 256).
constexpr int QK_K = 256;     // k-quants superblock
constexpr int Q6KB = 210;     // sizeof(block_q6_K)
constexpr int Q8KB = 292;     // sizeof(block_q8_K)
// quantize_row_q8_K_reference / dequantize_row_q6_K, bit-exact
hipError_t quantize_q8_K(const float *x, int64_t K, int64_t N, void *xq8k, hipStream_t s);
hipError_t dequantize_q6_K(const void *wq, int64_t K, int64_t M, float *w, hipStream_t s);
// fused q8_K quantize of x (LDS) + q6_K.q8_K GEMV; K % 256 == 0, K <= 16384; N > 8 runs column tiles of 8
hipError_t gemv_q6_K(const void *W, int64_t K, int64_t M, const float *x, int64_t N, float *y, int64_t ldy,
                     const DeviceInfo &dev, hipStream_t s);
// exact mode: y bit-identical to the AVX2 ggml_vec_dot_q6_K_q8_K on the pre-quantized xq8k; any N
hipError_t mm_exact_q6_K(const void *W, int64_t K, int64_t M, const void *xq8k, int64_t N, float *y, int64_t ldy,
                         hipStream_t s);
// Q8_0 weights (blk32_w.hip): the layer matrices of a "mostly Q8_0" file.  W: ggml block_q8_0 rows, verbatim
// (34 bytes per 32 weights, rows 4-byte aligned: K % 64 == 0).
hipError_t dequantize_q8_0(const void *wq, int64_t K, int64_t M, float *w, hipStream_t s);
// fused q8_0 quantize of x (LDS) + q8_0.q8_0 GEMV; N > gemv_q8_0w_max_tokens(K) runs column tiles (a column's y
// does not depend on its tile); max_tokens is 8 up to K = 7232 and 0 where one token's q8_0 exceeds the LDS
int gemv_q8_0w_max_tokens(int64_t K);
hipError_t gemv_q8_0w(const void *W, int64_t K, int64_t M, const float *x, int64_t N, float *y, int64_t ldy,
                      const DeviceInfo &dev, hipStream_t s);
// test hook: force the launch policy (row mapping -1 auto / 0 / 1 / 2, ring depth 0 auto / 1 / 2, workgroups per CU)
void gemv_q8_0w_set_policy(int map, int depth, int wg_per_cu);
// exact mode: y bit-identical to the AVX2 ggml_vec_dot_q8_0_q8_0 on the SoA q8_0 of x (quantize_q8_0_soa); any N
hipError_t mm_exact_q8_0w(const void *W, int64_t K, int64_t M, const int8_t *xqs, const float *xd, int64_t N, float *y,
                          int64_t ldy, hipStream_t s);
// prefill: the k_gemm8 weight image (gemm8_w_bytes(K, M) bytes) from Q8_0 rows; then gemm8_prep_x + gemm8_run
hipError_t gemm8_prep_w_q8_0(const void *W, int64_t K, int64_t M, void *wws, hipStream_t s);

// Q5_K / Q4_K (q45_k.hip): the layer matrices of a "mostly Q5_K" / "mostly Q4_K" file.  W: ggml block_q5_K
// (176 bytes per 256 weights) or block_q4_K (144 bytes) rows, verbatim, 16-byte aligned; qh: true Q5_K, false Q4_K.
constexpr int Q5KB = 176;     // sizeof(block_q5_K)
constexpr int Q4KB = 144;     // sizeof(block_q4_K)
// dequantize_row_q5_K / dequantize_row_q4_K, bit-exact
hipError_t dequantize_q45_K(bool qh, const void *wq, int64_t K, int64_t M, float *w, hipStream_t s);
// fused q8_K quantize of x (LDS) + q.q8_K GEMV; K % 256 == 0, K <= 16384; N > 8 runs column tiles of 8
hipError_t gemv_q45_K(bool qh, const void *W, int64_t K, int64_t M, const float *x, int64_t N, float *y, int64_t ldy,
                      const DeviceInfo &dev, hipStream_t s);
// exact mode: y bit-identical to the AVX2 ggml_vec_dot_q5_K_q8_K / _q4_K_q8_K on the pre-quantized xq8k; any N
hipError_t mm_exact_q45_K(bool qh, const void *W, int64_t K, int64_t M, const void *xq8k, int64_t N, float *y,
                          int64_t ldy, hipStream_t s);
// Q3_K / Q2_K (q23_k.hip): the layer matrices of a "mostly Q3_K" / "mostly Q2_K" file.  W: ggml block_q3_K (110 bytes
// per 256 weights) or block_q2_K (84 bytes) rows, verbatim, the matrix 4-byte aligned (a Q3_K block is then only
// 2-byte aligned; no byte outside the matrix is read); q3: true Q3_K, false Q2_K.
constexpr int Q3KB = 110;     // sizeof(block_q3_K)
constexpr int Q2KB = 84;      // sizeof(block_q2_K)
// dequantize_row_q3_K / dequantize_row_q2_K, bit-exact
hipError_t dequantize_q23_K(bool q3, const void *wq, int64_t K, int64_t M, float *w, hipStream_t s);
// fused q8_K quantize of x (LDS) + q.q8_K GEMV; K % 256 == 0, K <= 16384; N > 8 runs column tiles of 8
hipError_t gemv_q23_K(bool q3, const void *W, int64_t K, int64_t M, const float *x, int64_t N, float *y, int64_t ldy,
                      const DeviceInfo &dev, hipStream_t s);
// exact mode: y bit-identical to the AVX2 ggml_vec_dot_q3_K_q8_K / _q2_K_q8_K on the pre-quantized xq8k; any N
hipError_t mm_exact_q23_K(bool q3, const void *W, int64_t K, int64_t M, const void *xq8k, int64_t N, float *y,
                          int64_t ldy, hipStream_t s);

// prefill of the five k-quants (q6_k_gemm.hip, q45_k_gemm.hip, q23_k_gemm.hip; what they share is kquant_gemm.h).
// The q8_K values of x as planes: qs int8 [N][K] (16-byte aligned) + d f32 [N][K / 256], and where dig is not null
// (Q5_K / Q4_K) dig int8 [N][K / 256][16], 16-byte aligned: the low then the high base-128 digits of the eight per-32
// sums.  The int8-MFMA GEMMs on them, the blocks read in place, y bitwise the type's GEMV's; any K % 256 == 0
// (N K < 2^31), M, N >= 1.
hipError_t quantize_q8_K_planes(const float *x, int64_t K, int64_t N, void *qs, float *xd, void *dig, hipStream_t s);
hipError_t gemm_q6_K(const void *W, int64_t K, int64_t M, const void *xqs, const float *xd, int64_t N, float *y,
                     int64_t ldy, const DeviceInfo &dev, hipStream_t s);
hipError_t gemm_q45_K(bool qh, const void *W, int64_t K, int64_t M, const void *xqs, const float *xd, const void *xdig,
                      int64_t N, float *y, int64_t ldy, const DeviceInfo &dev, hipStream_t s);
hipError_t gemm_q23_K(bool q3, const void *W, int64_t K, int64_t M, const void *xqs, const float *xd, int64_t N, float *y,
                      int64_t ldy, const DeviceInfo &dev, hipStream_t s);

// Q4_1 / Q5_0 / Q5_1 weights (blk32_w.hip): the layer matrices of a "mostly Q4_1 / Q5_0 / Q5_1" file.  W: ggml
// block_q4_1 (20 bytes per 32 weights), block_q5_0 (22) or block_q5_1 (24) rows, verbatim, 4-byte aligned (K % 64
// == 0); qh: the type has a fifth bit plane (Q5_0, Q5_1), mn: a minimum and q8_1 activations (Q4_1, Q5_1).
// dequantize_row_q4_1 / _q5_0 / _q5_1, bit-exact
hipError_t dequantize_q5x(bool qh, bool mn, const void *wq, int64_t K, int64_t M, float *w, hipStream_t s);
// quantize_row_q8_1 (AVX2 branch), bit-exact: block_q8_1 rows (40 bytes per 32 elements), or the planes qs int8
// [N][K], d f32 [N][K / 32], s f32 [N][K / 32]
hipError_t quantize_q8_1_aos(const float *x, int64_t K, int64_t N, void *xq, hipStream_t s);
hipError_t quantize_q8_1_soa(const float *x, int64_t K, int64_t N, int8_t *qs, float *d, float *sx, hipStream_t s);
// fused quantize of x (LDS, 40 bytes per block and token) + GEMV; N > gemv_q5x_max_tokens(K) runs column tiles (a
// column's y does not depend on its tile); max_tokens is 8 up to K = 6528 and 0 where one token exceeds the LDS
int gemv_q5x_max_tokens(int64_t K);
hipError_t gemv_q5x(bool qh, bool mn, const void *W, int64_t K, int64_t M, const float *x, int64_t N, float *y,
                    int64_t ldy, const DeviceInfo &dev, hipStream_t s);
// test hook: force the launch policy (row mapping -1 auto / 0 / 1 / 2, ring depth 0 auto / 1 / 2, workgroups per CU)
void gemv_q5x_set_policy(int map, int depth, int wg_per_cu);
// exact mode: y bit-identical to the type's AVX2 ggml_vec_dot on the planes of x: quantize_q8_0_soa's qs and d for
// Q5_0 (xsum unused), quantize_q8_1_soa's for the other two; any N, no K limit
hipError_t mm_exact_q5x(bool qh, bool mn, const void *W, int64_t K, int64_t M, const int8_t *xqs, const float *xd,
                        const float *xsum, int64_t N, float *y, int64_t ldy, hipStream_t s);
// Q5_0 prefill: the k_gemm8 weight image (gemm8_w_bytes(K, M) bytes) of q - 16; then gemm8_prep_x + gemm8_run
hipError_t gemm8_prep_w_q5_0(const void *W, int64_t K, int64_t M, void *wws, hipStream_t s);
// Q4_1 / Q5_1 prefill (q5x_gemm.hip): the int8-MFMA GEMM on the weights in place and quantize_q8_1_soa's planes of x
// (qs 16-byte, d and sx 8-byte aligned); one fp32 chain per output, block by block (y within the parity bound of
// gemv_q5x's, not bitwise it); any K % 64 == 0 (N K < 2^31), M, N >= 1
hipError_t gemm_q5x1(bool qh, const void *W, int64_t K, int64_t M, const int8_t *xqs, const float *xd, const float *xsum,
                     int64_t N, float *y, int64_t ldy, const DeviceInfo &dev, hipStream_t s);

// ---- F16 weights (f16_w.hip): y[n * ldy + m] = sum_e W[m][e] * fp16(x[n][e]), W contiguous F16 rows (16-byte
// aligned, K % 32 == 0), one fixed fp32 order per K (tests/f16w_ref.py).  N > gemv_f16w_max_tokens(K) runs column tiles
// (a column's y does not depend on its tile); max_tokens is 8 up to K = 8192, 5 at K = 11008 and 0 where one token's
// fp16 image exceeds the LDS (K > 65536)
int gemv_f16w_max_tokens(int64_t K);
hipError_t gemv_f16w(const void *W, int64_t K, int64_t M, const float *x, int64_t N, float *y, int64_t ldy,
                     const DeviceInfo &dev, hipStream_t s);
// prefill (f16_w_gemm.hip): the f16-MFMA GEMM decomposed for weight shapes, any K % 32 == 0 (N K < 2^31), M, N >= 1,
// ldy >= M; y within the fp32-accumulation bound, its order a function of K and the plan alone.  A plan (1 ..
// F16W_WGEMM_PLANS) is a pure function of (K, M, N, CU count; 256 CUs where num_cus <= 0) unless one is pinned
// (set_plan: 0 auto, returns the previous).  ws: ws_bytes(K, M, N, num_cus) bytes for the fp16 image of x and the
// plan's K-slice slabs.  supported: the index products and every plan's grid fit one launch.
constexpr int F16W_WGEMM_PLANS = 3;
int gemm_f16w_plan(int64_t K, int64_t M, int64_t N, int num_cus);        // the pinned plan, or auto's
int gemm_f16w_auto_plan(int64_t K, int64_t M, int64_t N, int num_cus);
int gemm_f16w_set_plan(int plan);
bool gemm_f16w_supported(int64_t K, int64_t M, int64_t N);
size_t gemm_f16w_ws_bytes(int64_t K, int64_t M, int64_t N, int num_cus);
hipError_t gemm_f16w(const void *W, int64_t K, int64_t M, const float *x, int64_t N, float *y, int64_t ldy, void *ws,
                     size_t ws_bytes, const DeviceInfo &dev, hipStream_t s);

// ---- F32 weights (f32_w.hip): y[n * ldy + m] = sum_e W[m][e] * x[n][e], W contiguous F32 rows (16-byte aligned,
// K % 32 == 0), fmaf on the unrounded operands, one fixed order per K (tests/f32w_ref.py gemv_schedule).  N >
// gemv_f32w_max_tokens(K) runs column tiles (a column's y does not depend on its tile); max_tokens is 8 up to K = 4096,
// 2 at K = 11008 and 0 where one column's floats exceed the LDS (K > 32768).  mm_exact: ggml_vec_dot_f32's AVX2
// schedule bit for bit, any N, ldy >= M.
int gemv_f32w_max_tokens(int64_t K);
hipError_t gemv_f32w(const void *W, int64_t K, int64_t M, const float *x, int64_t N, float *y, int64_t ldy,
                     const DeviceInfo &dev, hipStream_t s);
hipError_t mm_exact_f32w(const void *W, int64_t K, int64_t M, const float *x, int64_t N, float *y, int64_t ldy,
                         hipStream_t s);
// prefill (f32_w_gemm.hip): the f32-MFMA GEMM, any K % 32 == 0 (N K < 2^31), M, N >= 1, ldy >= M; y is one fmaf chain
// per K slice in natural order and the slices added in order, a function of K and the split S alone.  S (1, 2, 4) is a
// pure function of (K, M, N, CU count; 256 CUs where num_cus <= 0) unless one is pinned (set_ksplit: 0 auto, returns
// the previous); a pinned S that leaves no whole 32-element chunks per slice runs as the next smaller one (ksplit
// returns what runs).  ws: ws_bytes(K, M, N, num_cus) bytes for the slabs.
int gemm_f32w_ksplit(int64_t K, int64_t M, int64_t N, int num_cus);      // the pinned split, or auto's
int gemm_f32w_auto_ksplit(int64_t K, int64_t M, int64_t N, int num_cus);
int gemm_f32w_set_ksplit(int s);
bool gemm_f32w_supported(int64_t K, int64_t M, int64_t N);
size_t gemm_f32w_ws_bytes(int64_t K, int64_t M, int64_t N, int num_cus);
hipError_t gemm_f32w(const void *W, int64_t K, int64_t M, const float *x, int64_t N, float *y, int64_t ldy, void *ws,
                     size_t ws_bytes, const DeviceInfo &dev, hipStream_t s);

// Multi-GPU helper: y[n*ldy + row0[r] + i] = slab[r][n][i] for i < rows[r] (gather compaction).
// row_begin travels as a kernel argument (no host->device copy, capture-safe)
static constexpr int SCATTER_MAX_RANKS = 256;
struct RowBegins {
    int64_t v[SCATTER_MAX_RANKS + 1];
};
hipError_t scatter_slabs(const float *slabs, int nranks, int64_t max_rows, const RowBegins &row_begin,
                         int64_t N, float *y, int64_t ldy, hipStream_t s);

// Direct-store all-gather over xGMI (p2p_gather.hip): land[r] = rank r's landing buffer as mapped in
// this process ([2 slots][R][cap] floats), flag[r] = its R flag words, ctl = this rank's control block
// (epoch, arrivals, error bits).
constexpr int P2P_MAX_RANKS = 8;
struct P2PArgs {
    float *land[P2P_MAX_RANKS];
    uint64_t *flag[P2P_MAX_RANKS];
    uint64_t *ctl;                   // [0] epoch, [1] arrivals, [2] error bits (peer q timed out: bit q),
                                     // [3] failure notices from peers (peer p failed: bit p, stored by p)
    uint64_t *pctl[P2P_MAX_RANKS];   // every rank's control block (ctl of rank r, mapped here)
    uint32_t *herr;                  // host-mapped words, or nullptr: [0] error (nonzero: the comm failed),
                                     // [1] abort request (set by the host in ggml_hip_comm_abort; polled by
                                     // this rank's own waits, so an in-flight gather ends at its next poll)
    uint64_t timeout;                // peer-wait bound in s_memrealtime ticks (100 MHz)
    int me, R;
    int64_t cap;
};
hipError_t p2p_allgather(const P2PArgs &a, const float *send, int64_t count, float *recv, hipStream_t s);
// fail this rank's comm and notify every peer (bit me in each peer's ctl[3]); stream-ordered on s (the host
// sets herr[1] first, so a gather of this rank blocked ahead of it on s ends and sends the notice itself)
hipError_t p2p_abort(const P2PArgs &a, hipStream_t s);

// Synthetic inputs for the bench (splitmix64 + Box-Muller on device).
hipError_t fill_gaussian(float *dst, int64_t n, uint64_t seed, float mean, float std, hipStream_t s);

}  // namespace ghip
