/*
 * ggml-hip.h — C ABI of the MI355X-native (gfx950) q4_0 mul_mat backend for ggml.
 *
 * Drop-in for the reference's GPU backend ABI, ggml-cuda.h:15-36 of
 * Fcucgvhhhvjv/llama.cpp-q_4_0 (the hook sites in ggml.c / llama.cpp /
 * arch/arch-util.h call these exactly where they call ggml_cuda_*; see
 * INTEGRATION.md).  Plain pointers and sizes only; no torch types.
 *
 * Scope: GGML_OP_MUL_MAT with src0 = GGML_TYPE_Q4_0, src1 = dst = GGML_TYPE_F32
 * (the path BASELINE.json names), and the same with src0 = GGML_TYPE_Q6_K: the
 * output.weight a k-quants build's quantizer writes into every q4_0 file
 * (llama.cpp:2416-2421; ggml_vec_dot_q6_K_q8_K semantics, k_quants.c), and with
 * src0 = GGML_TYPE_Q8_0: the matrices of a "mostly Q8_0" file
 * (ggml_vec_dot_q8_0_q8_0 semantics), and with src0 = GGML_TYPE_Q5_K: the layer
 * matrices of a "mostly Q5_K" file (ggml_vec_dot_q5_K_q8_K semantics), and with
 * src0 = GGML_TYPE_Q3_K / GGML_TYPE_Q2_K: the layer matrices of the "mostly
 * Q3_K" and "mostly Q2_K" files (ggml_vec_dot_q3_K_q8_K / _q2_K_q8_K semantics),
 * and with src0 = GGML_TYPE_Q4_1 / Q5_0 / Q5_1, and with src0 = a 2-D
 * GGML_TYPE_F16 leaf: the matrices of a "mostly F16" file
 * (ggml_compute_forward_mul_mat_f16_f32 semantics), and with src0 = a 2-D
 * GGML_TYPE_F32 leaf with K % 32 == 0: the matrices of an "all F32" file
 * (ggml_compute_forward_mul_mat_f32 semantics) once an operand is on the
 * device; an all-host F32 node only with GGML_HIP_F32_W=1 /
 * ggml_hip_debug_set_f32_w(1) (off by default).
 * src0 = GGML_TYPE_Q4_K (a "mostly Q4_K" file) is taken on this hook path only
 * with GGML_HIP_Q4_K=1 / ggml_hip_debug_set_q4_K(1) (off by default);
 * the tensor-free ggml_hip_mul_mat_q4_K always runs.  Everything
 * else (Q4_K with its switch off and every operand on the host included;
 * between device operands it is served from the host copy, since ggml's CPU
 * op cannot run there) returns "cannot" so ggml's CPU path runs, exactly as ggml_cuda_can_mul_mat / ggml_cuda_compute_forward
 * return false for what they do not handle.
 *
 * Numerics (pinned by tests/): the q8_0 activation bytes are bit-exact to the
 * AVX2 branch of quantize_row_q8_0 (ggml.c:1192-1275); y agrees with
 * ggml_vec_dot_q4_0_q8_0 within 1e-3 relative + fp32 accumulation bound.
 */
#ifndef GGML_HIP_H
#define GGML_HIP_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GGML_HIP_MAX_DEVICES 16   /* GGML_CUDA_MAX_DEVICES, ggml-cuda.h:9 */

struct ggml_tensor;              /* ggml.h:378-414 (mirrored bit-for-bit in csrc/ggml_abi.h) */
struct ggml_compute_params;      /* ggml.h:459-468 */

/* tensor->extra of device-resident tensors (ggml-cuda.h:11-13): one pointer per
 * device; for GGML_BACKEND_GPU_SPLIT tensors device i holds its row slice. */
struct ggml_tensor_extra_gpu {
    void *data_device[GGML_HIP_MAX_DEVICES];
};

/* status codes of the tensor-free entry points */
enum ggml_hip_status {
    GGML_HIP_OK = 0,
    GGML_HIP_ERR_INVALID = -1,      /* bad shape / pointer / alignment */
    GGML_HIP_ERR_UNSUPPORTED = -2,  /* valid request outside the q4_0 path */
    GGML_HIP_ERR_DEVICE = -3,       /* HIP runtime error (message on stderr) */
    GGML_HIP_ERR_NOMEM = -4,
    GGML_HIP_ERR_COMM = -5,         /* RCCL error */
};

/* ------------------------------------------------------------------------------------------
 * ggml-cuda.h equivalents (same argument meaning, same error behaviour: HIP errors are
 * fatal with a message, like CUDA_CHECK in ggml-cuda.cu:22-51).
 * ---------------------------------------------------------------------------------------- */

/* ggml_init_cublas (ggml-cuda.h:15, ggml-cuda.cu:1826-1861): enumerate devices, default
 * split proportional to VRAM, one non-blocking stream per device.  Idempotent, thread-safe. */
void   ggml_init_hip(void);
/* ggml_cuda_set_tensor_split (ggml-cuda.h:16): per-device fractions (cumulative sums are
 * normalised, all-zero = keep default). */
void   ggml_hip_set_tensor_split(const float *tensor_split);
/* ggml_cuda_can_mul_mat (ggml-cuda.h:19, ggml-cuda.cu:2595-2610). */
bool   ggml_hip_can_mul_mat(const struct ggml_tensor *src0, const struct ggml_tensor *src1,
                            struct ggml_tensor *dst);
/* ggml-cuda.h:20 declares ggml_cuda_mul_mat_get_wsize but ggml-cuda.cu never defines it; ours
 * returns 0 (no host work buffer is needed). */
size_t ggml_hip_mul_mat_get_wsize(const struct ggml_tensor *src0, const struct ggml_tensor *src1,
                                  struct ggml_tensor *dst);
/* ggml_cuda_mul_mat (ggml-cuda.h:21 / ggml-cuda.cu:2671): dst = src0 x src1 for Q4_0 src0.
 * Operands may be host (GGML_BACKEND_CPU) or device resident; synchronous on return when dst
 * is a host tensor. */
void   ggml_hip_mul_mat(const struct ggml_tensor *src0, const struct ggml_tensor *src1,
                        struct ggml_tensor *dst);
/* ggml_cuda_mul (ggml-cuda.h:18, ggml-cuda.cu:2580-2583): dst = src0 * src1 (F32, src1 rows
 * repeated over src0), on the device, operands host or device resident. */
void   ggml_hip_mul(const struct ggml_tensor *src0, const struct ggml_tensor *src1, struct ggml_tensor *dst);
/* ggml_cuda_host_malloc / host_free (ggml-cuda.h:24-25): pinned host memory, NULL on failure. */
void  *ggml_hip_host_malloc(size_t size);
void   ggml_hip_host_free(void *ptr);
/* ggml_cuda_transform_tensor (ggml-cuda.h:27, ggml-cuda.cu:2766-2809): upload tensor data
 * (whole, or the device's row slice for GGML_BACKEND_GPU_SPLIT) and set tensor->extra. */
void   ggml_hip_transform_tensor(void *data, struct ggml_tensor *tensor);
/* ggml_cuda_free_data (ggml-cuda.h:29). */
void   ggml_hip_free_data(struct ggml_tensor *tensor);
/* ggml_cuda_assign_buffers{,_no_scratch,_force_inplace} (ggml-cuda.h:30-32): give a
 * graph tensor device storage (scratch ring unless no_scratch). */
void   ggml_hip_assign_buffers(struct ggml_tensor *tensor);
void   ggml_hip_assign_buffers_no_scratch(struct ggml_tensor *tensor);
void   ggml_hip_assign_buffers_force_inplace(struct ggml_tensor *tensor);
/* ggml_cuda_set_main_device / set_scratch_size / free_scratch (ggml-cuda.h:33-35). */
void   ggml_hip_set_main_device(int main_device);
void   ggml_hip_set_scratch_size(size_t scratch_size);
void   ggml_hip_free_scratch(void);
/* ggml_cuda_compute_forward (ggml-cuda.h:36, ggml-cuda.cu:2933-3021): returns true when the
 * node was taken by the backend (the CPU op is then skipped, ggml.c:15645-15652).  Only thread
 * ith == 0 in the COMPUTE phase launches; the other threads/phases return true immediately. */
bool   ggml_hip_compute_forward(struct ggml_compute_params *params, struct ggml_tensor *tensor);
/* ggml_cpu_has_cublas (ggml.c:19465-19470) equivalent: 1 when a HIP device is usable. */
int    ggml_cpu_has_hipblas(void);

/* Device weight-residency cache.  A CPU-backend Q4_0 src0 (the arch/
 * frontends never call transform_tensor; the reference re-uploads it every call,
 * ggml-cuda.cu:2496-2502) is uploaded once per device and reused while a sampled fingerprint of
 * its bytes is unchanged; LRU under GGML_HIP_WEIGHT_CACHE_MB (default 65536), off with
 * GGML_HIP_WEIGHT_CACHE=0.  Counters since the last clear; clear frees every cached copy. */
int    ggml_hip_weight_cache_stats(int64_t *hits, int64_t *misses, int64_t *resident_bytes);
int    ggml_hip_weight_cache_clear(void);
/* Host writes into cached weights.  Writes made by ggml nodes (the reference's LoRA apply rewrites
 * Q4_0 weights in place through ggml_add_inplace / ggml_cpy graphs, llama.cpp:2950-2967) are seen
 * by ggml_hip_compute_forward's INIT phase and invalidate the overlapping copies exactly.  A host
 * that edits weight bytes outside ggml calls ggml_hip_weight_cache_invalidate(ptr, bytes) (drops
 * every copy overlapping [ptr, ptr+bytes), bytes 0 = the copies containing ptr; returns how many,
 * or a negative status), or runs with GGML_HIP_WEIGHT_CACHE_VERIFY=full / set_verify(1): every
 * lookup then fingerprints every byte of the host weight (exact; one host read per call; -1 =
 * environment, 0 = sampled fingerprint). */
int64_t ggml_hip_weight_cache_invalidate(const void *host, size_t bytes);
int    ggml_hip_weight_cache_set_verify(int mode);
int64_t ggml_hip_weight_cache_invalidations(void);

/* ------------------------------------------------------------------------------------------
 * Tensor-free entry points (device pointers, stream-ordered on `stream` = hipStream_t or NULL
 * for the backend's stream on the current device).  Return enum ggml_hip_status.
 * Layouts: ggml's.  W = block_q4_0 rows (18*K/32 bytes per row), x = f32 [N][K] row-major,
 * y = f32 [N][M] row-major (y[n*M + m], i.e. ggml dst with ne0 = M, ne1 = N).
 * Pointers must be 16-byte aligned; K % 64 == 0 (ggml.c:2344 asserts nb % 2 == 0).
 * ---------------------------------------------------------------------------------------- */

/* q8_0 quantize of N activation rows, ggml block_q8_0 output (34*K/32 bytes per row);
 * bit-exact to quantize_row_q8_0's AVX2 branch (ggml.c:1192-1275). */
int ggml_hip_quantize_q8_0(const float *dev_x, int64_t K, int64_t N, void *dev_xq, void *stream);
/* q4_0 weight quantizer, bit-exact to quantize_row_q4_0_reference (ggml.c:918-953). */
int ggml_hip_quantize_q4_0(const float *dev_w, int64_t K, int64_t M, void *dev_wq, void *stream);
/* dequantize_row_q4_0 (ggml.c:1500-1518). */
int ggml_hip_dequantize_q4_0(const void *dev_wq, int64_t K, int64_t M, float *dev_w, void *stream);

/* y = W x (ggml_compute_forward_mul_mat_q_f32, ggml.c:11226-11424, INIT + COMPUTE fused):
 * N <= 8: fused quantize + GEMV (one wave64 per weight row); N > 8: q8_0 quantize + int8-MFMA
 * GEMM.  Uses the backend's device workspace for N > 8 (grown outside stream capture by
 * ggml_hip_reserve_workspace or the first call). */
int ggml_hip_mul_mat_q4_0(const void *dev_w, int64_t K, int64_t M, const float *dev_x, int64_t N,
                          float *dev_y, void *stream);
/* Same with an explicit algorithm and output stride ldy: 0 auto (4 in exact mode; else 1 for N <= 8,
 * 3 for N <= 128, else 2), 1 fused GEMV (N <= 8), 2 LDS-staged int8-MFMA GEMM, 3 split-K int8-MFMA
 * GEMM (small N), 4 exact: every y bit-identical to the reference's x86 AVX2+FMA
 * ggml_vec_dot_q4_0_q8_0 (ggml.c:2412-2435; same q8_0 bytes, same fp32 fma schedule). */
int ggml_hip_mul_mat_q4_0_ex(const void *dev_w, int64_t K, int64_t M, const float *dev_x, int64_t N,
                             float *dev_y, int64_t ldy, int algo, void *stream);
/* Q6_K weights (block_q6_K rows, 210 bytes per 256 weights, 2-byte aligned) x F32 -> F32 with the semantics of
 * the reference's CPU path (k_quants.c, QK_K = 256).  Stream-ordered and graph-capturable: no allocation in a
 * call once the workspace is reserved (ggml_hip_reserve_workspace(K, N) covers the exact mode's q8_K of x and the
 * prefill GEMM's q8_K planes).
 * Status codes as for the q4_0 entry points; K % 256 != 0 -> GGML_HIP_ERR_INVALID.
 * The kernels read the Q6_K rows as naturally aligned 32-bit words, so up to 2 bytes below dev_w (when it sits at
 * 2 mod 4) and up to 2 bytes past the last row (when it ends at 2 mod 4) are read and ignored: the matrix must lie
 * in an allocation whose first and last aligned 4-byte words are readable (any hipMalloc'ed buffer).
 * quantize_q8_K: N rows of K f32 -> block_q8_K (292 bytes per 256), bit-exact to quantize_row_q8_K_reference
 * (k_quants.c:1133-1168); bsums of an all-zero block are written as zeros (the reference leaves them unwritten). */
int ggml_hip_quantize_q8_K(const float *dev_x, int64_t K, int64_t N, void *dev_xq, void *stream);
/* dequantize_row_q6_K (k_quants.c:1065-1110), bit-exact. */
int ggml_hip_dequantize_q6_K(const void *dev_wq, int64_t K, int64_t M, float *dev_w, void *stream);
/* y[n*ldy + m] = W[m] . x[n].  algo: 0 auto (4 in exact mode; else 5 when N >= the GEMM threshold or K > 16384;
 * else 1), 1 GEMV with the q8_K quantization of x fused in (K <= 16384; column tiles of 8 for N > 8, bitwise the
 * per-tile calls), 4 exact: bit-identical to the AVX2 branch of ggml_vec_dot_q6_K_q8_K (k_quants.c:3484-3561),
 * 5 prefill GEMM on the int8 matrix cores (any K % 256 == 0): the Q6_K bytes read in place, x quantized to q8_K
 * into the workspace; every y bit for bit algo 1's (the same exact integer superblock sums and the same fp32
 * step per superblock, in order), so the auto switch between 1 and 5 never changes a result.  2 and 3 are invalid. */
int ggml_hip_mul_mat_q6_K(const void *dev_w, int64_t K, int64_t M, const float *dev_x, int64_t N,
                          float *dev_y, int64_t ldy, int algo, void *stream);
/* debug, no device needed: the algo that algo 0 of ggml_hip_mul_mat_q6_K would run now: 1, 4 or 5 */
int ggml_hip_debug_q6k_auto_algo(int64_t K, int64_t M, int64_t N);
/* debug: the smallest N at which auto takes the GEMM (default: the measured crossover; GGML_HIP_Q6K_GEMM_MIN_N;
 * values below 9 count as 9); -1 restores the environment value or the default.  Returns the previous value. */
int ggml_hip_debug_set_q6k_gemm_min_n(int n);
/* Q8_0 WEIGHTS (block_q8_0 rows, 34 bytes per 32 weights; dev_w 4-byte aligned, K % 64 == 0 so every row is) x F32
 * -> F32 with the semantics of ggml_vec_dot_q8_0_q8_0 on the bit-exact q8_0 of x.  Stream-ordered and
 * graph-capturable once ggml_hip_reserve_workspace_mm(K, N, M) has run (it covers the prefill path's per-call
 * weight image, 34 bytes per 32 weights, and the exact mode's q8_0 of x).  Status codes as for the q4_0 entry
 * points; K % 64 != 0 or ldy < M -> GGML_HIP_ERR_INVALID; N = 0 -> GGML_HIP_OK.
 * dequantize_q8_0: dequantize_row_q8_0 (ggml.c:1594-1610), bit-exact. */
int ggml_hip_dequantize_q8_0(const void *dev_wq, int64_t K, int64_t M, float *dev_w, void *stream);
/* y[n*ldy + m] = W[m] . x[n].  algo: 0 auto (4 in exact mode; else 1 below the GEMM threshold; else 2), 1 GEMV
 * with the q8_0 quantization of x fused in (column tiles of 8 for N > 8, fewer above K = 7232; a column's y is
 * bitwise the same in every tile and under every launch policy), 2 the weight's int8 image built per call into the
 * workspace, then the int8-MFMA GEMM of the q4_0 path (k_gemm8) unchanged, 4 exact: bit-identical to the AVX2
 * branch of ggml_vec_dot_q8_0_q8_0 (ggml.c:3231-3320).  Anything else -> GGML_HIP_ERR_INVALID. */
int ggml_hip_mul_mat_q8_0(const void *dev_w, int64_t K, int64_t M, const float *dev_x, int64_t N,
                          float *dev_y, int64_t ldy, int algo, void *stream);
/* debug, no device needed: the algo that algo 0 of ggml_hip_mul_mat_q8_0 would run now: 1, 2 or 4 */
int ggml_hip_debug_q8_0_auto_algo(int64_t K, int64_t M, int64_t N);
/* debug: the smallest N at which auto takes the GEMM (default 32: the measured crossover; GGML_HIP_Q8_0_GEMM_MIN_N; values
 * below 9 count as 9); -1 restores the environment value or the default.  Returns the previous value. */
int ggml_hip_debug_set_q8_0_gemm_min_n(int n);
/* Q4_1 / Q5_0 / Q5_1 WEIGHTS (block_q4_1 rows, 20 bytes per 32 weights; block_q5_0, 22; block_q5_1, 24; dev_w 4-byte
 * aligned, K % 64 == 0 so every row is) x F32 -> F32 with the semantics of ggml_vec_dot_q4_1_q8_1 /
 * ggml_vec_dot_q5_0_q8_0 / ggml_vec_dot_q5_1_q8_1 on the bit-exact q8_1 (Q4_1, Q5_1) or q8_0 (Q5_0) of x.
 * Stream-ordered and graph-capturable once ggml_hip_reserve_workspace(K, N) has run (the planes of x of the exact
 * mode and of the Q4_1 / Q5_1 GEMM, 40 bytes per 32 elements for q8_1) or, for Q5_0's GEMM, ggml_hip_reserve_workspace_mm(K, N, M).  No byte outside the
 * matrix is read.  Status codes as for ggml_hip_mul_mat_q8_0; N = 0 -> GGML_HIP_OK.
 * dequantize_q4_1 / _q5_0 / _q5_1: dequantize_row_q4_1 / _q5_0 / _q5_1 (ggml.c:1520-1592), bit-exact. */
int ggml_hip_dequantize_q4_1(const void *dev_wq, int64_t K, int64_t M, float *dev_w, void *stream);
int ggml_hip_dequantize_q5_0(const void *dev_wq, int64_t K, int64_t M, float *dev_w, void *stream);
int ggml_hip_dequantize_q5_1(const void *dev_wq, int64_t K, int64_t M, float *dev_w, void *stream);
/* q8_1 quantize of N activation rows, ggml block_q8_1 output (f32 d, f32 s, qs[32]: 40*K/32 bytes per row, 4-byte
 * aligned); bit-exact to quantize_row_q8_1's AVX2 branch (ggml.c:1402-1463). */
int ggml_hip_quantize_q8_1(const float *dev_x, int64_t K, int64_t N, void *dev_xq, void *stream);
/* y[n*ldy + m] = W[m] . x[n].  algo: 0 auto (4 in exact mode and where K is too long for the GEMV on Q4_1 / Q5_1;
 * Q5_0: 2 from the GEMM threshold and where K is too long for the GEMV; Q4_1 / Q5_1: 7 from their GEMM threshold,
 * whose default is "never"; else 1), 1 GEMV with the quantization of x
 * fused in (column tiles of 8 for N > 8, fewer above K = 6528, GGML_HIP_ERR_UNSUPPORTED where one token does not fit
 * the LDS; a column's y is bitwise the same in every tile and under every launch policy), 2 (Q5_0 only) the int8
 * image of q - 16 built per call into the workspace, then the int8-MFMA GEMM of the q4_0 path (k_gemm8) unchanged,
 * 4 exact: bit-identical to the AVX2 branch of the type's ggml_vec_dot (ggml.c:2680-2713, 2894-2916, 3144-3169), no
 * K limit, 7 (Q4_1 / Q5_1 only) prefill GEMM on the int8 matrix cores (any K % 64 == 0, any N >= 1): the blocks read
 * in place, x quantized to q8_1 planes into the workspace; per output one fp32 chain over the blocks in order, acc =
 * fma((float)isum_b, d_w * d_x, acc) then acc = fma(m_w, s_x, acc) with the exact integer block sum isum_b, so y
 * depends on (row, column, K) alone and is within the parity bound of algo 1's, not bitwise it.  Anything else (2 on
 * Q4_1 / Q5_1 and 7 on Q5_0 included) -> GGML_HIP_ERR_INVALID. */
int ggml_hip_mul_mat_q4_1(const void *dev_w, int64_t K, int64_t M, const float *dev_x, int64_t N,
                          float *dev_y, int64_t ldy, int algo, void *stream);
int ggml_hip_mul_mat_q5_0(const void *dev_w, int64_t K, int64_t M, const float *dev_x, int64_t N,
                          float *dev_y, int64_t ldy, int algo, void *stream);
int ggml_hip_mul_mat_q5_1(const void *dev_w, int64_t K, int64_t M, const float *dev_x, int64_t N,
                          float *dev_y, int64_t ldy, int algo, void *stream);
/* debug, no device needed: the algo that algo 0 of the type's mul_mat would run now: 1, 4 or 7 (Q5_0: 1, 2 or 4) */
int ggml_hip_debug_q4_1_auto_algo(int64_t K, int64_t M, int64_t N);
int ggml_hip_debug_q5_0_auto_algo(int64_t K, int64_t M, int64_t N);
int ggml_hip_debug_q5_1_auto_algo(int64_t K, int64_t M, int64_t N);
/* debug: the smallest N at which auto takes the Q5_0 GEMM (default 32: the measured crossover on the LLaMA-7B layer
 * shapes; GGML_HIP_Q5_0_GEMM_MIN_N; values below 9 count as 9); -1 restores the environment value or the default.
 * Returns the previous value. */
int ggml_hip_debug_set_q5_0_gemm_min_n(int n);
/* debug: the smallest N at which auto takes the Q4_1 / Q5_1 GEMM (algo 7).  Default INT_MAX: never, auto runs the
 * GEMV at every N; GGML_HIP_Q41_Q51_GEMM_MIN_N switches it on (the measured crossover is in DESIGN.md section 4b);
 * values below 9 count as 9; -1 restores the environment value or the default.  Returns the previous value. */
int ggml_hip_debug_set_q41_q51_gemm_min_n(int n);
/* Q5_K / Q4_K WEIGHTS (block_q5_K rows, 176 bytes per 256 weights; block_q4_K rows, 144 bytes; dev_w 16-byte
 * aligned, so every block and row is) x F32 -> F32 with the semantics of ggml_vec_dot_q5_K_q8_K /
 * ggml_vec_dot_q4_K_q8_K on the bit-exact q8_K of x.  K % 256 == 0.  Stream-ordered and capturable (exact mode
 * after ggml_hip_reserve_workspace).  No byte outside the matrix is read.  Status codes as for the q4_0 entry
 * points; N == 0 is a no-op.
 * dequantize_q5_K / _q4_K: dequantize_row_q5_K (k_quants.c:926-969) / dequantize_row_q4_K (733-770), bit-exact. */
int ggml_hip_dequantize_q5_K(const void *dev_wq, int64_t K, int64_t M, float *dev_w, void *stream);
int ggml_hip_dequantize_q4_K(const void *dev_wq, int64_t K, int64_t M, float *dev_w, void *stream);
/* y[n * ldy + m], ldy >= M.  algo: 0 auto (4 in exact mode and for K > 16384; else 6 when N >= the GEMM threshold;
 * else 1), 1 GEMV (K <= 16384) with the q8_K quantization of x fused in, exact int32 superblock sums and one fixed
 * fp32 order per superblock (column tiles of 8 for N > 8, bitwise the per-tile calls; y does not depend on the
 * launch geometry), 4 exact: bit-identical to the AVX2 branch of ggml_vec_dot_q5_K_q8_K (k_quants.c:2927-3010) /
 * ggml_vec_dot_q4_K_q8_K (2450-2513), 6 prefill GEMM on the int8 matrix cores (any K % 256 == 0): the blocks read
 * in place, x quantized to q8_K into the workspace (covered by ggml_hip_reserve_workspace(K, N)); every y bit for
 * bit algo 1's (the same exact integer superblock sums and the same fp32 step per superblock, in order), so the
 * auto switch between 1 and 6 never changes a result.  Anything else (2, 3 and 5 included) -> GGML_HIP_ERR_INVALID. */
int ggml_hip_mul_mat_q5_K(const void *dev_w, int64_t K, int64_t M, const float *dev_x, int64_t N,
                          float *dev_y, int64_t ldy, int algo, void *stream);
int ggml_hip_mul_mat_q4_K(const void *dev_w, int64_t K, int64_t M, const float *dev_x, int64_t N,
                          float *dev_y, int64_t ldy, int algo, void *stream);
/* debug, no device needed: the algo that algo 0 of ggml_hip_mul_mat_q5_K / _q4_K (type = GGML_TYPE_Q5_K 13 /
 * GGML_TYPE_Q4_K 12) would run now: 1, 4 or 6; a bad type or K -> GGML_HIP_ERR_INVALID */
int ggml_hip_debug_q45k_auto_algo(int type, int64_t K, int64_t M, int64_t N);
/* debug: the smallest N at which auto takes the GEMM, one value for both types (default 32: the measured crossover;
 * GGML_HIP_Q45K_GEMM_MIN_N; values below 9 count as 9); -1 restores the environment value or the default.  Returns
 * the previous value. */
int ggml_hip_debug_set_q45k_gemm_min_n(int n);
/* the hook path (can_mul_mat, transform_tensor, compute_forward, ggml_hip_mul_mat) takes GGML_TYPE_Q4_K tensors
 * only while this switch is on; off by default (or GGML_HIP_Q4_K=1 in the environment).  Off, a Q4_K matrix stays a
 * CPU tensor on a host copy; a mul_mat of it whose src1 or dst is a device tensor (an offloaded layer) is still
 * computed here, from that copy, because ggml's CPU op asserts host operands.  Returns the previous
 * value (0 / 1).  Tensors uploaded while it was on stay on the device, keep being served by
 * compute_forward after it is turned off (their data is not on the host), and are freed by ggml_hip_free_data. */
int ggml_hip_debug_set_q4_K(int on);
/* Q3_K / Q2_K WEIGHTS (block_q3_K rows, 110 bytes per 256 weights; block_q2_K rows, 84 bytes; dev_w 4-byte aligned,
 * which leaves a Q3_K block at 0 or 2 mod 4: every 32-bit field is read through the aligned dwords that hold it)
 * x F32 -> F32 with the semantics of ggml_vec_dot_q3_K_q8_K / ggml_vec_dot_q2_K_q8_K on the bit-exact q8_K of x.
 * K % 256 == 0.  Stream-ordered and capturable (exact mode after ggml_hip_reserve_workspace).  No byte outside
 * [dev_w, dev_w + M * (K / 256) * 110 or 84) is read.  Status codes as for the q4_0 entry points; N == 0 is a no-op.
 * dequantize_q3_K / _q2_K: dequantize_row_q3_K (k_quants.c:531-579) / dequantize_row_q2_K (352-396), bit-exact. */
int ggml_hip_dequantize_q3_K(const void *dev_wq, int64_t K, int64_t M, float *dev_w, void *stream);
int ggml_hip_dequantize_q2_K(const void *dev_wq, int64_t K, int64_t M, float *dev_w, void *stream);
/* y[n * ldy + m], ldy >= M.  algo: 0 auto (4 in exact mode and for K > 16384; else 8 when N >= the GEMM threshold,
 * which is "never" unless set; else 1), 1 GEMV (K <= 16384) with the q8_K quantization of x fused in, exact int32 superblock sums and one fixed fp32 order per superblock (column
 * tiles of 8 for N > 8, bitwise the per-tile calls; y does not depend on the launch geometry), 4 exact:
 * bit-identical to the AVX2 branch of ggml_vec_dot_q3_K_q8_K (k_quants.c:1836-1938) / ggml_vec_dot_q2_K_q8_K
 * (1330-1394), 8 prefill GEMM on the int8 matrix cores (any K % 256 == 0): the blocks read in place, the scale
 * folded into the int8 weight, x quantized to q8_K into the workspace (covered by ggml_hip_reserve_workspace(K, N));
 * every y bit for bit algo 1's (the same exact integer superblock sums and the same fp32 step per superblock, in
 * order), so the auto switch between 1 and 8 never changes a result.  Anything else (2, 3, 5, 6 and 7 included) ->
 * GGML_HIP_ERR_INVALID. */
int ggml_hip_mul_mat_q3_K(const void *dev_w, int64_t K, int64_t M, const float *dev_x, int64_t N,
                          float *dev_y, int64_t ldy, int algo, void *stream);
int ggml_hip_mul_mat_q2_K(const void *dev_w, int64_t K, int64_t M, const float *dev_x, int64_t N,
                          float *dev_y, int64_t ldy, int algo, void *stream);
/* debug, no device needed: the algo that algo 0 of ggml_hip_mul_mat_q3_K / _q2_K (type = GGML_TYPE_Q3_K 11 /
 * GGML_TYPE_Q2_K 10) would run now: 1, 4 or 8; a bad type or K -> GGML_HIP_ERR_INVALID */
int ggml_hip_debug_q23k_auto_algo(int type, int64_t K, int64_t M, int64_t N);
/* debug: the smallest N at which auto takes the Q3_K / Q2_K GEMM (algo 8), one value for both types.  Default
 * INT_MAX: never, auto runs the GEMV at every N; GGML_HIP_Q23K_GEMM_MIN_N switches it on (the measured crossover is
 * in DESIGN.md section 4b); values below 9 count as 9; -1 restores the environment value or the default.  Returns
 * the previous value. */
int ggml_hip_debug_set_q23k_gemm_min_n(int n);
/* F16 WEIGHTS (contiguous rows of K halves; dev_w 16-byte aligned, K % 32 == 0: the matrices of a "mostly F16" file)
 * x F32 -> F32 with the semantics of ggml_compute_forward_mul_mat_f16_f32 (ggml.c:11026): x is rounded to fp16
 * (round to nearest even) and every product of two fp16 values is exact in fp32.  y[n * ldy + m], ldy >= M.
 * Stream-ordered and capturable; no workspace but algo 11's.  No byte outside [dev_w, dev_w + M * K * 2) is read.  Status
 * codes as for the q4_0 entry points; N == 0 is a no-op.  algo: 0 auto (4 in exact mode; else 11 when N >= the
 * weight-shaped GEMM's threshold, default never, at any K; else 4 for a K the GEMV cannot take; else
 * 9 when N >= the GEMM threshold; else 1), 1 GEMV (K <= 65536) with the fp16 rounding of x fused in and one fixed
 * order of the fp32 additions per K (csrc/f16_w.hip, restated in tests/f16w_ref.py; column tiles of at most 8 above
 * that, bitwise the per-tile calls; y does not depend on N, M or the launch geometry) — within the fp32-accumulation
 * bound of the reference, 4 exact: bit-identical to ggml_vec_dot_f16 in its AVX2 / F16C schedule (the kernels of
 * the attention's F16 x F32 products, ldy == M only), 9 prefill GEMM on the f16 matrix cores (the attention's
 * fast-mode kernel, ldy == M only; within the same bound), 11 prefill GEMM decomposed for weight shapes
 * (csrc/f16_w_gemm.hip: v_mfma_f32_32x32x16_f16 on 64-element K chunks, narrow row tiles and a K split where the
 * shape alone does not fill the device).  Algo 11 takes any K % 32 == 0, any M, N >= 1 and any ldy >= M, reads no
 * byte outside dev_w's M * K * 2 and dev_x's N * K * 4 and writes only the M columns of the N rows of y.  Per output
 * |y - S| <= 1e-5 * sum |W * fp16(x)| of the float64 sum S of the exact products (algo 9's bound); it is
 * deterministic, and not bitwise algo 1 or 9: the switch moves a result within the bound, and exact mode never takes
 * it.  The order of one output's additions depends on K and on the plan (one of three tile / K-split
 * decompositions, a pure function of K, M, N and the device's CU count) and on nothing else, so with the plan pinned
 * (ggml_hip_debug_set_f16w_wgemm_plan) a column or row slice of a call is bitwise the call on that slice.  It uses
 * the stream's workspace: the fp16 image of x (2 * N * K bytes) and, for a plan that splits K, one fp32 [N][M] slab
 * per slice (at most 4), added in slice order by a second launch (no atomics, no waiting between workgroups);
 * ggml_hip_reserve_workspace_mm(K, N, M) reserves it for the plan in force at the time of the reservation, and a
 * reserved call is capturable.  Anything else (2, 3, 5, 6, 7, 8 and 10 included) -> GGML_HIP_ERR_INVALID, before
 * anything else is checked; 4 or 9 with ldy != M, and 11 on a shape whose tiles exceed one grid ->
 * GGML_HIP_ERR_UNSUPPORTED (auto then falls back to the rule without 11). */
int ggml_hip_mul_mat_f16(const void *dev_w, int64_t K, int64_t M, const float *dev_x, int64_t N,
                         float *dev_y, int64_t ldy, int algo, void *stream);
/* debug, no device needed: the algo that algo 0 of ggml_hip_mul_mat_f16 would run now: 1, 4, 9 or 11; a bad K ->
 * GGML_HIP_ERR_INVALID */
int ggml_hip_debug_f16w_auto_algo(int64_t K, int64_t M, int64_t N);
/* debug: the smallest N at which auto takes the weight-shaped F16 GEMM (algo 11).  Default never
 * (GGML_HIP_F16W_WGEMM_MIN_N; the measured rows are in DESIGN.md section 4b); values below 9 count as 9; -1 restores
 * the environment value or the default.  Returns the previous value. */
int ggml_hip_debug_set_f16w_wgemm_min_n(int n);
/* debug: pin algo 11's plan: 0 auto, 1 (32 rows x 64 columns, K split over the waves and 4 workgroups), 2 (64 x 128,
 * K split 2), 3 (128 x 128, no split).  Returns the previous value; anything else -> GGML_HIP_ERR_INVALID. */
int ggml_hip_debug_set_f16w_wgemm_plan(int plan);
/* debug, no device needed: the plan auto would take now for this shape (the current device's CU count; 256 where no
 * device is initialised), whatever is pinned */
int ggml_hip_debug_f16w_wgemm_plan(int64_t K, int64_t M, int64_t N);
/* debug: the smallest N at which auto takes the F16 GEMM (algo 9).  Default 32 (GGML_HIP_F16W_GEMM_MIN_N; the
 * measured rows are in DESIGN.md section 4b); values below 9 count as 9; -1 restores the environment value or the
 * default.  Returns the previous value. */
int ggml_hip_debug_set_f16w_gemm_min_n(int n);
/* F32 WEIGHTS (contiguous rows of K floats; dev_w 16-byte aligned, K % 32 == 0: the matrices of an "all F32" file,
 * ftype 0) x F32 -> F32 with the semantics of ggml_compute_forward_mul_mat_f32 (ggml.c:10855): no operand is rounded,
 * every product enters by one fmaf, fp32 subnormals are kept.  y[n * ldy + m], any ldy >= M for every algo.
 * Stream-ordered and capturable; no workspace but algo 12's.  No byte outside [dev_w, dev_w + M * K * 4) and
 * [dev_x, dev_x + N * K * 4) is read, and only the M columns of the N rows of y are written.  Status codes as for
 * ggml_hip_mul_mat_f16; N == 0 is a no-op.  algo: 0 auto (4 in exact mode; else 4 for a K the GEMV cannot take; else 12
 * when N >= the GEMM threshold; else 1), 1 GEMV (K <= 32768; column tiles of min(8, 32768 / K) columns, bitwise the
 * per-tile calls) with one fixed order of the additions per K (csrc/f32_w.hip, restated in tests/f32w_ref.py
 * gemv_schedule; y does not depend on N, M or the launch geometry), 4 exact: bit-identical to ggml_vec_dot_f32 in its
 * AVX2 + FMA schedule (32 chains, GGML_F32x8_REDUCE), 12 prefill GEMM on v_mfma_f32_32x32x2_f32 (csrc/f32_w_gemm.hip):
 * K is cut into S (1, 2 or 4) equal slices, each ONE fmaf chain per output over the slice's elements in natural order
 * from +0, the slices' values added in slice order by a second launch (no atomics); y is bitwise
 * tests/f32w_ref.py gemm_schedule(w, x, S) and depends on (row, column, K, S) alone, so with S pinned a column or row
 * slice of a call is bitwise the call on that slice.  S is a pure function of K, M, N and the device's CU count unless
 * pinned; a requested S for which K / S is no multiple of 32 runs as the next smaller one.  Algo 12 uses the stream's
 * workspace for S > 1 (S fp32 [N][M] slabs); ggml_hip_reserve_workspace_mm(K, N, M) reserves it for the split in force
 * at the time of the reservation, and a reserved call is capturable.  Every algo is within
 * |y - S64| <= 1.01 * K * 2^-24 * sum |W * x| of the float64 sum S64 of the exact products.  Anything else (2, 3, 5 - 11,
 * 13 included) -> GGML_HIP_ERR_INVALID, before anything else is checked; 1 on K > 32768 and 12 on a shape whose tiles
 * exceed one grid -> GGML_HIP_ERR_UNSUPPORTED (auto then runs the GEMV's tiles). */
int ggml_hip_mul_mat_f32(const void *dev_w, int64_t K, int64_t M, const float *dev_x, int64_t N,
                         float *dev_y, int64_t ldy, int algo, void *stream);
/* debug, no device needed: the algo that algo 0 of ggml_hip_mul_mat_f32 would run now: 1, 4 or 12; a bad K ->
 * GGML_HIP_ERR_INVALID */
int ggml_hip_debug_f32w_auto_algo(int64_t K, int64_t M, int64_t N);
/* debug: the smallest N at which auto takes the F32 GEMM (algo 12).  Default 16, the measured crossover (GGML_HIP_F32W_GEMM_MIN_N; DESIGN.md
 * section 4b); values below 9 count as 9; -1 restores the environment value or the default.  Returns the previous
 * value. */
int ggml_hip_debug_set_f32w_gemm_min_n(int n);
/* debug: pin algo 12's K split: 0 auto, 1, 2 or 4.  Returns the previous value; anything else ->
 * GGML_HIP_ERR_INVALID. */
int ggml_hip_debug_set_f32w_gemm_ksplit(int s);
/* debug, no device needed: the split auto would run now for this shape (the current device's CU count; 256 where no
 * device is initialised), whatever is pinned */
int ggml_hip_debug_f32w_gemm_ksplit(int64_t K, int64_t M, int64_t N);
/* The hook path takes an ALL-HOST mul_mat with an F32 weight (a contiguous 2-D F32 leaf, K % 32 == 0) only with this
 * switch on (GGML_HIP_F32_W=1; default off, so the small F32 matrices of graphs that never offload stay on ggml's CPU
 * op).  A matrix ggml_hip_transform_tensor uploaded, or a host one between device operands, is served regardless.
 * Returns the previous value (0 / 1). */
int ggml_hip_debug_set_f32_w(int on);

/* Sibling mul_mats that share the activation x (ggml graphs issue wq/wk/wv and w1/w3 on the same
 * src1): n <= 4 weight matrices of the same K, y_i = W_i x with y_i f32 [N][M_i].  One launch for
 * N <= 8 (rows concatenated); for N > 8 x is quantized once and each W_i runs the GEMM.  Results
 * are identical to n separate ggml_hip_mul_mat_q4_0 calls, except where siblings with fp6 weight images
 * run as one prefill launch whose tile plan (128 x 64 / 128 x 128, by the launch's tile count) differs from
 * the single calls' (within the oracle bound; bitwise with ggml_hip_debug_set_gemm9_wide pinning the tile). */
int ggml_hip_mul_mat_q4_0_multi(int n, const void *const *dev_w, const int64_t *M, int64_t K, const float *dev_x,
                                int64_t N, float *const *dev_y, void *stream);
/* Exact (reproducible) mode, process-wide: every auto-selected mul_mat, including the ggml hook
 * path (ggml_hip_mul_mat / ggml_hip_compute_forward) and the sibling-matrix calls, runs algorithm 4,
 * so a ggml graph on this backend reproduces the reference CPU build's mul_mat outputs bit for bit.
 * Default off (GGML_HIP_EXACT=1 switches it on at first use); the fast kernels stay within the
 * north-star 1e-3 tolerance.  No ggml-cuda.h counterpart. */
int ggml_hip_set_exact(int on);
int ggml_hip_get_exact(void);
/* Ensure the current device's workspace can serve mul_mat for N tokens of K (call before
 * capturing a HIP graph). */
int ggml_hip_reserve_workspace(int64_t K, int64_t N);
/* The same for prefill mul_mats (N > 128) of matrices up to M rows: the LDS GEMM also keeps a per-call
 * image of the weights in the workspace (up to 34 bytes per 32 weights). */
int ggml_hip_reserve_workspace_mm(int64_t K, int64_t N, int64_t M);

/* Prefill weight images (no ggml-cuda.h counterpart).  The LDS GEMM (N > 64 with an image, N > 128 without) runs fastest on an image
 * of the weight: by default fp6 (e2m3 codes of w/2, w = nibble - 8, fp16 d verbatim; 26 B per 32
 * weights, 1.44x the q4_0 bytes; the exact block sums on the block-scaled fp6 MFMA, k_gemm9), under GEMM
 * version 8 int8 (34 B per 32 weights, k_gemm8; bitwise the same results): create builds it once
 * (stream-ordered, outside capture) and every later prefill mul_mat of that device pointer with the
 * same K, M uses it; without one the GEMM reads the q4_0 bytes directly.  The weight
 * must not change while its image exists (free it first).  Device-resident ggml weights
 * (transform_tensor, the residency cache) get their image on their first prefill use, dropped with the
 * buffer.  Results are identical either way in exact arithmetic per block; the fp32 accumulation order
 * of the two GEMMs differs (both within the parity bound). */
int ggml_hip_weight_image_create(const void *dev_w, int64_t K, int64_t M, void *stream);
int ggml_hip_weight_image_free(const void *dev_w);        /* number of images dropped */
int64_t ggml_hip_weight_image_bytes(void);                  /* device bytes held by images */
/* test hook: prefill GEMM version 7 (q4_0 bytes), 8 / 10 (int8 / fp6 images built on registration, the
 * GEMM of the image when one exists; 10 is the default), 9 / 11 (k_gemm8 / k_gemm9 always, an
 * unregistered weight converted per call into the workspace); -1 = GGML_HIP_GEMM_V */
int ggml_hip_debug_set_gemm_version(int v);
// k_gemm9's tile: -1 = automatic (128 x 128 where it takes fewer CU rounds than 128 x 64; GGML_HIP_GEMM9_WIDE
// overrides), 0 = always 128 x 64, 1 = always 128 x 128 (block order: y within the oracle bound of 128 x 64's).
int ggml_hip_debug_set_gemm9_wide(int mode);

/* ------------------------------------------------------------------------------------------
 * Decode chains: a sequence of dependent N = 1 q4_0 mul_mats, validated once and launched together.
 * A decode eval issues its q4_0 mul_mats one after another on one stream (llama.cpp:1217-1600 ->
 * ggml_compute_forward_mul_mat_q_f32, ggml.c:11226-11411).  A chain runs tasks 0..n-1 in stream order,
 * each as one sibling GEMV launch (ggml_hip_mul_mat_q4_0_multi with N = 1): task t reads x only after
 * every task < t has written its y, so x of a task may be, or overlap, the y of an earlier task.
 * Results are bitwise those of n separate ggml_hip_mul_mat_q4_0_multi calls (exact mode included).
 * A task's y must not overlap its own x (create rejects it).  Graph-capturable.  Two in-launch
 * designs (one persistent launch, round 2; overlapped launches with flag hand-offs, round 4) were
 * bitwise equal and slower.  No ggml-cuda.h counterpart.
 * ---------------------------------------------------------------------------------------- */
typedef struct ggml_hip_chain_task {
    int nmat;                 /* 1..4 sibling matrices sharing x (e.g. wq|wk|wv) */
    int64_t K;                /* K % 64 == 0 */
    const float *x;           /* f32 [K], 16-byte aligned */
    const void *W[4];         /* block_q4_0 rows, M[i] x K, 16-byte aligned */
    int64_t M[4];
    float *y[4];              /* f32 [M[i]] */
} ggml_hip_chain_task;
typedef struct ggml_hip_chain ggml_hip_chain;
/* Validates the tasks (no device work). */
int ggml_hip_chain_create(int ntasks, const ggml_hip_chain_task *tasks, ggml_hip_chain **chain);
/* N-token chains (prefill): x of a task is f32 [N][K], y[i] f32 [N][M[i]]; otherwise as above, bitwise n
 * separate ggml_hip_mul_mat_q4_0_multi calls at N.  A task whose siblings take one k_gemm9 launch on fp6
 * weight images (ggml_hip_weight_image_create) reads a chain-owned x image (gemm9 x bytes per task,
 * allocated at create), built by k_prep9_x; with the epilogue fold on (ggml_hip_debug_set_chain_x9(1)), a
 * task whose x is exactly y[i] of an earlier such task (M[i] == K, nothing in between writes it) gets it
 * from that task's GEMM epilogue instead (bitwise the same; measured slower, so off by default). */
int ggml_hip_chain_create_n(int ntasks, const ggml_hip_chain_task *tasks, int64_t N, ggml_hip_chain **chain);
/* debug: 1 = N-token chains take x images from the producers' GEMM epilogues, 0 = every image by
 * k_prep9_x (default), -1 = GGML_HIP_CHAIN_X9 (1 turns the fold on) */
int ggml_hip_debug_set_chain_x9(int on);
/* debug, no device needed: the epilogue links ggml_hip_chain_create_n would plan; prod[t] = the task whose
 * epilogue writes task t's x image (-1: k_prep9_x), share[t] = the earlier consumer whose image t reads (-1) */
int ggml_hip_debug_chain_links(int ntasks, const ggml_hip_chain_task *tasks, int64_t N, int *prod, int *share);
/* Stream-ordered (graph-capturable): one GEMV launch per task. */
int ggml_hip_chain_launch(ggml_hip_chain *chain, void *stream);
/* Synchronizes the device; 0, or (engine) the nonzero error bits of a bounded wait that expired. */
int ggml_hip_chain_status(ggml_hip_chain *chain);
int ggml_hip_chain_destroy(ggml_hip_chain *chain);
/* The persistent decode engine: the whole chain as ONE launch, one workgroup per CU, a loader
 * wave streaming each CU's weight rows by LDS-DMA ahead across the dependency edges, the edges carried by q8_0
 * blocks quantized once by their producer.  Results are bitwise those of the per-launch chain.  It takes chains
 * in which every task t >= 1 reads x = y[i] of task t - 1 (the same pointer, its first K values), task 0 reads an
 * x that no task writes, K <= 12288, and any output region written again later is ordered by the edges; other
 * chains, and every launch in exact mode, keep the per-launch path.  It needs the device to itself while it
 * runs (all workgroups co-resident); every wait is bounded (GGML_HIP_ENGINE_TIMEOUT_MS, default 2000) and
 * chain_status reports an expired one.  mode 1 on (builds the plan; returns 1 when the engine runs the chain, 0
 * when it declined: ggml_hip_last_error says why), 0 off, -1 query.  GGML_HIP_CHAIN_ENGINE=1 turns it on at
 * create.  info: [0] engine on, [1] work units, [2] largest per-CU stream (bytes), [3] weight bytes, [4] CUs,
 * [5] (N-token chains) tasks whose x image a producer's GEMM epilogue writes. */
int ggml_hip_chain_set_engine(ggml_hip_chain *chain, int mode);
int ggml_hip_chain_engine_info(ggml_hip_chain *chain, int64_t *info, int n);

/* ------------------------------------------------------------------------------------------
 * Multi-GPU, one process per GPU (torch.distributed-style ranks), RCCL over xGMI.
 * The reference row-splits weights across devices (GGML_BACKEND_GPU_SPLIT, ggml-cuda.cu:
 * 2361-2368, 2773-2806) and gathers each device's dst rows with cudaMemcpyAsync
 * (ggml-cuda.cu:2514-2539); here every rank holds rows [row_begin[rank], row_begin[rank+1])
 * and the slices are exchanged with one ncclAllGather.
 * ---------------------------------------------------------------------------------------- */
typedef struct ggml_hip_comm ggml_hip_comm;

#define GGML_HIP_UNIQUE_ID_BYTES 128
/* rank 0 creates the id and ships it to the other ranks (e.g. torch.distributed broadcast). */
int ggml_hip_comm_unique_id(char out[GGML_HIP_UNIQUE_ID_BYTES]);
int ggml_hip_comm_init(ggml_hip_comm **comm, int nranks, int rank, const char id[GGML_HIP_UNIQUE_ID_BYTES]);
int ggml_hip_comm_destroy(ggml_hip_comm *comm);
/* In-process loopback group (testing / single-process multi-device): creates nranks
 * communicators comms[0..nranks-1] whose all-gather has ncclAllGather's semantics, for nranks
 * host threads of this process that each drive one rank (rank r on devices[r], or all on the
 * current device when devices is NULL; give each rank its own stream).  Every split entry point
 * below runs the same code on either transport.  Destroy each comm with ggml_hip_comm_destroy. */
int ggml_hip_comm_init_local(ggml_hip_comm **comms, int nranks, const int *devices);
/* One process per rank without RCCL: the comm's host collectives (allreduce_host, the P2P handle
 * exchange) go through files in dir, a directory every rank can read and write (rank r writes
 * <dir>/c<nonce>_<seq>_r<r>).  Init is collective: rank 0 publishes a fresh session nonce as <dir>/session
 * and refuses a directory where that name exists (a session in progress or a crashed one's leftover), so
 * files of different sessions never mix.  Device all-gathers need the P2P transport (ggml_hip_comm_enable_p2p); the RCCL
 * transport is unavailable.  It also lets several processes share ONE device (RCCL refuses that),
 * which is how the cross-process IPC path of the P2P all-gather is tested on a one-GPU box. */
int ggml_hip_comm_init_file(ggml_hip_comm **comm, int nranks, int rank, const char *dir);
int ggml_hip_comm_rank(const ggml_hip_comm *comm, int *rank, int *nranks);
/* Direct-store all-gather (SURVEY.md §8e's P2P alternative to ncclAllGather for latency-bound decode
 * gathers): each rank stores its slice straight into every peer's landing buffer over xGMI (an IPC
 * mapping across processes, the buffer itself in a loopback group) and raises a flag there; one
 * kernel per all-gather, graph-capturable (the epoch advances on the device).  Collective: call on
 * every rank of the comm with the same max_floats (the largest slice of one all-gather, floats);
 * at most 8 ranks.  After it the comm's all-gathers (the split mul_mats) use P2P stores;
 * set_transport(comm, 0) returns to RCCL (1 = P2P again).  Every rank takes part in every collective of
 * enable_p2p and the outcome is the group's: all ranks enable it or all return an error.
 * Failure: a peer's data that does not arrive within the timeout (set_p2p_timeout, ms; <= 0 selects
 * GGML_HIP_P2P_TIMEOUT_MS, default 10000) FAILS the comm for good: that gather writes NaN into the
 * peer's segment (never the stale landing slot), later gathers fill every peer segment with NaN
 * without waiting, and the next split mul_mat / all-gather on the comm returns GGML_HIP_ERR_COMM
 * before enqueueing anything (the reference stops at its first failed copy, CUDA_CHECK,
 * ggml-cuda.cu:22-51).  The rank that sees a failure first notifies every peer (a failure word stored
 * into each peer's control block over the same mapping), and the peers' waits poll it, so every rank
 * fails within one poll instead of after its own timeout.  p2p_status synchronizes the device and
 * returns 0, or the bit mask of peers whose data never arrived or that reported a failure (sticky).
 * comm_abort fails this rank's comm on purpose and sends the same notice (ncclCommAbort's role; the
 * timeout is a kernel argument, so gathers captured in a HIP graph keep the value of their capture). */
int ggml_hip_comm_enable_p2p(ggml_hip_comm *comm, int64_t max_floats);
int ggml_hip_comm_set_transport(ggml_hip_comm *comm, int transport);
int ggml_hip_comm_p2p_status(ggml_hip_comm *comm);
int ggml_hip_comm_set_p2p_timeout(ggml_hip_comm *comm, double ms);
int ggml_hip_comm_abort(ggml_hip_comm *comm);
/* All-reduce of n <= 64 host doubles in place (op 0 sum, 1 max, 2 min) over the comm; synchronous,
 * so it is also a barrier (bench harness: max-over-ranks timing without a second runtime). */
int ggml_hip_comm_allreduce_host(ggml_hip_comm *comm, double *vals, int n, int op);
/* All-gather of host bytes: recv[r * bytes ...] = rank r's send (every transport; synchronous). */
int ggml_hip_comm_allgather_host(ggml_hip_comm *comm, const void *send, size_t bytes, void *recv);
/* Row split of M rows over nranks by cumulative fractions (NULL = equal split), the same
 * rule as the reference's tensor_split (ggml-cuda.cu:1863-1882, 2361-2368).  row_begin has
 * nranks+1 entries. */
int ggml_hip_split_rows(int64_t M, int nranks, const float *tensor_split, int64_t *row_begin);
/* y_full[N][M_total] = W_full x on every rank; this rank holds W rows
 * [row_begin[rank], row_begin[rank+1]) in dev_w_local (block_q4_0 rows).  Equal splits with
 * N == 1 gather straight into y_full; otherwise through a padded slab + compaction. */
int ggml_hip_mul_mat_q4_0_split(ggml_hip_comm *comm, const void *dev_w_local, int64_t K, int64_t M_total,
                                const int64_t *row_begin, const float *dev_x, int64_t N, float *dev_y_full,
                                void *stream);
/* Sibling form ("fuse QKV (3) and w1/w3 (2) into one all-gather each"): n <= 4
 * matrices sharing x, matrix i row-split by row_begin[i] (nranks+1 entries each).  With equal
 * splits and N == 1 this rank's slices are computed by ONE multi-matrix GEMV launch straight into
 * their places in y_full[i], then ONE grouped RCCL all-gather (ncclGroupStart/End) completes all
 * n outputs in place.  Other cases run ggml_hip_mul_mat_q4_0_split per matrix.  Results are
 * identical to n separate split calls. */
int ggml_hip_mul_mat_q4_0_split_multi(ggml_hip_comm *comm, int n, const void *const *dev_w_local, const int64_t *M_total,
                                      const int64_t *const *row_begin, int64_t K, const float *dev_x, int64_t N,
                                      float *const *dev_y_full, void *stream);

/* ------------------------------------------------------------------------------------------
 * Device plumbing for bindings (ctypes / cgo / JNI) that have no HIP headers.
 * ---------------------------------------------------------------------------------------- */
int    ggml_hip_device_count(void);
int    ggml_hip_set_device(int device);
int    ggml_hip_get_device(void);
void  *ggml_hip_dev_malloc(size_t size);
void   ggml_hip_dev_free(void *ptr);
int    ggml_hip_memcpy_h2d(void *dst, const void *src, size_t size, void *stream);
int    ggml_hip_memcpy_d2h(void *dst, const void *src, size_t size, void *stream);
int    ggml_hip_memcpy_d2d(void *dst, const void *src, size_t size, void *stream);
int    ggml_hip_memset(void *dst, int value, size_t size, void *stream);
int    ggml_hip_stream_synchronize(void *stream);
int    ggml_hip_device_synchronize(void);
void  *ggml_hip_default_stream(void);          /* the backend's stream on the current device */
void  *ggml_hip_stream_create(void);           /* a non-blocking stream on the current device */
int    ggml_hip_stream_destroy(void *stream);  /* synchronizes, frees its mul_mat workspace */
int    ggml_hip_fill_gaussian(float *dev_dst, int64_t n, uint64_t seed, float mean, float stdv, void *stream);
/* timing and HIP-graph capture on a stream (bench harness; launch-bound decode chains) */
void  *ggml_hip_event_create(void);
int    ggml_hip_event_record(void *event, void *stream);
float  ggml_hip_event_elapsed_ms(void *start, void *stop);   /* waits for stop */
void   ggml_hip_event_destroy(void *event);
typedef struct ggml_hip_graph ggml_hip_graph;
int    ggml_hip_graph_begin(void *stream);
int    ggml_hip_graph_end(void *stream, ggml_hip_graph **graph);
int    ggml_hip_graph_launch(ggml_hip_graph *graph, void *stream);
int    ggml_hip_graph_destroy(ggml_hip_graph *graph);
const char *ggml_hip_last_error(void);
const char *ggml_hip_version(void);
/* debug: counts[op] = device nodes run per ggml op (GGML_OP_COUNT = 68 slots), counts[68] = host ns
   inside ggml_hip_compute_forward, counts[69 + op] = that host time per op of the arriving node,
   counts[137 + k] = fused launches of chain k (0 add/rms_norm/mul, 1 scale/diag_mask_inf/soft_max,
   2 silu/mul, 3 rope/cpy, 4 f16 mul_mat/permute/cpy, 5 q4_0 mul_mat run while a silu is pending,
   6 sibling q4_0 GEMVs sharing src1 run as one group: wq|wk|wv, w1|w3, 7 independent rope /
   rope->cpy / cpy nodes held behind a group run as one launch, 8 decode scale -> diag_mask_inf ->
   soft_max -> KQV -> merged copy as one launch, 9 / 10 decode norm / silu chain run in the q4_0
   GEMV prologue, 11 prefill norm / silu chain that wrote the k_gemm9 x image of its output for the
   q4_0 mul_mats consuming it) */
int    ggml_hip_debug_op_stats(int64_t *counts, int n, int reset);
/* debug: the attention's f16 x f32 mul_mat on device pointers (synchronous); tiled = 0 one 32-lane
   group per output, 1 the LDS-tiled kernel, -1 the backend's choice (bit-identical either way) */
int    ggml_hip_debug_f16_mul_mat(const void *s0, const void *s1, float *d, int K, int64_t ne01, int64_t ne11,
                                  int64_t ne02, int64_t nb01, int64_t nb02, int64_t nb11, int64_t nb12,
                                  float *merged, int tiled);
/* debug: mode-0 rope (ggml_compute_forward_rope_f32) of x [ne2 tokens][ne1 heads][ne0] (byte strides
   nbx[1..3]) into d (nbd[1..3]) at positions n_past.., then (c != nullptr) ggml_cpy of d into the view c
   (F16 when to_f16; shape ne10 x ne11 x .., byte strides nb10..nb12); batched = 1 through the batched
   elementwise launch (as the hook runs rope K -> K cache behind a q4_0 group), 0 its own kernel */
int    ggml_hip_debug_rope(const void *x, void *d, void *c, int to_f16, int64_t ne0, int64_t ne1, int64_t ne2,
                           int n_past, int n_dims, const int64_t *nbx, const int64_t *nbd, int64_t ne10,
                           int64_t ne11, int64_t nb10, int64_t nb11, int64_t nb12, int batched);
/* debug: ggml_cpy F32 -> F32 / F16 (to_f16) on device pointers (synchronous): source shape ne00 x ne01 x
   n / (ne00 ne01) with byte strides nb00..nb02, target ne10 x ne11 x .. with nb10..nb12; batched = 1
   through the batched elementwise launch (as the hook runs it behind a q4_0 group), 0 as its own node */
int    ggml_hip_debug_cpy_f32(const void *x, void *d, int to_f16, int64_t n, int64_t ne00, int64_t ne01,
                              int64_t nb00, int64_t nb01, int64_t nb02, int64_t ne10, int64_t ne11, int64_t nb10,
                              int64_t nb11, int64_t nb12, int batched);
/* debug: 1/0 = launch fusion of adjacent full-offload nodes on/off (default: env GGML_HIP_FUSE, on) */
int    ggml_hip_debug_set_fuse(int on);

#ifdef __cplusplus
}
#endif

#endif /* GGML_HIP_H */
