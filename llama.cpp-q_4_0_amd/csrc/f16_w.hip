// f16_w.hip — F16 WEIGHTS x F32 mul_mat at decode and small batches (gfx950, wave64): the layer matrices of the
// "mostly F16" files (ftype 1), which the reference's GPU backend serves with convert_mul_mat_vec_f16.
//
//   k_gemv_f16w<NT>   y[n][m] = sum_e W[m][e] * fp16(x[n][e]) for NT <= 8 tokens, W contiguous F16 rows, x F32:
//                     ggml_compute_forward_mul_mat_f16_f32 (ggml.c:11026), which rounds x to fp16 first
//                     (GGML_FP32_TO_FP16: round to nearest even, q4_0_device.h f2h) and then forms exact products
//                     of two fp16 values; only the order of the fp32 additions is this kernel's own, so y is within
//                     the fp32-accumulation bound of the reference, not bitwise (the bitwise kernels are
//                     ggml_ops.hip's, exact mode).
//
// Arithmetic: v_fma_mix_f32 on the fp16 operands (exact widening, one fp32 rounding: fmaf on the widened operands),
// fp32 denormals kept.  No packed dot instruction.
//
// THE ORDER (it depends on K alone; tests/f16w_ref.py restates it in numpy): a row is walked in steps of 512 elements,
// step s = elements 512 s .. 512 s + 511.  Lane l of the row's wave owns the 8 elements 512 s + 8 l .. + 7 of every
// step (one 16-byte load) and keeps two fp32 chains per token, both starting at +0:
//     chain 0:  c0 = fma(w[e], xh[e], c0)  for e = 512 s + 8 l + 0, 2, 4, 6   (the low halves of the four dwords)
//     chain 1:  c1 = fma(w[e], xh[e], c1)  for e = 512 s + 8 l + 1, 3, 5, 7   (the high halves)
// in that order within a step, steps in increasing s.  In the last step of a K that is no multiple of 512 (K = 11008
// is 21.5 steps) the lanes with 512 s + 8 l >= K add nothing (K % 32 == 0, so a lane has all 8 elements or none).  At the
// row's end t_l = c0 + c1 per lane, and the 64 t_l are added as the balanced binary tree over the lanes in order:
// ((t_0 + t_1) + (t_2 + t_3)) + ..., six levels (wave_sum_lane63's DPP steps).  Nothing else enters: not N, not the
// column's place in its tile, not M or the row's place, not the grid or the CU count.
//
// Memory: the matrix is streamed once per launch, 16 bytes per lane and load, F16W_DEPTH steps per batch and the next
// batch (of the next row after a row's last) in flight while the current one is consumed; loads at clamped indices,
// always inside the matrix, so none sits under a branch and no byte outside W is read.  The fp16 image of the NT x
// columns is built once per workgroup in LDS ([NT][K] halves, the first batch of weight loads already in flight) and
// read with ds_read_b128.  NT K 2 bytes of LDS bound the tile: gemv_f16w_max_tokens(K).
#include "q4_0_device.h"

namespace ghip {

static constexpr int F16W_WAVES = 16;              // rows in flight per workgroup, one wave each
static constexpr int F16W_DEPTH = 4;               // 512-element steps per batch
static constexpr int F16W_LDS_MAX = 128 * 1024;    // of the x image

// nontemporal weight loads: on (default) / off, GGML_HIP_F16W_NT (tools/f16w_bench.py measures both)
static bool f16w_nt() {
    static const bool nt = env_int("GGML_HIP_F16W_NT", 1) != 0;
    return nt;
}

int gemv_f16w_max_tokens(int64_t K) {
    if (K <= 0 || K % 32) return 0;
    const int64_t n = F16W_LDS_MAX / (2 * K);
    return (int)(n > 8 ? 8 : n);
}

__device__ __forceinline__ void f16w_fma_lo(uint32_t a, uint32_t b, float &c) {   // c = fp16 a.lo * b.lo + c
    asm("v_fma_mix_f32 %0, %1, %2, %0 op_sel_hi:[1,1,0]" : "+v"(c) : "v"(a), "v"(b));
}
__device__ __forceinline__ void f16w_fma_hi(uint32_t a, uint32_t b, float &c) {   // c = fp16 a.hi * b.hi + c
    asm("v_fma_mix_f32 %0, %1, %2, %0 op_sel:[1,1,0] op_sel_hi:[1,1,0]" : "+v"(c) : "v"(a), "v"(b));
}

template <int NT, bool NTL>
__global__ __launch_bounds__(F16W_WAVES * 64) void k_gemv_f16w(const uint16_t *__restrict__ W, int K, int M,
                                                               const float *__restrict__ x, float *__restrict__ y,
                                                               int64_t ldy) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    u32x4 *xs = reinterpret_cast<u32x4 *>(smem);            // [NT][K / 8]: 8 halves per entry
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int K8 = K >> 3;                                  // 16-byte pieces of a row
    const int nsteps = (K + 511) >> 9;
    const int stride = gridDim.x * F16W_WAVES;
    // (unconditional loads at clamped indices, always inside the matrix: a load under a branch would make the
    // compiler wait for every load in flight, the prefetched batch included, before the first use)
    auto load_batch = [&](int m, int s0, u32x4 *r) __attribute__((always_inline)) {
        const u32x4 *row = reinterpret_cast<const u32x4 *>(W + (int64_t)(m < M ? m : M - 1) * K);
#pragma unroll
        for (int u = 0; u < F16W_DEPTH; u++) {
            const int q = (s0 + u) * 64 + lane;
            const u32x4 *p = row + (q < K8 ? q : K8 - 1);
            r[u] = NTL ? __builtin_nontemporal_load(p) : *p;
        }
    };
    int m = blockIdx.x * F16W_WAVES + wave, s0 = 0;
    u32x4 cur[F16W_DEPTH], nxt[F16W_DEPTH];
    load_batch(m, s0, cur);
    // the fp16 image of x: [NT][K] f32 -> [NT][K] halves, 8 per thread and pass
    for (int i = threadIdx.x; i < NT * K8; i += F16W_WAVES * 64) {
        const float4 a = reinterpret_cast<const float4 *>(x)[2 * i], b = reinterpret_cast<const float4 *>(x)[2 * i + 1];
        u32x4 h;
        h.x = f2h(a.x) | (f2h(a.y) << 16);
        h.y = f2h(a.z) | (f2h(a.w) << 16);
        h.z = f2h(b.x) | (f2h(b.y) << 16);
        h.w = f2h(b.z) | (f2h(b.w) << 16);
        xs[i] = h;
    }
    __syncthreads();
    float c0[NT], c1[NT];
#pragma unroll
    for (int n = 0; n < NT; n++) c0[n] = c1[n] = 0.0f;
    while (m < M) {                                         // wave-uniform
        const bool last = s0 + F16W_DEPTH >= nsteps;        // of this row
        const int nm = last ? m + stride : m, ns0 = last ? 0 : s0 + F16W_DEPTH;
        load_batch(nm, ns0, nxt);
#pragma unroll
        for (int u = 0; u < F16W_DEPTH; u++) {
            const int q = (s0 + u) * 64 + lane;
            const int qc = q < K8 ? q : K8 - 1;             // the LDS reads clamped too: issued ahead of the branch
            u32x4 xv[NT];
#pragma unroll
            for (int n = 0; n < NT; n++) xv[n] = xs[n * K8 + qc];
            if (q < K8) {                                   // a lane past the row's end (or the row's last step) adds nothing
                const u32x4 w = cur[u];
#pragma unroll
                for (int n = 0; n < NT; n++) {
                    f16w_fma_lo(w.x, xv[n].x, c0[n]);
                    f16w_fma_hi(w.x, xv[n].x, c1[n]);
                    f16w_fma_lo(w.y, xv[n].y, c0[n]);
                    f16w_fma_hi(w.y, xv[n].y, c1[n]);
                    f16w_fma_lo(w.z, xv[n].z, c0[n]);
                    f16w_fma_hi(w.z, xv[n].z, c1[n]);
                    f16w_fma_lo(w.w, xv[n].w, c0[n]);
                    f16w_fma_hi(w.w, xv[n].w, c1[n]);
                }
            }
        }
        if (last) {
#pragma unroll
            for (int n = 0; n < NT; n++) {
                const float v = wave_sum_lane63(c0[n] + c1[n]);
                if (lane == 63) y[(int64_t)n * ldy + m] = v;
                c0[n] = c1[n] = 0.0f;
            }
        }
#pragma unroll
        for (int u = 0; u < F16W_DEPTH; u++) cur[u] = nxt[u];
        m = nm;
        s0 = ns0;
    }
}

template <int NT, bool NTL>
static hipError_t launch_gemv_f16w(const uint16_t *W, int K, int M, const float *x, float *y, int64_t ldy, int num_cus,
                                   hipStream_t s) {
    const size_t lds = (size_t)NT * (size_t)K * 2;
    const hipError_t e = raise_dynamic_lds<k_gemv_f16w<NT, NTL>>(F16W_LDS_MAX);
    if (e != hipSuccess) return e;
    // workgroups a CU holds: 2048 threads, 160 KB of LDS
    const int per_cu = lds > 80 * 1024 ? 1 : 2;
    const int64_t want = ((int64_t)M + F16W_WAVES - 1) / F16W_WAVES;
    const int64_t cap = (int64_t)(num_cus > 0 ? num_cus : 256) * per_cu;
    (void)hipGetLastError();  // report only this launch's error
    launch_k(k_gemv_f16w<NT, NTL>, dim3((unsigned)(want < cap ? want : cap)), dim3(F16W_WAVES * 64), lds, s, W, K, M, x, y,
             ldy);
    return hipGetLastError();
}

// any N: column tiles of gemv_f16w_max_tokens(K) through the same kernel (each tile is exactly the call on those
// columns)
hipError_t gemv_f16w(const void *W, int64_t K, int64_t M, const float *x, int64_t N, float *y, int64_t ldy,
                     const DeviceInfo &dev, hipStream_t s) {
    const int tile = gemv_f16w_max_tokens(K);
    if (tile < 1 || M < 1 || M >= ((int64_t)1 << 31)) return hipErrorInvalidValue;
    const bool nt = f16w_nt();
    return for_column_tiles(N, tile, [&](int64_t n0, int ntok) {
        return with_token_tile(ntok, [&](auto NT) {
            constexpr int T = decltype(NT)::value;
            return nt ? launch_gemv_f16w<T, true>((const uint16_t *)W, (int)K, (int)M, x + n0 * K, y + n0 * ldy, ldy,
                                                  dev.num_cus, s)
                      : launch_gemv_f16w<T, false>((const uint16_t *)W, (int)K, (int)M, x + n0 * K, y + n0 * ldy, ldy,
                                                   dev.num_cus, s);
        });
    });
}

}  // namespace ghip
