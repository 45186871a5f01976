// f32_w.hip — F32 WEIGHTS x F32 mul_mat at decode and small batches, and in exact mode (gfx950, wave64): the layer
// matrices of the "all F32" files (ftype 0), which the reference's GPU backend serves like every other src0 type.
//
//   k_gemv_f32w<NT>   y[n][m] = sum_e W[m][e] * x[n][e] for NT <= 8 tokens, W contiguous F32 rows, x F32:
//                     ggml_compute_forward_mul_mat_f32 (ggml.c:10855).  No operand is rounded, every product enters by
//                     an fmaf (one rounding), fp32 subnormals are kept; only the order of the additions is this
//                     kernel's own, so y is within the fp32-accumulation bound of the reference, not bitwise.
//   k_mm_exact_f32w   the same product in ggml_vec_dot_f32's AVX2 + FMA schedule (ggml.c:2266, GGML_F32_STEP 32,
//                     GGML_F32_EPR 8), bit for bit: any N, any K % 32 == 0, any ldy >= M.
//
// Arithmetic: fmaf on the f32 operands (-ffp-contract=off, so nothing else is contracted), nothing is converted.
//
// THE GEMV'S ORDER (it depends on K alone; tests/f32w_ref.py gemv_schedule restates it in numpy): a row is walked in
// steps of 256 elements, step s = elements 256 s .. 256 s + 255.  Lane l of the row's wave owns the 4 elements
// 256 s + 4 l .. + 3 of every step (one 16-byte load) and keeps two fp32 chains per token, both starting at +0:
//     chain 0:  c0 = fmaf(w[e], x[e], c0)  for e = 256 s + 4 l + 0, 2
//     chain 1:  c1 = fmaf(w[e], x[e], c1)  for e = 256 s + 4 l + 1, 3
// in that order within a step, steps in increasing s.  In the last step of a K that is no multiple of 256 the lanes
// with 256 s + 4 l >= K add nothing (K % 32 == 0, so a lane has all 4 elements or none).  At the row's end
// t_l = c0 + c1 per lane, and the 64 t_l are added as the balanced binary tree over the lanes in order:
// ((t_0 + t_1) + (t_2 + t_3)) + ..., six levels (wave_sum_lane63's DPP steps).  Nothing else enters: not N, not the
// column's place in its tile, not M or the row's place, not the grid or the CU count.
//
// THE EXACT KERNEL'S ORDER is ggml_vec_dot_f32's: 32 chains, chain e % 32 takes element e, sum = fmaf(w[e], x[e], sum)
// in order of e from +0; then GGML_F32x8_REDUCE: the four 8-lane vectors as (v0 + v2) + (v1 + v3), its low half + its
// high half, and (t0 + t1) + (t2 + t3).  32 lanes per output, as ggml_ops.hip's k_mul_mat_f16_f32 (copied, not shared:
// that kernel rounds and widens fp16 operands and carries a double tail, which K % 32 == 0 does not have).
//
// Memory (GEMV): the matrix is streamed once per launch, 16 bytes per lane and load, F32W_DEPTH steps per batch and the
// next batch (of the next row after a row's last) in flight while the current one is consumed; loads at clamped
// indices, always inside the matrix, so none sits under a branch and no byte outside W is read.  The NT x columns
// are copied once per workgroup into LDS ([NT][K] floats, the first batch of weight loads already in flight) and read
// with ds_read_b128: x is read NT times per weight row, which the LDS carries and the vector cache would not.  4 NT K
// bytes of LDS bound the tile: gemv_f32w_max_tokens(K) = min(8, 128 KiB / 4 K): 8 columns up to K = 4096, 2 at
// K = 11008, none past K = 32768 (auto runs the exact kernel there).
#include "q4_0_device.h"

namespace ghip {

static constexpr int F32W_WAVES = 16;              // rows in flight per workgroup, one wave each
static constexpr int F32W_DEPTH = 4;               // 256-element steps per batch
static constexpr int F32W_LDS_MAX = 128 * 1024;    // of the x copy

// nontemporal weight loads: on (default) / off, GGML_HIP_F32W_NT.  Measured both ways (tools/f32w_bench.py,
// profiles/f32w.json and f32w_gemv_plain_loads.json): equal on 4096 -> 4096, 2-13 % faster on the larger matrices
static bool f32w_nt() {
    static const bool nt = env_int("GGML_HIP_F32W_NT", 1) != 0;
    return nt;
}

int gemv_f32w_max_tokens(int64_t K) {
    if (K <= 0 || K % 32) return 0;
    const int64_t n = F32W_LDS_MAX / (4 * K);
    return (int)(n > 8 ? 8 : n);
}

template <int NT, bool NTL>
__global__ __launch_bounds__(F32W_WAVES * 64) void k_gemv_f32w(const float *__restrict__ W, int K, int M,
                                                               const float *__restrict__ x, float *__restrict__ y,
                                                               int64_t ldy) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    u32x4 *xs = reinterpret_cast<u32x4 *>(smem);            // [NT][K / 4]: 4 floats per entry
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int K4 = K >> 2;                                  // 16-byte pieces of a row
    const int nsteps = (K + 255) >> 8;
    const int stride = gridDim.x * F32W_WAVES;
    // (unconditional loads at clamped indices, always inside the matrix: a load under a branch would make the
    // compiler wait for every load in flight, the prefetched batch included, before the first use)
    auto load_batch = [&](int m, int s0, u32x4 *r) __attribute__((always_inline)) {
        const u32x4 *row = reinterpret_cast<const u32x4 *>(W + (int64_t)(m < M ? m : M - 1) * K);
#pragma unroll
        for (int u = 0; u < F32W_DEPTH; u++) {
            const int q = (s0 + u) * 64 + lane;
            const u32x4 *p = row + (q < K4 ? q : K4 - 1);
            r[u] = NTL ? __builtin_nontemporal_load(p) : *p;
        }
    };
    int m = blockIdx.x * F32W_WAVES + wave, s0 = 0;
    u32x4 cur[F32W_DEPTH], nxt[F32W_DEPTH];
    load_batch(m, s0, cur);
    // the copy of x: [NT][K] f32, 4 per thread and pass
    for (int i = threadIdx.x; i < NT * K4; i += F32W_WAVES * 64) xs[i] = reinterpret_cast<const u32x4 *>(x)[i];
    __syncthreads();
    float c0[NT], c1[NT];
#pragma unroll
    for (int n = 0; n < NT; n++) c0[n] = c1[n] = 0.0f;
    while (m < M) {                                         // wave-uniform
        const bool last = s0 + F32W_DEPTH >= nsteps;        // of this row
        const int nm = last ? m + stride : m, ns0 = last ? 0 : s0 + F32W_DEPTH;
        load_batch(nm, ns0, nxt);
#pragma unroll
        for (int u = 0; u < F32W_DEPTH; u++) {
            const int q = (s0 + u) * 64 + lane;
            const int qc = q < K4 ? q : K4 - 1;             // the LDS reads clamped too: issued ahead of the branch
            u32x4 xv[NT];
#pragma unroll
            for (int n = 0; n < NT; n++) xv[n] = xs[n * K4 + qc];
            if (q < K4) {                                   // a lane past the row's end (or the row's last step) adds nothing
                const u32x4 w = cur[u];
#pragma unroll
                for (int n = 0; n < NT; n++) {
                    c0[n] = fmaf(__uint_as_float(w.x), __uint_as_float(xv[n].x), c0[n]);
                    c1[n] = fmaf(__uint_as_float(w.y), __uint_as_float(xv[n].y), c1[n]);
                    c0[n] = fmaf(__uint_as_float(w.z), __uint_as_float(xv[n].z), c0[n]);
                    c1[n] = fmaf(__uint_as_float(w.w), __uint_as_float(xv[n].w), c1[n]);
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
        for (int u = 0; u < F32W_DEPTH; u++) cur[u] = nxt[u];
        m = nm;
        s0 = ns0;
    }
}

template <int NT, bool NTL>
static hipError_t launch_gemv_f32w(const float *W, int K, int M, const float *x, float *y, int64_t ldy, int num_cus,
                                   hipStream_t s) {
    const size_t lds = (size_t)NT * (size_t)K * 4;
    const hipError_t e = raise_dynamic_lds<k_gemv_f32w<NT, NTL>>(F32W_LDS_MAX);
    if (e != hipSuccess) return e;
    // workgroups a CU holds: 2048 threads, 160 KB of LDS
    const int per_cu = lds > 80 * 1024 ? 1 : 2;
    const int64_t want = ((int64_t)M + F32W_WAVES - 1) / F32W_WAVES;
    const int64_t cap = (int64_t)(num_cus > 0 ? num_cus : 256) * per_cu;
    (void)hipGetLastError();  // report only this launch's error
    launch_k(k_gemv_f32w<NT, NTL>, dim3((unsigned)(want < cap ? want : cap)), dim3(F32W_WAVES * 64), lds, s, W, K, M, x, y,
             ldy);
    return hipGetLastError();
}

// any N: column tiles of gemv_f32w_max_tokens(K) through the same kernel (each tile is exactly the call on those
// columns)
hipError_t gemv_f32w(const void *W, int64_t K, int64_t M, const float *x, int64_t N, float *y, int64_t ldy,
                     const DeviceInfo &dev, hipStream_t s) {
    const int tile = gemv_f32w_max_tokens(K);
    if (tile < 1 || M < 1 || M >= ((int64_t)1 << 31)) return hipErrorInvalidValue;
    const bool nt = f32w_nt();
    return for_column_tiles(N, tile, [&](int64_t n0, int ntok) {
        return with_token_tile(ntok, [&](auto NT) {
            constexpr int T = decltype(NT)::value;
            return nt ? launch_gemv_f32w<T, true>((const float *)W, (int)K, (int)M, x + n0 * K, y + n0 * ldy, ldy,
                                                  dev.num_cus, s)
                      : launch_gemv_f32w<T, false>((const float *)W, (int)K, (int)M, x + n0 * K, y + n0 * ldy, ldy,
                                                   dev.num_cus, s);
        });
    });
}

// ------------------------------------------------------------------------------------------------ exact
// 32 lanes per output o = n M + m; lane l takes elements l + 32 j in order of j (chain l of the AVX2 loop)
static constexpr int F32W_EX_TPB = 256;

__global__ __launch_bounds__(F32W_EX_TPB) void k_mm_exact_f32w(const float *__restrict__ W, int K, int64_t M,
                                                               const float *__restrict__ x, int64_t nout,
                                                               float *__restrict__ y, int64_t ldy) {
    const int64_t o = ((int64_t)blockIdx.x * F32W_EX_TPB + threadIdx.x) >> 5;   // output index
    const int l = threadIdx.x & 31;
    const bool valid = o < nout;
    const int64_t oc = valid ? o : nout - 1;               // clamped: loaded, not stored
    const int64_t n = oc / M, m = oc - n * M;
    const float *wr = W + m * K, *xr = x + n * K;
    float acc = 0.0f;
    // batches of 4 unconditional loads of clamped addresses (issued back to back), used in order of e
    for (int e0 = 0; e0 < K; e0 += 128) {
        float wb[4], xb[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int e = min(e0 + l + 32 * j, K - 1);
            wb[j] = wr[e];
            xb[j] = xr[e];
        }
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (e0 + l + 32 * j < K) acc = fmaf(wb[j], xb[j], acc);
    }
    // lane = 8 j + i: GGML_F32x8_REDUCE
    const float a = acc + __shfl_xor(acc, 16, 32);          // lanes 0-7: v0 + v2, 8-15: v1 + v3
    const float c = a + __shfl_xor(a, 8, 32);               // lanes 0-7: (v0 + v2) + (v1 + v3)
    const float t0 = c + __shfl_xor(c, 4, 32);              // lanes 0-3: c_i + c_{i + 4}
    const float t01 = t0 + __shfl_xor(t0, 1, 32);           // lane 0: t0_0 + t0_1, lane 2: t0_2 + t0_3
    const float res = t01 + __shfl(t01, 2, 32);             // lane 0
    if (l == 0 && valid) y[n * ldy + m] = res;
}

hipError_t mm_exact_f32w(const void *W, int64_t K, int64_t M, const float *x, int64_t N, float *y, int64_t ldy,
                         hipStream_t s) {
    if (K <= 0 || K % 32 || M < 1 || N < 1 || K >= ((int64_t)1 << 31)) return hipErrorInvalidValue;
    const int64_t nout = N * M, blocks = (nout * 32 + F32W_EX_TPB - 1) / F32W_EX_TPB;
    if (blocks >= ((int64_t)1 << 31)) return hipErrorInvalidValue;
    (void)hipGetLastError();  // report only this launch's error
    launch_k(k_mm_exact_f32w, dim3((unsigned)blocks), dim3(F32W_EX_TPB), 0, s, (const float *)W, (int)K, M, x, nout, y, ldy);
    return hipGetLastError();
}

}  // namespace ghip
