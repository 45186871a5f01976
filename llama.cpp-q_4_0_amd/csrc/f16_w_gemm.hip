// f16_w_gemm.hip — F16 WEIGHTS x F32 mul_mat at prefill (gfx950, wave64): algo 11 of ggml_hip_mul_mat_f16, the GEMM
// decomposed for weight shapes (f16_w.hip is the GEMV; ggml_ops.hip's k_mul_mat_f16_f32_mfma, algo 9, is the
// attention's kernel: 64 x 128 tiles, 32-element chunks, no K split, 32 workgroups on a 4096-row matrix at N <= 64).
//
//   y[n][m] = sum_e W[m][e] * fp16(x[n][e])        ggml_compute_forward_mul_mat_f16_f32: x rounded to fp16 first (round
//   to nearest even, q4_0_device.h f2h, the GEMV's function), exact products of two fp16 values, fp32 sums in an order of
//   this file's own: y is within the fp32-accumulation bound of the reference, not bitwise it and not bitwise the GEMV.
//
// Three launches at most, all plain kernels (nothing to zero, no counter, no workgroup waits for another):
//   k_f16w_ximage   the fp16 image of x, [N][K] halves, once per call into the workspace: both operands are then K-
//                   contiguous fp16 rows and stage the same way
//   k_gemm_f16w     v_mfma_f32_32x32x16_f16, A = 32 tokens, B = 32 weight rows (so a register of the result is 32
//                   consecutive m of one token: one coalesced store).  256 threads; a workgroup owns BM weight rows x BN
//                   tokens x one of KS slices of K.  K runs in chunks of 64 elements through two LDS buffers (one array,
//                   rows of 64 halves at a pitch of 72: the ds_read_b128 of 32 rows 144 bytes apart), the next chunk's
//                   global loads in flight while this chunk's MFMAs run, one barrier per chunk.  Every global load is a
//                   16-byte piece of a row, 8 lanes per 128-byte line, at a clamped index (row < M / N, piece inside the
//                   row), so no byte outside W or the image is read; a piece past K is replaced by zeros on its way
//                   into the LDS and adds exact zeros; rows past M / N compute outputs that are never stored.
//   k_f16w_slabs    plans with KS > 1 write one fp32 slab [N][M] per slice into the workspace and this kernel adds
//                   them in increasing slice order, ((s0 + s1) + s2) + s3, into y (no atomics on y)
//
// THE PLANS (a plan = BM x BN tile, the split of a chunk over the waves, KS; chosen as a pure function of K, M, N and
// the CU count, gemm_f16w_plan):
//   1  32 x 64, the four waves split every 64-element chunk into its four 16-element MFMA steps (wave w takes elements
//      16 w .. 16 w + 15 of every chunk) and are added through the LDS in wave order ((w0 + w1) + w2) + w3; KS = 4.
//      128 row tiles x 4 slices = 512 workgroups on a 4096-row matrix: what fills the device at N <= 64.
//   2  64 x 128, waves 2 (m) x 2 (n) of 32 x 64 each, every wave walks all four steps of a chunk; KS = 2
//   3  128 x 128, waves 2 x 2 of 64 x 64 each; KS = 1 (y written directly)
//
// THE ORDER of one output's additions is a function of K and of the plan and of nothing else: slice s of KS covers the
// chunks [s cps, (s + 1) cps) with cps = ceil(ceil(K / 64) / KS); within a slice one accumulator per (wave-)step
// sequence is chained through the MFMAs in increasing K, each MFMA adding its 16 products in the instruction's own
// fixed order; then the wave sum of plan 1 and the slice sum, both in index order.  Not N, not the column's or the row's
// place in its tile or in the matrix, not M, not whether neighbours are ragged padding (an MFMA's output element
// depends on its own A row and B column only), not the grid or the CU count.  With the plan pinned a column slice or a
// row slice of a call is bitwise the call on that slice.
//
// Relied on and not stated by the hardware guides at hand: v_mfma_f32_32x32x16_f16 takes fp16 SUBNORMAL inputs at their
// value (it does not flush them) and forms each product exactly.  The guides speak of f32 inputs (MODE.denorm) and of
// C / D only.  Algo 9 relies on the same; tests/test_gpu_f16w.py and tests/test_gpu_f16w_gemm.py hold both against the
// float64 sum of the exact products on inputs with fp16 subnormals, where a flush would show.
#include <atomic>

#include "q4_0_device.h"

namespace ghip {

typedef _Float16 f16w_h8 __attribute__((ext_vector_type(8)));
typedef float f16w_f16 __attribute__((ext_vector_type(16)));

static constexpr int WG_KC = 64;                    // K chunk, elements
static constexpr int WG_PITCH = WG_KC + 8;          // LDS row pitch, halves (144 bytes)
static constexpr int WG_THREADS = 256;

struct WgPlan {
    int bm, bn, ks;
};
static constexpr WgPlan WG_PLANS[F16W_WGEMM_PLANS] = {{32, 64, 4}, {64, 128, 2}, {128, 128, 1}};

static std::atomic<int> g_wg_plan{0};               // 0 auto, k >= 1 pinned

int gemm_f16w_set_plan(int plan) {
    if (plan < 0 || plan > F16W_WGEMM_PLANS) plan = 0;
    return g_wg_plan.exchange(plan, std::memory_order_relaxed);
}

// The rule: the largest tile whose grid covers the CUs, held against the per-plan sweep of tools/f16w_bench.py
// (profiles/f16w_wgemm.json: the plan it names is the fastest of the three in every cell of the three LLaMA-7B layer
// shapes and the lm_head, N = 9 .. 512).  At N <= 64 plan 1 as long as its 32-row tiles without the K split are fewer
// than two per CU (the split is what fills the device there: 128 / 344 row tiles on the layer shapes; on the lm_head's
// 1000 it only adds slab traffic, 99 against 80 us).  Else plan 3 where its 128 x 128 tiles are at least three quarters
// of the CUs (the lm_head at N <= 128 has 250 on 256 CUs: 89 against plan 2's 100 us; the layer shapes where plan 2
// wins have at most half), else plan 2 where its 64 x 128 tiles x 2 slices cover the CUs, else plan 1.
int gemm_f16w_plan(int64_t K, int64_t M, int64_t N, int num_cus) {
    const int pin = g_wg_plan.load(std::memory_order_relaxed);
    return pin ? pin : gemm_f16w_auto_plan(K, M, N, num_cus);
}
int gemm_f16w_auto_plan(int64_t K, int64_t M, int64_t N, int num_cus) {
    (void)K;
    const int64_t cus = num_cus > 0 ? num_cus : 256;
    auto wgs = [&](const WgPlan &p) { return ((M + p.bm - 1) / p.bm) * ((N + p.bn - 1) / p.bn) * p.ks; };
    if (N <= 64 && (M + 31) / 32 < 2 * cus) return 1;
    if (4 * wgs(WG_PLANS[2]) >= 3 * cus) return 3;
    if (wgs(WG_PLANS[1]) >= cus) return 2;
    return 1;
}

// one launch's grid under every plan (plan 1 has the most workgroups)
bool gemm_f16w_supported(int64_t K, int64_t M, int64_t N) {
    if (K <= 0 || K % 32 || M < 1 || N < 1 || M >= ((int64_t)1 << 31) || N * K >= ((int64_t)1 << 31)) return false;
    const WgPlan &p = WG_PLANS[0];
    return ((M + p.bm - 1) / p.bm) * ((N + p.bn - 1) / p.bn) * p.ks < ((int64_t)1 << 31) &&
           (M * N + WG_THREADS - 1) / WG_THREADS < ((int64_t)1 << 31);
}

static size_t wg_ximage_bytes(int64_t K, int64_t N) { return ((size_t)N * (size_t)K * 2 + 255) & ~(size_t)255; }

// the x image, and the slabs of the plan the call would run now
size_t gemm_f16w_ws_bytes(int64_t K, int64_t M, int64_t N, int num_cus) {
    if (K <= 0 || M < 1 || N < 1) return 0;
    const WgPlan &p = WG_PLANS[gemm_f16w_plan(K, M, N, num_cus) - 1];
    return wg_ximage_bytes(K, N) + (p.ks > 1 ? (size_t)p.ks * (size_t)N * (size_t)M * 4 : 0);
}

// [N][K] f32 -> [N][K] halves, 8 per thread
__global__ __launch_bounds__(WG_THREADS) void k_f16w_ximage(const float *__restrict__ x, u32x4 *__restrict__ xh, int64_t n8) {
    const int64_t i = (int64_t)blockIdx.x * WG_THREADS + threadIdx.x;
    if (i >= n8) return;
    const float4 a = reinterpret_cast<const float4 *>(x)[2 * i], b = reinterpret_cast<const float4 *>(x)[2 * i + 1];
    u32x4 h;
    h.x = f2h(a.x) | (f2h(a.y) << 16);
    h.y = f2h(a.z) | (f2h(a.w) << 16);
    h.z = f2h(b.x) | (f2h(b.y) << 16);
    h.w = f2h(b.z) | (f2h(b.w) << 16);
    xh[i] = h;
}

// y[n * ldy + m] = ((slab 0 + slab 1) + slab 2) + ...
template <int KS>
__global__ __launch_bounds__(WG_THREADS) void k_f16w_slabs(const float *__restrict__ slabs, int64_t M, int64_t NM,
                                                           float *__restrict__ y, int64_t ldy) {
    const int64_t i = (int64_t)blockIdx.x * WG_THREADS + threadIdx.x;
    if (i >= NM) return;
    float v = slabs[i];
#pragma unroll
    for (int s = 1; s < KS; s++) v += slabs[(int64_t)s * NM + i];
    const int64_t n = i / M;
    y[n * ldy + (i - n * M)] = v;
}

// BM weight rows x BN tokens; waves WK (split of a chunk's four steps) x WM x WN, WK WM WN = 4.  out: y (KS = 1, pitch
// ldo = ldy) or the slabs (pitch M, slice stride N M).  Grid: token tiles fastest (the workgroups that share weight
// rows run together), then row tiles, then slices.
template <int BM, int BN, int WK, int WM, int WN, int KS>
__global__ __launch_bounds__(WG_THREADS) void k_gemm_f16w(const uint16_t *__restrict__ W, const uint16_t *__restrict__ xh,
                                                          int K, int M, int N, float *__restrict__ out, int64_t ldo,
                                                          int64_t slice_stride, int ntn, int ntm) {
    static_assert(WK * WM * WN == 4 && (WK == 1 || WK == 4), "four waves");
    constexpr int TM = BM / WM, TN = BN / WN;              // a wave's tile
    constexpr int RM = TM / 32, RN = TN / 32;              // in 32 x 32 MFMA blocks
    static_assert(RM >= 1 && RN >= 1 && RM * 32 * WM == BM && RN * 32 * WN == BN, "tiles of 32 x 32 blocks");
    constexpr int PIECES = (BM + BN) * (WG_KC / 8);        // 16-byte pieces of a chunk: the x tile, then the W tile
    static_assert(PIECES % WG_THREADS == 0 && (BN * (WG_KC / 8)) % WG_THREADS == 0, "whole staging passes per operand");
    constexpr int NP = PIECES / WG_THREADS, NPX = BN * (WG_KC / 8) / WG_THREADS;
    constexpr int BUF = (BM + BN) * WG_PITCH;              // halves per buffer
    static_assert(WK == 1 || (WK - 1) * RM * RN * 16 * 64 * 4 <= 2 * BUF * 2, "the wave sums fit the staging buffers");
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint16_t *lds = reinterpret_cast<uint16_t *>(smem);    // [2][BN + BM][WG_PITCH]: token rows, then weight rows

    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int rl = lane & 31, kh = lane >> 5;
    int b = blockIdx.x;
    const int tn = b % ntn;
    b /= ntn;
    const int tm = b % ntm, kz = b / ntm;
    const int64_t m0 = (int64_t)tm * BM, n0 = (int64_t)tn * BN;
    const int K8 = K >> 3;
    const int nchunks = (K + WG_KC - 1) / WG_KC, cps = (nchunks + KS - 1) / KS;
    const int c0 = kz * cps, c1 = c0 + cps < nchunks ? c0 + cps : nchunks;      // this slice's chunks (may be none)

    // staging roles: pass i moves piece p = t + 256 i = row p / 8, 16-byte column p % 8; rows past the matrix clamped
    const u32x4 *src[NP];
    int dst[NP];
    const int pc = t & 7;
#pragma unroll
    for (int i = 0; i < NP; i++) {
        const int row = (t >> 3) + i * (WG_THREADS / 8);   // in [0, BN + BM)
        if (i < NPX) {
            const int64_t n = n0 + row < N ? n0 + row : N - 1;
            src[i] = reinterpret_cast<const u32x4 *>(xh + n * K);
        } else {
            const int64_t m = m0 + (row - BN) < M ? m0 + (row - BN) : M - 1;
            src[i] = reinterpret_cast<const u32x4 *>(W + m * K);
        }
        dst[i] = row * WG_PITCH + pc * 8;
    }
    u32x4 g[NP];
    auto gload = [&](int c) __attribute__((always_inline)) {
        const int q = c * (WG_KC / 8) + pc;
        const int qc = q < K8 ? q : K8 - 1;                // always inside the row
#pragma unroll
        for (int i = 0; i < NP; i++) g[i] = src[i][qc];
    };
    auto lstore = [&](int c, int buf) __attribute__((always_inline)) {
        const bool in = c * (WG_KC / 8) + pc < K8;         // a piece past K: zeros
#pragma unroll
        for (int i = 0; i < NP; i++) {
            u32x4 v = g[i];
            if (!in) v = u32x4{0, 0, 0, 0};
            *reinterpret_cast<u32x4 *>(lds + buf * BUF + dst[i]) = v;
        }
    };

    const int wk = WK == 4 ? wave : 0;
    const int wn = WK == 4 ? 0 : (wave & (WN - 1)), wm = WK == 4 ? 0 : wave / WN;
    const int arow = wn * TN + rl;                         // this lane's token row of the first A block
    const int brow = BN + wm * TM + rl;                    // and weight row of the first B block
    f16w_f16 acc[RN][RM];
#pragma unroll
    for (int a = 0; a < RN; a++)
#pragma unroll
        for (int r = 0; r < RM; r++) acc[a][r] = f16w_f16{};

    if (c0 < c1) {
        gload(c0);
        lstore(c0, 0);
    }
    __syncthreads();
    for (int c = c0; c < c1; c++) {
        const int buf = (c - c0) & 1;
        const bool more = c + 1 < c1;                      // workgroup-uniform
        if (more) gload(c + 1);
        const uint16_t *L = lds + buf * BUF;
#pragma unroll
        for (int st = 0; st < (WK == 4 ? 1 : 4); st++) {
            const int ko = 16 * (WK == 4 ? wk : st) + 8 * kh;
            f16w_h8 fa[RN], fb[RM];
#pragma unroll
            for (int a = 0; a < RN; a++) fa[a] = *reinterpret_cast<const f16w_h8 *>(L + (arow + 32 * a) * WG_PITCH + ko);
#pragma unroll
            for (int r = 0; r < RM; r++) fb[r] = *reinterpret_cast<const f16w_h8 *>(L + (brow + 32 * r) * WG_PITCH + ko);
#pragma unroll
            for (int a = 0; a < RN; a++)
#pragma unroll
                for (int r = 0; r < RM; r++)
                    acc[a][r] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[a], fb[r], acc[a][r], 0, 0, 0);
        }
        if (more) lstore(c + 1, buf ^ 1);
        __syncthreads();
    }

    if constexpr (WK == 4) {
        // the four waves' sums of the same tile: waves 1 .. 3 park theirs in the LDS (every read of the staging
        // buffers is behind the loop's last barrier), wave 0 adds them in wave order
        float *red = reinterpret_cast<float *>(smem);      // [3][RN * RM * 16][64]
        if (wave > 0) {
#pragma unroll
            for (int a = 0; a < RN; a++)
#pragma unroll
                for (int r = 0; r < RM; r++)
#pragma unroll
                    for (int e = 0; e < 16; e++)
                        red[(((wave - 1) * RN * RM + a * RM + r) * 16 + e) * 64 + lane] = acc[a][r][e];
        }
        __syncthreads();
        if (wave > 0) return;
#pragma unroll
        for (int w = 1; w < 4; w++)
#pragma unroll
            for (int a = 0; a < RN; a++)
#pragma unroll
                for (int r = 0; r < RM; r++)
#pragma unroll
                    for (int e = 0; e < 16; e++)
                        acc[a][r][e] += red[(((w - 1) * RN * RM + a * RM + r) * 16 + e) * 64 + lane];
    }

    // acc[a][r][e] = D[token n0 + wn TN + 32 a + (e & 3) + 8 (e >> 2) + 4 kh][row m0 + wm TM + 32 r + rl]
    float *o = out + (int64_t)kz * slice_stride;
#pragma unroll
    for (int a = 0; a < RN; a++)
#pragma unroll
        for (int e = 0; e < 16; e++) {
            const int64_t n = n0 + wn * TN + 32 * a + (e & 3) + 8 * (e >> 2) + 4 * kh;
            if (n >= N) continue;
#pragma unroll
            for (int r = 0; r < RM; r++) {
                const int64_t m = m0 + wm * TM + 32 * r + rl;
                if (m < M) o[n * ldo + m] = acc[a][r][e];
            }
        }
}

template <int BM, int BN, int WK, int WM, int WN, int KS>
static hipError_t launch_gemm_f16w(const uint16_t *W, const uint16_t *xh, int64_t K, int64_t M, int64_t N, float *y,
                                   int64_t ldy, float *slabs, hipStream_t s) {
    constexpr int lds = 2 * (BM + BN) * WG_PITCH * 2;
    if (const hipError_t e = raise_dynamic_lds<k_gemm_f16w<BM, BN, WK, WM, WN, KS>>(lds); e != hipSuccess) return e;
    const int64_t ntn = (N + BN - 1) / BN, ntm = (M + BM - 1) / BM;
    (void)hipGetLastError();  // report only these launches' error
    launch_k(k_gemm_f16w<BM, BN, WK, WM, WN, KS>, dim3((unsigned)(ntn * ntm * KS)), dim3(WG_THREADS), (size_t)lds, s, W, xh,
             (int)K, (int)M, (int)N, KS > 1 ? slabs : y, KS > 1 ? M : ldy, KS > 1 ? N * M : (int64_t)0, (int)ntn, (int)ntm);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    if constexpr (KS > 1) {
        launch_k(k_f16w_slabs<KS>, dim3((unsigned)((N * M + WG_THREADS - 1) / WG_THREADS)), dim3(WG_THREADS), 0, s,
                 (const float *)slabs, M, N * M, y, ldy);
        return hipGetLastError();
    }
    return hipSuccess;
}

// ws: ws_bytes >= gemm_f16w_ws_bytes(K, M, N, dev.num_cus) bytes, 16-byte aligned (checked against the plan that
// runs: a pin that changed since the sizing cannot write past the workspace)
hipError_t gemm_f16w(const void *W, int64_t K, int64_t M, const float *x, int64_t N, float *y, int64_t ldy, void *ws,
                     size_t ws_bytes, const DeviceInfo &dev, hipStream_t s) {
    if (!gemm_f16w_supported(K, M, N) || !ws) return hipErrorInvalidValue;
    const int plan = gemm_f16w_plan(K, M, N, dev.num_cus);
    const size_t need = wg_ximage_bytes(K, N) + (WG_PLANS[plan - 1].ks > 1 ? (size_t)WG_PLANS[plan - 1].ks * N * M * 4 : 0);
    if (ws_bytes < need) return hipErrorInvalidValue;
    uint16_t *xh = (uint16_t *)ws;
    float *slabs = (float *)((char *)ws + wg_ximage_bytes(K, N));
    const int64_t n8 = N * K / 8;
    if (const hipError_t e = launch_1d(k_f16w_ximage, n8, WG_THREADS, s, x, (u32x4 *)xh, n8); e != hipSuccess) return e;
    const uint16_t *w = (const uint16_t *)W;
    switch (plan) {
        case 1: return launch_gemm_f16w<32, 64, 4, 1, 1, 4>(w, xh, K, M, N, y, ldy, slabs, s);
        case 2: return launch_gemm_f16w<64, 128, 1, 2, 2, 2>(w, xh, K, M, N, y, ldy, slabs, s);
        default: return launch_gemm_f16w<128, 128, 1, 2, 2, 1>(w, xh, K, M, N, y, ldy, slabs, s);
    }
}

}  // namespace ghip
