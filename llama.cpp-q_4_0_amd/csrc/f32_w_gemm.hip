// f32_w_gemm.hip — F32 WEIGHTS x F32 mul_mat at prefill (gfx950, wave64): algo 12 of ggml_hip_mul_mat_f32, an LDS-tiled
// GEMM on v_mfma_f32_32x32x2_f32 (f32_w.hip has the GEMV and the exact kernel).
//
//   y[n][m] = sum_e W[m][e] * x[n][e]      ggml_compute_forward_mul_mat_f32: no operand is rounded, one rounding per
//   product.  The f32-input MFMA is bit for bit a k-ordered fmaf chain on its C input (subnormals kept), so the order
//   below is the whole result: y is within the fp32-accumulation bound of the reference and bitwise
//   tests/f32w_ref.py gemm_schedule.
//
// W and x are read as f32 straight from global memory: no image of either operand is built, nothing is registered.
// Two launches at most, both plain kernels (nothing to zero, no counter, no workgroup waits for another):
//   k_gemm_f32w     A = 32 tokens, B = 32 weight rows (so a register of the result is 32 consecutive m of one token: one
//                   coalesced store).  256 threads, four waves; a workgroup owns 128 weight rows x BN tokens x one of S
//                   slices of K.  K runs in chunks of 32 elements through two LDS buffers (rows of 32 floats at a pitch
//                   of 36), the next chunk's global loads in flight while this chunk's MFMAs run, one barrier per
//                   chunk.  Every global load is a 16-byte piece of a row, 8 lanes per 128-byte line, at a clamped row
//                   (row < M / N) inside the slice, so no byte outside W's 4 M K or x's 4 N K is read; rows past M / N
//                   compute outputs that are never stored.
//   k_f32w_slabs    with S > 1 every slice writes one fp32 slab [N][M] into the workspace and this kernel adds them in
//                   increasing slice order, ((s0 + s1) + s2) + s3, into y (no atomics on y)
//
// THE TILES (chosen as a pure function of M, N and the CU count; they do NOT enter the result): 128 x 32 (waves 4 x 1,
// one 32 x 32 block each), 128 x 64 (waves 2 x 2 of 64 x 32) and 128 x 128 (waves 2 x 2 of 64 x 64).
//
// THE ORDER of one output's additions is a function of K and S and of nothing else.  S in {1, 2, 4} equal slices,
// slice s = elements [s K / S, (s + 1) K / S); a slice is a whole number of 32-element chunks, so a requested S runs
// as the largest S' <= S of {4, 2, 1} with K % (32 S') == 0 (gemm_f32w_ksplit returns the S' that runs).  Within a
// slice ONE accumulator per output is carried through every MFMA of the slice, which is the sequential chain
//     acc = fmaf(w[e], x[e], acc)   for e = s K / S, s K / S + 1, ... in natural order, starting at +0
// (MFMA step t of a chunk feeds element 2 t from lanes 0-31 and 2 t + 1 from lanes 32-63, and the instruction adds k = 0
// before k = 1).  S = 1 stores the chain's value; S > 1 stores ((a_0 + a_1) + a_2) + a_3 of the slices' values.
// Not N, not the column's or the row's place in its tile or in the matrix, not M, not the tile, not whether neighbours
// are ragged padding (an MFMA's output element depends on its own A row and B column only), not the grid.  Auto S is a
// pure function of (K, M, N, CU count) and can be pinned; with S pinned a column slice or a row slice of a call is
// bitwise the call on that slice.
#include <atomic>

#include "q4_0_device.h"

namespace ghip {

typedef float f32w_f16 __attribute__((ext_vector_type(16)));

static constexpr int FG_KC = 32;                    // K chunk, elements
static constexpr int FG_PITCH = FG_KC + 4;          // LDS row pitch, floats (144 bytes: 16-byte rows)
static constexpr int FG_THREADS = 256;
static constexpr int FG_BM = 128;

static std::atomic<int> g_fg_ksplit{0};             // 0 auto, else 1 / 2 / 4 requested

int gemm_f32w_set_ksplit(int s) {
    if (s != 1 && s != 2 && s != 4) s = 0;
    return g_fg_ksplit.exchange(s, std::memory_order_relaxed);
}

// the token tile: 32 up to N = 32, 64 up to N = 64 and wherever the 128 x 128 tiles alone would not cover the CUs
static int fg_bn(int64_t M, int64_t N, int num_cus) {
    const int64_t cus = num_cus > 0 ? num_cus : 256;
    if (N <= 32) return 32;
    if (N <= 64) return 64;
    return ((M + FG_BM - 1) / FG_BM) * ((N + 127) / 128) >= cus ? 128 : 64;
}

static int fg_fit(int64_t K, int s) {               // the largest S' <= s with whole chunks per slice
    while (s > 1 && K % (FG_KC * s)) s >>= 1;
    return s;
}

// auto, held against the per-split sweep of tools/f32w_bench.py (profiles/f32w.json): the S with the fewest rounds of
// workgroups per slice length, ceil(tiles S / CUs) / S (a 128-row tile's time is its MFMAs, so 344 tiles on 256 CUs
// take two rounds unsplit and three half rounds at S = 2).  Among equals the largest S whose grid is still resident at
// once, tiles S <= 2 CUs (more loads in flight where the weight stream bounds the time: 86 tiles run S = 4), else the
// smallest (no slab traffic for nothing).  Slices of at least 8 chunks.
int gemm_f32w_auto_ksplit(int64_t K, int64_t M, int64_t N, int num_cus) {
    const int64_t cus = num_cus > 0 ? num_cus : 256;
    const int bn = fg_bn(M, N, num_cus);
    const int64_t tiles = ((M + FG_BM - 1) / FG_BM) * ((N + bn - 1) / bn);
    int best = 1;
    int64_t best_cost = 0;
    for (int s = 1; s <= 4; s <<= 1) {
        if (s > 1 && K / s < 8 * FG_KC) break;
        const int64_t cost = (tiles * s + cus - 1) / cus * (4 / s);      // 4 x rounds / S
        if (s == 1 || cost < best_cost || (cost == best_cost && tiles * s <= 2 * cus)) best = s, best_cost = cost;
    }
    return fg_fit(K, best);
}
int gemm_f32w_ksplit(int64_t K, int64_t M, int64_t N, int num_cus) {
    const int pin = g_fg_ksplit.load(std::memory_order_relaxed);
    return pin ? fg_fit(K, pin) : gemm_f32w_auto_ksplit(K, M, N, num_cus);
}

// one launch's grid under every tile (token tiles on grid.y)
bool gemm_f32w_supported(int64_t K, int64_t M, int64_t N) {
    return K > 0 && K % 32 == 0 && M >= 1 && N >= 1 && M < ((int64_t)1 << 31) && N * K < ((int64_t)1 << 31) &&
           (N + 31) / 32 <= 65535 && (M * N + FG_THREADS - 1) / FG_THREADS < ((int64_t)1 << 31);
}

// the slabs of the S the call would run now
size_t gemm_f32w_ws_bytes(int64_t K, int64_t M, int64_t N, int num_cus) {
    if (K <= 0 || K % 32 || M < 1 || N < 1) return 0;
    const int s = gemm_f32w_ksplit(K, M, N, num_cus);
    return s > 1 ? (size_t)s * (size_t)N * (size_t)M * 4 : 0;
}

// y[n * ldy + m] = ((slab 0 + slab 1) + slab 2) + slab 3
__global__ __launch_bounds__(FG_THREADS) void k_f32w_slabs(const float *__restrict__ slabs, int S, int64_t M, int64_t NM,
                                                           float *__restrict__ y, int64_t ldy) {
    const int64_t i = (int64_t)blockIdx.x * FG_THREADS + threadIdx.x;
    if (i >= NM) return;
    float v = slabs[i];
    for (int s = 1; s < S; s++) v += slabs[(int64_t)s * NM + i];
    const int64_t n = i / M;
    y[n * ldy + (i - n * M)] = v;
}

// 128 weight rows x BN tokens; waves WM x WN.  out: y (S = 1, pitch ldo = ldy) or the slabs (pitch M, slice stride N M).
// Grid: x = row tiles, y = token tiles, z = slices.  kslice = K / S elements, a multiple of 32.
template <int BN, int WM, int WN>
__global__ __launch_bounds__(FG_THREADS) void k_gemm_f32w(const float *__restrict__ W, const float *__restrict__ x, int K,
                                                          int M, int N, int kslice, float *__restrict__ out, int64_t ldo,
                                                          int64_t slice_stride) {
    static_assert(WM * WN == 4, "four waves");
    constexpr int BM = FG_BM;
    constexpr int TM = BM / WM, TN = BN / WN;              // a wave's tile
    constexpr int RM = TM / 32, RN = TN / 32;              // in 32 x 32 MFMA blocks
    static_assert(RM >= 1 && RN >= 1 && RM * 32 * WM == BM && RN * 32 * WN == BN, "tiles of 32 x 32 blocks");
    constexpr int PIECES = (BM + BN) * (FG_KC / 4);        // 16-byte pieces of a chunk: the x tile, then the W tile
    static_assert(PIECES % FG_THREADS == 0 && (BN * (FG_KC / 4)) % FG_THREADS == 0, "whole staging passes per operand");
    constexpr int NP = PIECES / FG_THREADS, NPX = BN * (FG_KC / 4) / FG_THREADS;
    constexpr int BUF = (BM + BN) * FG_PITCH;              // floats per buffer
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    float *lds = reinterpret_cast<float *>(smem);          // [2][BN + BM][FG_PITCH]: token rows, then weight rows

    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int rl = lane & 31, kh = lane >> 5;
    const int64_t m0 = (int64_t)blockIdx.x * BM, n0 = (int64_t)blockIdx.y * BN;
    const int kz = blockIdx.z;
    const int nchunks = kslice / FG_KC;                    // >= 1
    const int64_t k0 = (int64_t)kz * kslice;

    // staging roles: pass i moves piece p = t + 256 i = row p / 8, 16-byte column p % 8; rows past the matrix clamped
    const u32x4 *src[NP];
    int dst[NP];
    const int pc = t & 7;
#pragma unroll
    for (int i = 0; i < NP; i++) {
        const int row = (t >> 3) + i * (FG_THREADS / 8);   // in [0, BN + BM)
        if (i < NPX) {
            const int64_t n = n0 + row < N ? n0 + row : N - 1;
            src[i] = reinterpret_cast<const u32x4 *>(x + n * K + k0) + pc;
        } else {
            const int64_t m = m0 + (row - BN) < M ? m0 + (row - BN) : M - 1;
            src[i] = reinterpret_cast<const u32x4 *>(W + m * K + k0) + pc;
        }
        dst[i] = row * FG_PITCH + pc * 4;
    }
    u32x4 g[NP];
    auto gload = [&](int c) __attribute__((always_inline)) {        // c < nchunks: inside the slice, inside the row
#pragma unroll
        for (int i = 0; i < NP; i++) g[i] = src[i][c * (FG_KC / 4)];
    };
    auto lstore = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < NP; i++) *reinterpret_cast<u32x4 *>(lds + buf * BUF + dst[i]) = g[i];
    };

    const int wn = wave % WN, wm = wave / WN;
    const int arow = wn * TN + rl;                         // this lane's token row of the first A block
    const int brow = BN + wm * TM + rl;                    // and weight row of the first B block
    f32w_f16 acc[RN][RM];
#pragma unroll
    for (int a = 0; a < RN; a++)
#pragma unroll
        for (int r = 0; r < RM; r++) acc[a][r] = f32w_f16{};

    gload(0);
    lstore(0);
    __syncthreads();
    for (int c = 0; c < nchunks; c++) {
        const int buf = c & 1;
        const bool more = c + 1 < nchunks;                 // workgroup-uniform
        if (more) gload(c + 1);
        const float *L = lds + buf * BUF;
#pragma unroll
        for (int st = 0; st < FG_KC / 2; st++) {           // elements 2 st (lanes 0-31) and 2 st + 1 (lanes 32-63)
            const int ko = 2 * st + kh;
            float fa[RN], fb[RM];
#pragma unroll
            for (int a = 0; a < RN; a++) fa[a] = L[(arow + 32 * a) * FG_PITCH + ko];
#pragma unroll
            for (int r = 0; r < RM; r++) fb[r] = L[(brow + 32 * r) * FG_PITCH + ko];
#pragma unroll
            for (int a = 0; a < RN; a++)
#pragma unroll
                for (int r = 0; r < RM; r++)
                    acc[a][r] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[a], fb[r], acc[a][r], 0, 0, 0);
        }
        if (more) lstore(buf ^ 1);
        __syncthreads();
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

template <int BN, int WM, int WN>
static hipError_t launch_gemm_f32w(const float *W, const float *x, int64_t K, int64_t M, int64_t N, int S, float *y,
                                   int64_t ldy, float *slabs, hipStream_t s) {
    constexpr int lds = 2 * (FG_BM + BN) * FG_PITCH * 4;
    if (const hipError_t e = raise_dynamic_lds<k_gemm_f32w<BN, WM, WN>>(lds); e != hipSuccess) return e;
    const int64_t ntn = (N + BN - 1) / BN, ntm = (M + FG_BM - 1) / FG_BM;
    (void)hipGetLastError();  // report only these launches' error
    launch_k(k_gemm_f32w<BN, WM, WN>, dim3((unsigned)ntm, (unsigned)ntn, (unsigned)S), dim3(FG_THREADS), (size_t)lds, s, W, x, (int)K,
             (int)M, (int)N, (int)(K / S), S > 1 ? slabs : y, S > 1 ? M : ldy, S > 1 ? N * M : (int64_t)0);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    if (S > 1) {
        launch_k(k_f32w_slabs, dim3((unsigned)((N * M + FG_THREADS - 1) / FG_THREADS)), dim3(FG_THREADS), 0, s,
                 (const float *)slabs, S, M, N * M, y, ldy);
        return hipGetLastError();
    }
    return hipSuccess;
}

// ws: ws_bytes >= gemm_f32w_ws_bytes(K, M, N, dev.num_cus) bytes, 16-byte aligned (checked against the S that runs: a
// pin that changed since the sizing cannot write past the workspace)
hipError_t gemm_f32w(const void *W, int64_t K, int64_t M, const float *x, int64_t N, float *y, int64_t ldy, void *ws,
                     size_t ws_bytes, const DeviceInfo &dev, hipStream_t s) {
    if (!gemm_f32w_supported(K, M, N)) return hipErrorInvalidValue;
    const int S = gemm_f32w_ksplit(K, M, N, dev.num_cus);
    if (S > 1 && (!ws || ws_bytes < (size_t)S * (size_t)N * (size_t)M * 4)) return hipErrorInvalidValue;
    const float *w = (const float *)W;
    switch (fg_bn(M, N, dev.num_cus)) {
        case 32: return launch_gemm_f32w<32, 4, 1>(w, x, K, M, N, S, y, ldy, (float *)ws, s);
        case 64: return launch_gemm_f32w<64, 2, 2>(w, x, K, M, N, S, y, ldy, (float *)ws, s);
        default: return launch_gemm_f32w<128, 2, 2>(w, x, K, M, N, S, y, ldy, (float *)ws, s);
    }
}

}  // namespace ghip
