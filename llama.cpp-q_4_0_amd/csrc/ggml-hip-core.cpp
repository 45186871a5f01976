// ggml-hip-core.cpp — host side of the MI355X q4_0 mul_mat backend: per-device state, temporaries,
// workspaces and the device-pointer mul_mat core (ggml_compute_forward_mul_mat_q_f32 INIT + COMPUTE).
// The C ABI of include/ggml-hip.h is spread over ggml-hip-{api,tensor,fuse,ops,wcache,comm}.cpp, which
// share the declarations of ggml-hip-internal.h.  Mirrors the reference's ggml-cuda.cu host plumbing for
// this path (file:line in each function comment) with a native design:
//   * one non-blocking HIP stream per device, created once (ggml-cuda.cu:1849);
//   * a per-device caching pool for temporaries (ggml-cuda.cu:1751-1811);
//   * mul_mat = fused q8_0-quantize + GEMV for N <= 8 tokens, q8_0-quantize + MFMA GEMMs otherwise
//     (replacing dequantize_mul_mat_vec / dequantize_block + cublasSgemm, ggml-cuda.cu:1177-1244,
//     1156-1175, 2143-2182).
#include "ggml-hip-internal.h"

using namespace ghh;

namespace ghh {

// ------------------------------------------------------------------------------------------
// errors: the tensor ABI is fail-fast like CUDA_CHECK (ggml-cuda.cu:22-51); the tensor-free
// ABI returns a status and keeps the message for ggml_hip_last_error().

thread_local std::string g_last_error;

}  // namespace ghh

namespace ghh {

int fail(int code, const std::string &msg) {
    g_last_error = msg;
    return code;
}

}  // namespace ghh

namespace ghh {

std::once_flag g_init_once;
int g_device_count = 0;
Device *g_dev = nullptr;
int g_main_device = 0;
float g_tensor_split[GGML_HIP_MAX_DEVICES] = {0};

}  // namespace ghh

namespace ghh {

size_t g_scratch_size = 0;
void *g_scratch = nullptr;
size_t g_scratch_offset = 0;
bool g_eval_computed = false;            // a node ran since the last buffer assignment

void init_impl() {
    if (hipGetDeviceCount(&g_device_count) != hipSuccess) g_device_count = 0;
    if (g_device_count > GGML_HIP_MAX_DEVICES) g_device_count = GGML_HIP_MAX_DEVICES;
    g_dev = new Device[g_device_count > 0 ? g_device_count : 1];
    int cur = 0;
    if (g_device_count > 0) HIP_FATAL(hipGetDevice(&cur));
    double total = 0;
    for (int id = 0; id < g_device_count; id++) {
        hipDeviceProp_t prop;
        HIP_FATAL(hipGetDeviceProperties(&prop, id));
        g_dev[id].info.num_cus = prop.multiProcessorCount;
        g_dev[id].total_mem = prop.totalGlobalMem;
        g_tensor_split[id] = (float)total;        // default split proportional to VRAM (ggml-cuda.cu:1838-1843)
        total += (double)prop.totalGlobalMem;
        if (getenv("GGML_HIP_VERBOSE"))
            fprintf(stderr, "ggml_init_hip: device %d: %s (%s), %d CUs, %.1f GiB\n", id, prop.name,
                    prop.gcnArchName, prop.multiProcessorCount, prop.totalGlobalMem / 1073741824.0);
    }
    for (int id = 0; id < g_device_count; id++) g_tensor_split[id] = (float)(g_tensor_split[id] / total);
    for (int id = 0; id < g_device_count; id++) {
        HIP_FATAL(hipSetDevice(id));
        HIP_FATAL(hipStreamCreateWithFlags(&g_dev[id].stream, hipStreamNonBlocking));
        HIP_FATAL(hipEventCreateWithFlags(&g_dev[id].ev_a, hipEventDisableTiming));
        HIP_FATAL(hipEventCreateWithFlags(&g_dev[id].ev_b, hipEventDisableTiming));
    }
    if (g_device_count > 0) HIP_FATAL(hipSetDevice(cur));
}

void ensure_init() { std::call_once(g_init_once, init_impl); }

int current_device() {
    int d = 0;
    (void)hipGetDevice(&d);
    return d;
}

hipStream_t resolve_stream(void *stream) {
    if (stream) return (hipStream_t)stream;
    ensure_init();
    return g_dev[current_device()].stream;
}

void *pool_malloc(int id, size_t size, size_t *actual) {
    Device &d = g_dev[id];
    {
        std::lock_guard<std::mutex> lk(d.mu);
        int best = -1;
        for (size_t i = 0; i < d.pool.size(); i++)
            if (d.pool[i].size >= size && (best < 0 || d.pool[i].size < d.pool[best].size)) best = (int)i;
        if (best >= 0) {
            PoolBuf b = d.pool[best];
            d.pool.erase(d.pool.begin() + best);
            *actual = b.size;
            return b.ptr;
        }
    }
    const size_t sz = (size_t)(size * 1.05) + 256;     // a little slack, like ggml_cuda_pool_malloc
    void *p = nullptr;
    HIP_FATAL(hipMalloc(&p, sz));
    *actual = sz;
    return p;
}

void pool_free(int id, void *p, size_t size) {
    Device &d = g_dev[id];
    std::lock_guard<std::mutex> lk(d.mu);
    d.pool.push_back({p, size});
}

// the planes of a quantized x at the start of a workspace: qs [N][K] int8, d [N][K/32] f32, and behind them a third
// plane (q8_1's s [N][K/32] f32, or the fp16 copy of d below); every plane starts at a multiple of 256 bytes
static size_t pad256(size_t n) { return (n + 255) & ~(size_t)255; }
static size_t ws_d_offset(int64_t K, int64_t N) { return pad256((size_t)(N * K)); }
static size_t ws_d_bytes(int64_t K, int64_t N) { return pad256((size_t)N * (K / QK) * 4); }
// workspace for the q8_0 activations of one mul_mat: the qs and d planes + the same d as fp16, block-major
// [K/32][N rounded up to 4] (the LDS GEMM's operand layout), in the third plane's place
size_t ws_d16_offset(int64_t K, int64_t N) { return ws_d_offset(K, N) + ws_d_bytes(K, N); }
XPlanes x_planes(void *ws, int64_t K, int64_t N) {
    return {(int8_t *)ws, (float *)((char *)ws + ws_d_offset(K, N)), (float *)((char *)ws + ws_d16_offset(K, N))};
}
size_t workspace_bytes(int64_t K, int64_t N) { return ws_d16_offset(K, N) + (size_t)((N + 3) & ~3) * (K / QK) * 2; }
// the LDS GEMM (algo 2, v8 / v9) adds its x image and the per-call weight image of an M-row matrix (room
// for either image format)
size_t ws_g8x_offset(int64_t K, int64_t N) { return (workspace_bytes(K, N) + 255) & ~(size_t)255; }
size_t ws_g8w_offset(int64_t K, int64_t N) {
    return (ws_g8x_offset(K, N) + std::max(ghip::gemm8_x_bytes(K, N), ghip::gemm9_x_bytes(K, N)) + 255) & ~(size_t)255;
}
size_t workspace_bytes_mm(int64_t K, int64_t N, int64_t M) {
    return ws_g8w_offset(K, N) + std::max(ghip::gemm8_w_bytes(K, M), ghip::gemm9_w_bytes(K, M));
}
// prefill GEMM version (GGML_HIP_GEMM_V / ggml_hip_debug_set_gemm_version): 10 (default) = k_gemm9 when
// the weight has an image (ggml_hip_weight_image_create, or built on first prefill use of a
// device-resident ggml weight; images are built in fp6 format), else k_gemm7 on the q4_0 bytes; 8 = the
// same with int8 images (k_gemm8); 9 / 11 = k_gemm8 / k_gemm9 always (an unregistered weight is
// converted into the workspace per call); 7 = k_gemm7 always.  A weight's image keeps the format it
// was built in; the GEMM follows the image.
std::atomic<int> g_gemm_v{-1};
int gemm_version() {
    int v = g_gemm_v.load(std::memory_order_relaxed);
    if (v < 0) {
        const char *e = getenv("GGML_HIP_GEMM_V");
        int want = e ? atoi(e) : 10, expect = -1;
        g_gemm_v.compare_exchange_strong(expect, want);
        v = g_gemm_v.load(std::memory_order_relaxed);
    }
    return v;
}

}  // namespace ghh

namespace ghh {

int reserve_workspace(int id, size_t bytes, hipStream_t s) {
    Device &d = g_dev[id];
    std::lock_guard<std::mutex> lk(d.mu);
    if (!s) s = d.stream;
    void *&ws = s == d.stream ? d.ws : d.stream_ws[s].ptr;
    size_t &ws_size = s == d.stream ? d.ws_size : d.stream_ws[s].size;
    if (ws_size >= bytes) return GGML_HIP_OK;
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &st) == hipSuccess && st != hipStreamCaptureStatusNone)
        return fail(GGML_HIP_ERR_INVALID, "workspace must be reserved before stream capture");
    if (ws) {
        HIP_RET(GHIP_SYNC(hipDeviceSynchronize)());
        HIP_RET(GHIP_SYNC(hipFree)(ws));
        ws = nullptr;
        ws_size = 0;
    }
    HIP_RET(hipMalloc(&ws, bytes));
    ws_size = bytes;
    return GGML_HIP_OK;
}

// the workspace of stream s on device id (grown on demand outside capture)
int stream_workspace(int id, hipStream_t s, size_t need, void **out) {
    Device &d = g_dev[id];
    {
        std::lock_guard<std::mutex> lk(d.mu);
        if (s == d.stream && d.ws_size >= need) {
            *out = d.ws;
            return GGML_HIP_OK;
        }
        if (s != d.stream) {
            auto it = d.stream_ws.find(s);
            if (it != d.stream_ws.end() && it->second.size >= need) {
                *out = it->second.ptr;
                return GGML_HIP_OK;
            }
        }
    }
    const int rc = reserve_workspace(id, need, s);
    if (rc != GGML_HIP_OK) return rc;
    std::lock_guard<std::mutex> lk(d.mu);
    *out = s == d.stream ? d.ws : d.stream_ws[s].ptr;
    return GGML_HIP_OK;
}

bool aligned(const void *p, size_t a) { return ((uintptr_t)p % a) == 0; }

}  // namespace ghh

namespace ghh {

// ------------------------------------------------------------------------------------------
// the mul_mat core (device pointers): ggml_compute_forward_mul_mat_q_f32 INIT + COMPUTE

// exact mode (algo 4 for every auto-selected mul_mat): GGML_HIP_EXACT=1 or ggml_hip_set_exact
std::atomic<int> g_exact{-1};
bool exact_mode() {
    int v = g_exact.load(std::memory_order_relaxed);
    if (v < 0) {
        const char *e = getenv("GGML_HIP_EXACT");
        int want = (e && atoi(e) != 0) ? 1 : 0, expect = -1;
        g_exact.compare_exchange_strong(expect, want);
        v = g_exact.load(std::memory_order_relaxed);
    }
    return v == 1;
}

// xq: in/out mask of the q8_0(x) forms already in this stream's workspace from the previous call
// (siblings that share x: ggml_hip_mul_mat_q4_0_multi quantizes once per form): XQ_SOA = qs + d (split-K,
// exact, gemm7), XQ_G8 = the k_gemm8 x image; null = quantize; ignored by the fused GEMV
int mul_mat_dev(const void *w, int64_t K, int64_t M, const float *x, int64_t N, float *y, int64_t ldy, int algo,
                hipStream_t s, unsigned *xq) {
    unsigned xq_local = 0;
    if (!xq) xq = &xq_local;
    if (!w || !x || !y || K <= 0 || M <= 0 || N < 0) return fail(GGML_HIP_ERR_INVALID, "null pointer or bad shape");
    if (N == 0) return GGML_HIP_OK;
    if (K % 64 != 0) return fail(GGML_HIP_ERR_INVALID, "K must be a multiple of 64 (ggml.c:2344 nb % 2 == 0)");
    if (ldy < M) return fail(GGML_HIP_ERR_INVALID, "ldy < M");
    if (!aligned(w, 16) || !aligned(x, 16) || !aligned(y, 4))
        return fail(GGML_HIP_ERR_INVALID, "W and x must be 16-byte aligned, y 4-byte aligned");
    if (M * (K / QK) * Q4B >= ((int64_t)1 << 31) || N * K >= ((int64_t)1 << 31) || M >= (1 << 30))
        return fail(GGML_HIP_ERR_UNSUPPORTED, "matrix too large for 32-bit buffer offsets; split rows");
    const int id = current_device();
    const int max_nt = ghip::gemv_max_tokens(K);
    // auto: exact mode if switched on; else fused GEMV for N <= 8, split-K MFMA for N <= 128,
    // LDS-staged MFMA GEMM above (crossovers measured with tools/n_sweep.py); a
    // weight with an image takes the image GEMM from N > IMG_MIN_N (tools/n_sweep9.py)
    if (algo == 0) {
        if (exact_mode()) algo = 4;
        else if (N <= max_nt) algo = 1;
        else if (N > 128) algo = 2;
        else if ((N > IMG_MIN_N || M >= IMG_MIN_M) && gemm_version() >= 8 && wimage_find(id, w, K, M)) algo = 2;
        else algo = 3;
    }
    if (algo == 1) {
        if (N > max_nt) return fail(GGML_HIP_ERR_INVALID, "GEMV path supports N <= gemv_max_tokens(K)");
        HIP_RET(ghip::gemv_q4_0(w, K, M, x, N, y, ldy, g_dev[id].info, s));
        return GGML_HIP_OK;
    }
    if (algo < 2 || algo > 4) return fail(GGML_HIP_ERR_INVALID, "algo must be 0, 1, 2, 3 or 4");
    void *ws = nullptr;
    const int gv = gemm_version();
    int fmt = 0;
    const void *wimg = algo == 2 && gv >= 8 ? wimage_find(id, w, K, M, &fmt) : nullptr;
    if (algo == 2 && (wimg || gv == 9 || gv == 11)) {   // k_gemm8 / k_gemm9 on weight + x images
        if (!wimg) fmt = gv == 11 ? 9 : 8;
        const int wrc = stream_workspace(id, s, workspace_bytes_mm(K, N, wimg ? 0 : M), &ws);
        if (wrc != GGML_HIP_OK) return wrc;
        void *xws = (char *)ws + ws_g8x_offset(K, N);
        const unsigned form = fmt == 9 ? XQ_G9 : XQ_G8;        // one x image region: the forms exclude
        if (!(*xq & form))
            HIP_RET(fmt == 9 ? ghip::gemm9_prep_x(x, K, N, xws, s) : ghip::gemm8_prep_x(x, K, N, xws, s));
        *xq = (*xq & ~(unsigned)(XQ_G8 | XQ_G9)) | form;
        if (!wimg) {                            // unregistered weight: converted per call
            void *wws = (char *)ws + ws_g8w_offset(K, N);
            HIP_RET(fmt == 9 ? ghip::gemm9_prep_w(w, K, M, wws, s) : ghip::gemm8_prep_w(w, K, M, wws, s));
            wimg = wws;
        }
        HIP_RET(fmt == 9 ? ghip::gemm9_run(wimg, K, M, xws, N, y, ldy, s) : ghip::gemm8_run(wimg, K, M, xws, N, y, ldy, s));
        return GGML_HIP_OK;
    }
    const int wrc = stream_workspace(id, s, workspace_bytes(K, N), &ws);
    if (wrc != GGML_HIP_OK) return wrc;
    const XPlanes xp = x_planes(ws, K, N);
    int8_t *qs = xp.qs;
    float *xd = xp.d;
    uint16_t *xd16 = (uint16_t *)xp.s;                       // the fp16 d copy takes the third plane's place
    // the fp16 block-major d_x copy (gemm7) is written whenever qs/d are: a sibling group may mix algos
    if (!(*xq & XQ_SOA)) HIP_RET(ghip::quantize_q8_0_soa(x, K, N, qs, xd, s, xd16));
    *xq |= XQ_SOA;
    if (algo == 4)
        HIP_RET(ghip::mm_exact_q4_0(w, K, M, qs, xd, N, y, ldy, s));
    else if (algo == 3)
        HIP_RET(ghip::gemm_sk_q4_0(w, K, M, qs, xd, N, y, ldy, g_dev[id].info.num_cus, s));
    else
        HIP_RET(ghip::gemm_q4_0(w, K, M, qs, xd, N, y, ldy, s, xd16));
    return GGML_HIP_OK;
}

// ------------------------------------------------------------------------------------------
// The weight types beside Q4_0: one row each (WeightType, ggml-hip-internal.h).  A type's mul_mat has algo 0 auto
// (auto_algo), 1 the fused GEMV in column tiles, 4 the exact kernel and the type's own GEMM algo; the GEMM's y is
// bit for bit the GEMV's on the k-quants (the same exact integer superblock sums, the same fp32 step per
// superblock in the same order), so the switch between the two never changes a result.  On Q8_0, Q5_0, Q4_1 and
// Q5_1 it is not: the GEMV adds a row's blocks as 64 lane chains and a tree, the GEMMs as one chain per output (Q4_1
// / Q5_1, algo 7) or k_gemm8's order (Q8_0, Q5_0), so there the switch between GEMV and GEMM moves a result within
// the parity bound.

int GemmMinN::get() {
    int n = v.load(std::memory_order_relaxed);
    if (n < 0) {
        const char *e = getenv(env);
        int want = e ? atoi(e) : dflt, expect = -1;
        if (want < 9) want = 9;
        v.compare_exchange_strong(expect, want);
        n = v.load(std::memory_order_relaxed);
    }
    return n;
}
int GemmMinN::set(int n) {
    const int prev = get();
    v.store(n < 0 ? -1 : (n < 9 ? 9 : n), std::memory_order_relaxed);     // -1: re-read the environment
    return prev;
}

// the measured crossovers.  Q6_K (tools/q6k_gemm_bench.py, profiles/q6k_gemm.json, lm_head shape): the
// GEMM wins at every swept N from 9, the rule's floor.  Q8_0 (tools/q8_0_bench.py, profiles/q8_0_gemm.json, 4096 x
// 4096): the tiled GEMV wins at N = 9 and 16 (16.2 / 22.7 us against the GEMM arm's flat 35 us, most of it the
// per-call image), the GEMM from N = 32 (35.3 against 43.4 us).  Q5_K / Q4_K (tools/q45k_gemm_bench.py,
// profiles/q45k_gemm.json; the LLaMA-7B layer shapes, weights from memory): the GEMM's time is flat in N up to 128,
// so the tiled GEMV wins at N = 9 and ties at N = 16; from N = 32 the GEMM wins on every shape of both types (Q5_K
// 4096 -> 4096: 52.5 against 99.6 us).  One threshold for the two: their crossovers do not differ.
static GemmMinN g_q6k_min_n{"GGML_HIP_Q6K_GEMM_MIN_N", 9};
static GemmMinN g_q8_0_min_n{"GGML_HIP_Q8_0_GEMM_MIN_N", 32};
static GemmMinN g_q45k_min_n{"GGML_HIP_Q45K_GEMM_MIN_N", 32};
// Q5_0 (tools/q5x_bench.py, profiles/q5x_gemm.json; the three LLaMA-7B layer shapes, N = 9 .. 128): the GEMM arm is
// flat in N (34-35 / 45-46 / 76-77 us, most of it the per-call image), the tiled GEMV wins at N = 9 and 16 on every
// shape (4096 -> 11008 at N = 16: 44.8 against 44.9 us) and loses from N = 32 on every shape (4096 -> 4096: 45.6
// against 34.9 us)
static GemmMinN g_q5_0_min_n{"GGML_HIP_Q5_0_GEMM_MIN_N", 32};
// Q4_1 / Q5_1 (algo 7, q5x_gemm.hip): "never" by default, so auto runs the GEMV at every N until the user sets the
// threshold (the measured crossover is in DESIGN §4b; tools/q5x_bench.py, profiles/q5x1_gemm.json)
static GemmMinN g_q41_q51_min_n{"GGML_HIP_Q41_Q51_GEMM_MIN_N", INT_MAX};
// Q3_K / Q2_K (algo 8, q23_k_gemm.hip): "never" by default, so auto runs the GEMV's column tiles at every N until the
// user sets the threshold (the measured crossover is in DESIGN §4b; tools/q23k_gemm_bench.py,
// profiles/q23k_gemm.json).  The GEMM's y is the GEMV's bit for bit, so setting it never changes a result.
static GemmMinN g_q23k_min_n{"GGML_HIP_Q23K_GEMM_MIN_N", INT_MAX};
// F16 (algo 9 = k_mul_mat_f16_f32_mfma, the attention's fast-mode kernel): 32, the N at which an F16 src0 took that
// kernel before the GEMV existed (GGML_HIP_F16_MFMA_MIN's default).  Measured (tools/f16w_bench.py,
// profiles/f16w_gemm.json; weights from HBM; tiled GEMV against the MFMA kernel, us): 4096 -> 4096 N = 32 47.4 / 93.9,
// N = 64 92.3 / 94.5, N = 128 182.7 / 93.3; 4096 -> 11008 N = 16 52.0 / 95.2, N = 32 103.2 / 97.3, N = 64 203.7 /
// 98.6; 11008 -> 4096 N = 32 143.6 / 250.5, N = 64 273.4 / 252.3.  The crossover is at 128 / 32 / 64: it is not away
// from 32 on all three shapes, so the default stays 32.  The MFMA kernel, built for K = 128, is flat in N at ~93 / 97 /
// 250 us up to N = 512 (0.36 / 0.93 / 0.36 TB/s of weight bytes): a weight-shaped F16 GEMM is DESIGN §8's.
static GemmMinN g_f16w_min_n{"GGML_HIP_F16W_GEMM_MIN_N", 32};
// F16 (algo 11 = k_gemm_f16w, f16_w_gemm.hip, the GEMM decomposed for weight shapes): "never" by default, so auto runs
// the rule above at every N until the user sets the threshold (the measured table is in DESIGN §4b; tools/f16w_bench.py,
// profiles/f16w_wgemm.json).  Its y is within the bound of the GEMV's and of algo 9's, not bitwise either.
static GemmMinN g_f16w_wgemm_min_n{"GGML_HIP_F16W_WGEMM_MIN_N", INT_MAX};
GemmMinN *f16w_wgemm_min_n() { return &g_f16w_wgemm_min_n; }
// F32 (algo 12 = k_gemm_f32w, f32_w_gemm.hip): 16, the smallest swept N from which the GEMM beats the GEMV's column
// tiles on all three LLaMA-7B layer shapes with spreads that do not overlap (tools/f32w_bench.py, profiles/f32w.json,
// DESIGN §4b; weights from HBM).  At N = 9 the two tie on 4096 -> 4096 and the GEMM wins the other two shapes; at
// K = 11008, where the GEMV takes 2 columns per launch, the GEMM wins from the rule's floor of 9.
static GemmMinN g_f32w_min_n{"GGML_HIP_F32W_GEMM_MIN_N", 16};

// the K a type's GEMV takes: one token's q8_K image in the LDS for the k-quants (w2 of a 30B / 65B model has K =
// 17920 / 22016), one token's q8_0 for Q8_0
static bool gemv_takes_k_kquant(int64_t K) { return K <= 16384; }
static bool gemv_takes_k_q8_0(int64_t K) { return ghip::gemv_q8_0w_max_tokens(K) >= 1; }
static bool gemv_takes_k_q5x(int64_t K) { return ghip::gemv_q5x_max_tokens(K) >= 1; }
static bool gemv_takes_k_f16w(int64_t K) { return ghip::gemv_f16w_max_tokens(K) >= 1; }
static bool gemv_takes_k_f32w(int64_t K) { return ghip::gemv_f32w_max_tokens(K) >= 1; }

static MulMatSig mul_mat_q6k_dev, mul_mat_q8_0_dev, mul_mat_q5k_dev, mul_mat_q4k_dev;
static MulMatSig mul_mat_q4_1_dev, mul_mat_q5_0_dev, mul_mat_q5_1_dev;
static MulMatSig mul_mat_q3k_dev, mul_mat_q2k_dev;
static MulMatSig mul_mat_f16w_dev, mul_mat_f32w_dev;

static constexpr const char *ERR_K256 = "K must be a multiple of 256 (QK_K)";
static constexpr const char *ERR_ALIGN_Q45K = "W and x must be 16-byte, y 4-byte aligned";
static constexpr const char *ERR_GEMV_Q45K = "the Q5_K / Q4_K GEMV supports K <= 16384";
static constexpr const char *ERR_DQ_Q45K = "w and the Q5_K / Q4_K rows must be 16-byte aligned";

// Where the GEMV cannot take K, auto runs the GEMM on Q6_K and Q8_0 and the exact kernel, which has no K limit, on
// Q5_K / Q4_K (so no shape the hook path accepts fails, and a long K computes what it did before their GEMM existed).
// The Q5_K / Q4_K blocks are multiples of 16 bytes and their kernels read them as naturally aligned vectors.
// fields, in WeightType's order: K granule, W alignment, M limit | GEMM algo, algo where the GEMV cannot take K, threshold,
// the GEMV's K rule, run | texts: K granule, alignment, GEMV K | dequantizer: K granule, row alignment, text
static const WeightType ROW_Q6_K = {
    QK_K, 2, (int64_t)1 << 31,
    5, 5, &g_q6k_min_n, gemv_takes_k_kquant, mul_mat_q6k_dev,
    ERR_K256, "W must be 2-byte, x 16-byte, y 4-byte aligned", "the Q6_K GEMV supports K <= 16384",
    QK_K, 2, "w must be 16-byte aligned, the Q6_K rows 2-byte aligned"};
static const WeightType ROW_Q8_0 = {
    64, 4, 1 << 30,
    2, 2, &g_q8_0_min_n, gemv_takes_k_q8_0, mul_mat_q8_0_dev,
    "K must be a multiple of 64 (ggml.c:3236 nb % 2 == 0)", "W must be 4-byte, x 16-byte, y 4-byte aligned",
    "K too long for the Q8_0 GEMV",
    QK, 2, "w must be 16-byte aligned, the Q8_0 rows 2-byte aligned"};
static const WeightType ROW_Q5_K = {
    QK_K, 16, (int64_t)1 << 31,
    6, 4, &g_q45k_min_n, gemv_takes_k_kquant, mul_mat_q5k_dev,
    ERR_K256, ERR_ALIGN_Q45K, ERR_GEMV_Q45K,
    QK_K, 16, ERR_DQ_Q45K};
static const WeightType ROW_Q4_K = {
    QK_K, 16, (int64_t)1 << 31,
    6, 4, &g_q45k_min_n, gemv_takes_k_kquant, mul_mat_q4k_dev,
    ERR_K256, ERR_ALIGN_Q45K, ERR_GEMV_Q45K,
    QK_K, 16, ERR_DQ_Q45K};

// Q3_K / Q2_K (q23_k.hip): the matrix 4-byte aligned, which leaves a Q3_K block (110 bytes) at 0 or 2 mod 4; the
// kernels read no byte outside the matrix.  The GEMM (algo 8) sits behind a threshold whose default is "never"; the
// exact kernel where the GEMV cannot take K.
static constexpr const char *ERR_ALIGN_Q23K = "W must be 4-byte, x 16-byte, y 4-byte aligned";
static constexpr const char *ERR_GEMV_Q23K = "the Q3_K / Q2_K GEMV supports K <= 16384";
static constexpr const char *ERR_DQ_Q23K = "w must be 16-byte aligned, the Q3_K / Q2_K rows 2-byte aligned";
static const WeightType ROW_Q3_K = {
    QK_K, 4, (int64_t)1 << 31,
    8, 4, &g_q23k_min_n, gemv_takes_k_kquant, mul_mat_q3k_dev,
    ERR_K256, ERR_ALIGN_Q23K, ERR_GEMV_Q23K,
    QK_K, 2, ERR_DQ_Q23K};
static const WeightType ROW_Q2_K = {
    QK_K, 4, (int64_t)1 << 31,
    8, 4, &g_q23k_min_n, gemv_takes_k_kquant, mul_mat_q2k_dev,
    ERR_K256, ERR_ALIGN_Q23K, ERR_GEMV_Q23K,
    QK_K, 2, ERR_DQ_Q23K};

// Q4_1 / Q5_0 / Q5_1 (blk32_w.hip).  Q5_0's values q - 16 are int8 and its activations q8_0, so it takes Q8_0's GEMM
// (algo 2).  Q4_1 and Q5_1 cannot: their activation scale is an unrounded f32 and they carry a second term m_w s_x
// per block, which k_gemm8's fp16 d_x plane and single-term epilogue do not hold.  They have a GEMM of their own on
// the weights in place (algo 7, k_gemm_q5x1) behind a threshold of their own whose default is "never": until it is
// set, prefill runs as column tiles of the GEMV.  Where the GEMV cannot take K they run the exact kernel, which has
// no K limit.
static constexpr const char *ERR_K64_Q5X = "K must be a multiple of 64 (ggml.c:2614, 2740, 2980 nb % 2 == 0)";
static constexpr const char *ERR_ALIGN_Q5X = "W must be 4-byte, x 16-byte, y 4-byte aligned";
static constexpr const char *ERR_GEMV_Q5X = "K too long for the Q4_1 / Q5_0 / Q5_1 GEMV";
static constexpr const char *ERR_DQ_Q5X = "w must be 16-byte aligned, the Q4_1 / Q5_0 / Q5_1 rows 4-byte aligned";
static const WeightType ROW_Q4_1 = {
    64, 4, 1 << 30,
    7, 4, &g_q41_q51_min_n, gemv_takes_k_q5x, mul_mat_q4_1_dev,
    ERR_K64_Q5X, ERR_ALIGN_Q5X, ERR_GEMV_Q5X,
    64, 4, ERR_DQ_Q5X};
static const WeightType ROW_Q5_0 = {
    64, 4, 1 << 30,
    2, 2, &g_q5_0_min_n, gemv_takes_k_q5x, mul_mat_q5_0_dev,
    ERR_K64_Q5X, ERR_ALIGN_Q5X, ERR_GEMV_Q5X,
    64, 4, ERR_DQ_Q5X};
static const WeightType ROW_Q5_1 = {
    64, 4, 1 << 30,
    7, 4, &g_q41_q51_min_n, gemv_takes_k_q5x, mul_mat_q5_1_dev,
    ERR_K64_Q5X, ERR_ALIGN_Q5X, ERR_GEMV_Q5X,
    64, 4, ERR_DQ_Q5X};

// F16 (f16_w.hip; the "mostly F16" files): contiguous rows of K halves, 16-byte aligned, K % 32 == 0 (the reference's
// GGML_CUDA_DMMV_X).  There is nothing to dequantize: exact mode (algo 4) and the table's GEMM (algo 9) are the
// attention's F16 x F32 kernels (ggml_ops.hip) on contiguous strides, unchanged.  The exact kernels where the GEMV
// cannot take K.  The weight-shaped GEMM (algo 11) sits in front of this row's rule behind a threshold of its own
// (auto_algo_f16w).
static const WeightType ROW_F16 = {
    32, 16, (int64_t)1 << 31,
    9, 4, &g_f16w_min_n, gemv_takes_k_f16w, mul_mat_f16w_dev,
    "K must be a multiple of 32", "W and x must be 16-byte, y 4-byte aligned", "K too long for the F16 GEMV",
    32, 16, "F16 rows are not dequantized"};

// F32 (f32_w.hip, f32_w_gemm.hip; the "all F32" files): contiguous rows of K floats, 16-byte aligned, K % 32 == 0 (the
// scalar leftover loop of ggml_vec_dot_f32 is contracted or not at the compiler's discretion, so no exact kernel can
// restate it).  Nothing is dequantized.  The exact kernel where the GEMV cannot take K (one column's 4 K bytes past
// the LDS).
static const WeightType ROW_F32 = {
    32, 16, (int64_t)1 << 31,
    12, 4, &g_f32w_min_n, gemv_takes_k_f32w, mul_mat_f32w_dev,
    "K must be a multiple of 32", "W and x must be 16-byte, y 4-byte aligned", "K too long for the F32 GEMV",
    32, 16, "F32 rows are not dequantized"};

const WeightType *weight_type(int type) {
    switch (type) {
        case gabi::TYPE_F32: return &ROW_F32;
        case gabi::TYPE_F16: return &ROW_F16;
        case gabi::TYPE_Q4_1: return &ROW_Q4_1;
        case gabi::TYPE_Q5_0: return &ROW_Q5_0;
        case gabi::TYPE_Q5_1: return &ROW_Q5_1;
        case gabi::TYPE_Q6_K: return &ROW_Q6_K;
        case gabi::TYPE_Q8_0: return &ROW_Q8_0;
        case gabi::TYPE_Q5_K: return &ROW_Q5_K;
        case gabi::TYPE_Q4_K: return &ROW_Q4_K;
        case gabi::TYPE_Q3_K: return &ROW_Q3_K;
        case gabi::TYPE_Q2_K: return &ROW_Q2_K;
        default: return nullptr;
    }
}

int auto_algo(const WeightType &t, int64_t K, int64_t N) {
    if (exact_mode()) return 4;
    if (!t.gemv_takes_k(K)) return t.no_gemv_algo;
    return N >= t.min_n->get() ? t.gemm_algo : 1;
}

// F16: exact mode -> 4; from the weight-shaped GEMM's threshold (default "never") and where its launch takes the shape
// -> 11, at any K (it has no LDS-bound K limit); else the table's rule
int auto_algo_f16w(int64_t K, int64_t M, int64_t N) {
    if (exact_mode()) return 4;
    if (N >= g_f16w_wgemm_min_n.get() && ghip::gemm_f16w_supported(K, M, N)) return 11;
    return auto_algo(ROW_F16, K, N);
}

// the workspace of algo 11 (the fp16 image of x + the K-slice slabs of the plan the call would run now on device id;
// 256 CUs where there is no device)
size_t workspace_bytes_f16w_gemm(int id, int64_t K, int64_t N, int64_t M) {
    return ghip::gemm_f16w_ws_bytes(K, M, N, id >= 0 && id < g_device_count ? g_dev[id].info.num_cus : 0);
}

// F32: the table's rule; the GEMM only where one launch's grid takes the shape (else the GEMV's column tiles)
int auto_algo_f32w(int64_t K, int64_t M, int64_t N) {
    const int algo = auto_algo(ROW_F32, K, N);
    return algo == 12 && !ghip::gemm_f32w_supported(K, M, N) ? 1 : algo;
}

// the workspace of algo 12 (the K-slice slabs of the split the call would run now on device id; 256 CUs where there
// is no device)
size_t workspace_bytes_f32w_gemm(int id, int64_t K, int64_t N, int64_t M) {
    return ghip::gemm_f32w_ws_bytes(K, M, N, id >= 0 && id < g_device_count ? g_dev[id].info.num_cus : 0);
}

// OK with N == 0 means there is nothing to run: the steps behind it are not checked then
int check_operands(const WeightType &t, const void *w, int64_t K, int64_t M, const float *x, int64_t N, const float *y,
                   int64_t ldy) {
    if (!w || !x || !y || K <= 0 || M <= 0 || N < 0) return fail(GGML_HIP_ERR_INVALID, "null pointer or bad shape");
    if (K % t.k_granule != 0) return fail(GGML_HIP_ERR_INVALID, t.err_k);
    if (N == 0) return GGML_HIP_OK;
    if (ldy < M) return fail(GGML_HIP_ERR_INVALID, "ldy < M");
    if (!aligned(w, t.w_align) || !aligned(x, 16) || !aligned(y, 4)) return fail(GGML_HIP_ERR_INVALID, t.err_align);
    if (M >= t.m_limit || N * K >= ((int64_t)1 << 31))
        return fail(GGML_HIP_ERR_UNSUPPORTED, "matrix too large for 32-bit indices; split rows or columns");
    return GGML_HIP_OK;
}

// the workspaces of the k-quant arms.  Exact: x as q8_K blocks.  Q6_K and Q3_K / Q2_K GEMM: qs int8 [N][K] + d f32
// [N][K / 256].
// Q5_K / Q4_K GEMM: qs int8 [N][K] + dig int8 [N][K / 256][16] + d f32 [N][K / 256], 256 + 20 bytes per 256 elements
// against the 288 of workspace_bytes(K, N) behind the same padding of qs.  None is more than workspace_bytes(K, N),
// which ggml_hip_reserve_workspace reserves.
static size_t workspace_bytes_q8k(int64_t K, int64_t N) { return (size_t)N * (size_t)(K / QK_K) * Q8KB; }
static size_t kquant_planes_offset(int64_t K, int64_t N) { return ws_d_offset(K, N); }
static size_t workspace_bytes_kquant_gemm(int64_t K, int64_t N) {          // (without Q5_K / Q4_K's dig)
    return kquant_planes_offset(K, N) + (size_t)N * (size_t)(K / QK_K) * 4;
}

static bool too_many_tiles(int64_t M, int64_t N) { return ((M + 63) / 64) * ((N + 63) / 64) >= ((int64_t)1 << 31); }
static constexpr const char *ERR_TILES = "too many tiles for one grid; split rows or columns";

// the exact arm of the k-quants: the q8_K quantizer into the stream's workspace; *ws = the blocks
static int quantize_q8k_ws(int id, const float *x, int64_t K, int64_t N, hipStream_t s, void **ws) {
    const int wrc = stream_workspace(id, s, workspace_bytes_q8k(K, N), ws);
    if (wrc != GGML_HIP_OK) return wrc;
    HIP_RET(ghip::quantize_q8_K(x, K, N, *ws, s));
    return GGML_HIP_OK;
}

// The five k-quants (q6_k.hip, q45_k.hip, q23_k.hip; kquant_gemm.h), one body over their rows.  algo 1 = the type's
// GEMV, 4 = the q8_K blocks of x + the type's exact kernel, the row's gemm_algo (5 Q6_K, 6 Q5_K / Q4_K, 8 Q3_K / Q2_K;
// each number is valid for its own types only) = the q8_K values of x as planes in the workspace + the type's GEMM on
// the weights in place, any K % 256 == 0.  Q5_K / Q4_K read the digits of x's sub-block sums from a plane of their
// own, between qs and d.
enum class KQuant { Q6_K, Q5_K, Q4_K, Q3_K, Q2_K };
static int mul_mat_kquant_dev(const WeightType &t, KQuant type, const void *w, int64_t K, int64_t M, const float *x,
                              int64_t N, float *y, int64_t ldy, int algo, hipStream_t s) {
    const bool q45 = type == KQuant::Q5_K || type == KQuant::Q4_K, q23 = type == KQuant::Q3_K || type == KQuant::Q2_K;
    const bool algo_ok = algo == 0 || algo == 1 || algo == 4 || algo == t.gemm_algo;
    auto bad_algo = [&] { return fail(GGML_HIP_ERR_INVALID, "algo must be 0, 1, 4 or " + std::to_string(t.gemm_algo)); };
    // Q6_K checks the operands first, so its empty call is OK whatever the algo; the others refuse an algo they
    // reject before anything else, an empty call included
    if (type != KQuant::Q6_K && !algo_ok) return bad_algo();
    const int rc = check_operands(t, w, K, M, x, N, y, ldy);
    if (rc != GGML_HIP_OK || N == 0) return rc;
    const int id = current_device();
    if (algo == 0) algo = auto_algo(t, K, N);
    if (algo == 1) {
        if (!t.gemv_takes_k(K)) return fail(GGML_HIP_ERR_UNSUPPORTED, t.err_gemv_k);
        HIP_RET(q45   ? ghip::gemv_q45_K(type == KQuant::Q5_K, w, K, M, x, N, y, ldy, g_dev[id].info, s)
                : q23 ? ghip::gemv_q23_K(type == KQuant::Q3_K, w, K, M, x, N, y, ldy, g_dev[id].info, s)
                      : ghip::gemv_q6_K(w, K, M, x, N, y, ldy, g_dev[id].info, s));
        return GGML_HIP_OK;
    }
    if (!algo_ok) return bad_algo();                     // (Q6_K only: the others were refused above)
    void *ws = nullptr;
    if (algo == t.gemm_algo) {
        if (too_many_tiles(M, N)) return fail(GGML_HIP_ERR_UNSUPPORTED, ERR_TILES);
        const size_t dig_bytes = q45 ? (size_t)N * (size_t)(K / QK_K) * 16 : 0;
        const int wrc = stream_workspace(id, s, workspace_bytes_kquant_gemm(K, N) + dig_bytes, &ws);
        if (wrc != GGML_HIP_OK) return wrc;
        char *dig = (char *)ws + kquant_planes_offset(K, N);
        float *xd = (float *)(dig + dig_bytes);
        HIP_RET(ghip::quantize_q8_K_planes(x, K, N, ws, xd, q45 ? dig : nullptr, s));
        HIP_RET(q45   ? ghip::gemm_q45_K(type == KQuant::Q5_K, w, K, M, ws, xd, dig, N, y, ldy, g_dev[id].info, s)
                : q23 ? ghip::gemm_q23_K(type == KQuant::Q3_K, w, K, M, ws, xd, N, y, ldy, g_dev[id].info, s)
                      : ghip::gemm_q6_K(w, K, M, ws, xd, N, y, ldy, g_dev[id].info, s));
        return GGML_HIP_OK;
    }
    const int wrc = quantize_q8k_ws(id, x, K, N, s, &ws);
    if (wrc != GGML_HIP_OK) return wrc;
    HIP_RET(q45   ? ghip::mm_exact_q45_K(type == KQuant::Q5_K, w, K, M, ws, N, y, ldy, s)
            : q23 ? ghip::mm_exact_q23_K(type == KQuant::Q3_K, w, K, M, ws, N, y, ldy, s)
                  : ghip::mm_exact_q6_K(w, K, M, ws, N, y, ldy, s));
    return GGML_HIP_OK;
}
static int mul_mat_q6k_dev(const void *w, int64_t K, int64_t M, const float *x, int64_t N, float *y, int64_t ldy, int algo,
                           hipStream_t s) {
    return mul_mat_kquant_dev(ROW_Q6_K, KQuant::Q6_K, w, K, M, x, N, y, ldy, algo, s);
}
static int mul_mat_q5k_dev(const void *w, int64_t K, int64_t M, const float *x, int64_t N, float *y, int64_t ldy, int algo,
                           hipStream_t s) {
    return mul_mat_kquant_dev(ROW_Q5_K, KQuant::Q5_K, w, K, M, x, N, y, ldy, algo, s);
}
static int mul_mat_q4k_dev(const void *w, int64_t K, int64_t M, const float *x, int64_t N, float *y, int64_t ldy, int algo,
                           hipStream_t s) {
    return mul_mat_kquant_dev(ROW_Q4_K, KQuant::Q4_K, w, K, M, x, N, y, ldy, algo, s);
}
static int mul_mat_q3k_dev(const void *w, int64_t K, int64_t M, const float *x, int64_t N, float *y, int64_t ldy, int algo,
                           hipStream_t s) {
    return mul_mat_kquant_dev(ROW_Q3_K, KQuant::Q3_K, w, K, M, x, N, y, ldy, algo, s);
}
static int mul_mat_q2k_dev(const void *w, int64_t K, int64_t M, const float *x, int64_t N, float *y, int64_t ldy, int algo,
                           hipStream_t s) {
    return mul_mat_kquant_dev(ROW_Q2_K, KQuant::Q2_K, w, K, M, x, N, y, ldy, algo, s);
}

// Q8_0 / Q4_1 / Q5_0 / Q5_1 (blk32_w.hip), one body over the four rows.  mn: the type has a minimum and q8_1
// activations (Q4_1, Q5_1); the other two multiply against q8_0.  algo 2 (Q8_0 and Q5_0) = the weight's k_gemm8 image
// built per call into the workspace (k_prep8_w: the int8 weights verbatim, or q - 16; the way GEMM version 9 treats
// an unregistered q4_0 weight; ggml_hip_reserve_workspace_mm budgets its 34 B per 32 weights), then gemm8_prep_x +
// gemm8_run unchanged; algo 4 = the SoA quantizer (q8_0's planes; q8_1's qs, d and s for the types with a minimum,
// workspace_bytes_q81) + the exact kernel; algo 7 (the types with a minimum only, any N >= 1, no K limit) = the same
// q8_1 planes + k_gemm_q5x1 on the weights in place (q5x_gemm.hip)
size_t workspace_bytes_q81(int64_t K, int64_t N) { return ws_d16_offset(K, N) + ws_d_bytes(K, N); }
enum class Blk32 { Q8_0, Q4_1, Q5_0, Q5_1 };
static int mul_mat_blk32_dev(const WeightType &t, Blk32 type, const void *w, int64_t K, int64_t M, const float *x, int64_t N,
                             float *y, int64_t ldy, int algo, hipStream_t s) {
    const bool q8 = type == Blk32::Q8_0, mn = type == Blk32::Q4_1 || type == Blk32::Q5_1;
    const bool qh = type == Blk32::Q5_0 || type == Blk32::Q5_1;
    const int rc = check_operands(t, w, K, M, x, N, y, ldy);
    if (rc != GGML_HIP_OK || N == 0) return rc;
    const int id = current_device();
    if (algo == 0) algo = auto_algo(t, K, N);
    if (algo == 1) {
        if (!t.gemv_takes_k(K)) return fail(GGML_HIP_ERR_UNSUPPORTED, t.err_gemv_k);
        HIP_RET(q8 ? ghip::gemv_q8_0w(w, K, M, x, N, y, ldy, g_dev[id].info, s)
                   : ghip::gemv_q5x(qh, mn, w, K, M, x, N, y, ldy, g_dev[id].info, s));
        return GGML_HIP_OK;
    }
    if (algo != 4 && algo != (mn ? 7 : 2))
        return fail(GGML_HIP_ERR_INVALID, mn ? "algo must be 0, 1, 4 or 7" : "algo must be 0, 1, 2 or 4");
    if (algo == 7 && too_many_tiles(M, N)) return fail(GGML_HIP_ERR_UNSUPPORTED, ERR_TILES);
    void *ws = nullptr;
    if (algo == 2) {
        if ((N + 7) / 8 > 65535) return fail(GGML_HIP_ERR_UNSUPPORTED, "too many columns for one launch; split columns");
        const int wrc = stream_workspace(id, s, workspace_bytes_mm(K, N, M), &ws);
        if (wrc != GGML_HIP_OK) return wrc;
        void *xws = (char *)ws + ws_g8x_offset(K, N), *wws = (char *)ws + ws_g8w_offset(K, N);
        HIP_RET(ghip::gemm8_prep_x(x, K, N, xws, s));
        HIP_RET(q8 ? ghip::gemm8_prep_w_q8_0(w, K, M, wws, s) : ghip::gemm8_prep_w_q5_0(w, K, M, wws, s));
        HIP_RET(ghip::gemm8_run(wws, K, M, xws, N, y, ldy, s));
        return GGML_HIP_OK;
    }
    const int wrc = stream_workspace(id, s, mn ? workspace_bytes_q81(K, N) : workspace_bytes(K, N), &ws);
    if (wrc != GGML_HIP_OK) return wrc;
    const XPlanes xp = x_planes(ws, K, N);
    if (mn)
        HIP_RET(ghip::quantize_q8_1_soa(x, K, N, xp.qs, xp.d, xp.s, s));
    else
        HIP_RET(ghip::quantize_q8_0_soa(x, K, N, xp.qs, xp.d, s));
    if (algo == 7)
        HIP_RET(ghip::gemm_q5x1(qh, w, K, M, xp.qs, xp.d, xp.s, N, y, ldy, g_dev[id].info, s));
    else if (q8)
        HIP_RET(ghip::mm_exact_q8_0w(w, K, M, xp.qs, xp.d, N, y, ldy, s));
    else
        HIP_RET(ghip::mm_exact_q5x(qh, mn, w, K, M, xp.qs, xp.d, xp.s, N, y, ldy, s));
    return GGML_HIP_OK;
}
static int mul_mat_q8_0_dev(const void *w, int64_t K, int64_t M, const float *x, int64_t N, float *y, int64_t ldy, int algo,
                            hipStream_t s) {
    return mul_mat_blk32_dev(ROW_Q8_0, Blk32::Q8_0, w, K, M, x, N, y, ldy, algo, s);
}
static int mul_mat_q4_1_dev(const void *w, int64_t K, int64_t M, const float *x, int64_t N, float *y, int64_t ldy, int algo,
                            hipStream_t s) {
    return mul_mat_blk32_dev(ROW_Q4_1, Blk32::Q4_1, w, K, M, x, N, y, ldy, algo, s);
}
static int mul_mat_q5_0_dev(const void *w, int64_t K, int64_t M, const float *x, int64_t N, float *y, int64_t ldy, int algo,
                            hipStream_t s) {
    return mul_mat_blk32_dev(ROW_Q5_0, Blk32::Q5_0, w, K, M, x, N, y, ldy, algo, s);
}
static int mul_mat_q5_1_dev(const void *w, int64_t K, int64_t M, const float *x, int64_t N, float *y, int64_t ldy, int algo,
                            hipStream_t s) {
    return mul_mat_blk32_dev(ROW_Q5_1, Blk32::Q5_1, w, K, M, x, N, y, ldy, algo, s);
}

// F16 (f16_w.hip, ggml_ops.hip): algo 1 = k_gemv_f16w in column tiles; algo 4 = op_mul_mat_f16_f32's bitwise kernels
// (ggml_vec_dot_f16 in its AVX2 / F16C schedule) and algo 9 = its MFMA kernel, both on contiguous strides.  Those
// launchers write y as [N][M] with no row pitch, so 4 and 9 take ldy == M only (the hook never passes another).
// Algo 11 = k_gemm_f16w (f16_w_gemm.hip) on the fp16 image of x in the workspace: any ldy >= M, any K % 32 == 0.  An
// algo the type rejects is refused before anything else, an empty call included.
static int mul_mat_f16w_dev(const void *w, int64_t K, int64_t M, const float *x, int64_t N, float *y, int64_t ldy, int algo,
                            hipStream_t s) {
    if (algo != 0 && algo != 1 && algo != 4 && algo != 9 && algo != 11)
        return fail(GGML_HIP_ERR_INVALID, "algo must be 0, 1, 4, 9 or 11");
    const WeightType &t = ROW_F16;
    const int rc = check_operands(t, w, K, M, x, N, y, ldy);
    if (rc != GGML_HIP_OK || N == 0) return rc;
    const int id = current_device();
    if (algo == 0) algo = auto_algo_f16w(K, M, N);
    if (algo == 1) {
        if (!t.gemv_takes_k(K)) return fail(GGML_HIP_ERR_UNSUPPORTED, t.err_gemv_k);
        HIP_RET(ghip::gemv_f16w(w, K, M, x, N, y, ldy, g_dev[id].info, s));
        return GGML_HIP_OK;
    }
    if (algo == 11) {
        if (!ghip::gemm_f16w_supported(K, M, N))
            return fail(GGML_HIP_ERR_UNSUPPORTED, "too many tiles for one grid of the F16 GEMM (algo 11); split rows or columns");
        void *ws = nullptr;
        const size_t need = workspace_bytes_f16w_gemm(id, K, N, M);
        const int wrc = stream_workspace(id, s, need, &ws);
        if (wrc != GGML_HIP_OK) return wrc;
        HIP_RET(ghip::gemm_f16w(w, K, M, x, N, y, ldy, ws, need, g_dev[id].info, s));
        return GGML_HIP_OK;
    }
    if (ldy != M) return fail(GGML_HIP_ERR_UNSUPPORTED, "the exact and MFMA F16 kernels (algo 4, 9) need ldy == M");
    HIP_RET(ghip::op_mul_mat_f16_f32(w, x, y, (int)K, M, N, 1, K * 2, M * K * 2, K * 4, N * K * 4, s, nullptr,
                                     algo == 4 ? -1 : 2));
    return GGML_HIP_OK;
}

// F32 (f32_w.hip, f32_w_gemm.hip): algo 1 = k_gemv_f32w in column tiles, algo 4 = k_mm_exact_f32w (ggml_vec_dot_f32's
// AVX2 schedule, bitwise), algo 12 = k_gemm_f32w on v_mfma_f32_32x32x2_f32 with its K-slice slabs in the workspace.
// Every algo takes any ldy >= M.  An algo the type rejects is refused before anything else, an empty call included.
static int mul_mat_f32w_dev(const void *w, int64_t K, int64_t M, const float *x, int64_t N, float *y, int64_t ldy, int algo,
                            hipStream_t s) {
    if (algo != 0 && algo != 1 && algo != 4 && algo != 12) return fail(GGML_HIP_ERR_INVALID, "algo must be 0, 1, 4 or 12");
    const WeightType &t = ROW_F32;
    const int rc = check_operands(t, w, K, M, x, N, y, ldy);
    if (rc != GGML_HIP_OK || N == 0) return rc;
    const int id = current_device();
    if (algo == 0) algo = auto_algo_f32w(K, M, N);
    if (algo == 1) {
        if (!t.gemv_takes_k(K)) return fail(GGML_HIP_ERR_UNSUPPORTED, t.err_gemv_k);
        HIP_RET(ghip::gemv_f32w(w, K, M, x, N, y, ldy, g_dev[id].info, s));
        return GGML_HIP_OK;
    }
    if (algo == 12) {
        if (!ghip::gemm_f32w_supported(K, M, N))
            return fail(GGML_HIP_ERR_UNSUPPORTED, "too many tiles for one grid of the F32 GEMM (algo 12); split rows or columns");
        void *ws = nullptr;
        const size_t need = workspace_bytes_f32w_gemm(id, K, N, M);
        if (need) {
            const int wrc = stream_workspace(id, s, need, &ws);
            if (wrc != GGML_HIP_OK) return wrc;
        }
        HIP_RET(ghip::gemm_f32w(w, K, M, x, N, y, ldy, ws, need, g_dev[id].info, s));
        return GGML_HIP_OK;
    }
    if (N * M * 32 / 256 + 1 >= ((int64_t)1 << 31))
        return fail(GGML_HIP_ERR_UNSUPPORTED, "too many outputs for one grid of the exact F32 kernel; split rows or columns");
    HIP_RET(ghip::mm_exact_f32w(w, K, M, x, N, y, ldy, s));
    return GGML_HIP_OK;
}

// Sibling matrices (one x) that all take k_gemm9 on a registered fp6 image: ONE launch over their
// row tiles (the x image built once, as before).  The launch plans its tiles (128 x 128 / 128 x 64 /
// mixed, half tiles) from its own total tile count, which can differ from the per-matrix launches'
// plans: y is within the oracle bound of the separate calls, and bitwise equal to them only with the
// tile pinned (ggml_hip_debug_set_gemm9_wide 0 or 1; include/ggml-hip.h).
// Returns 1 when the group does not qualify (the caller runs one launch per matrix).
bool g9_images(int n, const void *const *w, const int64_t *M, int64_t K, int64_t N, const void **img) {
    static const bool grp = !getenv("GGML_HIP_GEMM9_GROUP") || atoi(getenv("GGML_HIP_GEMM9_GROUP")) != 0;
    if ((n > 1 && !grp) || n < 1 || n > 4 || exact_mode() || gemm_version() != 10 || K <= 0 || K % 64 != 0 ||
        N <= ghip::gemv_max_tokens(K) || N * K >= ((int64_t)1 << 31))
        return false;
    const int id = current_device();
    for (int i = 0; i < n; i++) {
        int fmt = 0;
        img[i] = wimage_find(id, w[i], K, M[i], &fmt);
        // mul_mat_dev's algo rule: the image GEMM above 128 tokens, or above IMG_MIN_N / for tall
        // matrices when an image exists
        if (!img[i] || fmt != 9 || !(N > 128 || N > IMG_MIN_N || M[i] >= IMG_MIN_M)) return false;
        if (M[i] * (K / QK) * Q4B >= ((int64_t)1 << 31) || M[i] >= (1 << 30)) return false;
    }
    return true;
}

int mul_mat_group_g9(int n, const void *const *w, const int64_t *M, int64_t K, const float *x, int64_t N,
                     float *const *y, hipStream_t s) {
    const void *img[4];
    if (n < 2 || !x || !aligned(x, 16) || !g9_images(n, w, M, K, N, img)) return 1;
    const int id = current_device();
    int64_t ldy[4];
    for (int i = 0; i < n; i++) ldy[i] = M[i];
    void *ws = nullptr;
    const int wrc = stream_workspace(id, s, workspace_bytes_mm(K, N, 0), &ws);
    if (wrc != GGML_HIP_OK) return wrc;
    void *xws = (char *)ws + ws_g8x_offset(K, N);
    HIP_RET(ghip::gemm9_prep_x(x, K, N, xws, s));
    HIP_RET(ghip::gemm9_run_multi(n, img, M, K, xws, N, y, ldy, s));
    return GGML_HIP_OK;
}

// ------------------------------------------------------------------------------------------
// tensor helpers

bool is_contiguous(const tensor *t) {
    const size_t ts = gabi::type_size(t->type);
    const int bs = gabi::blck_size(t->type);
    return t->nb[0] == ts && t->nb[1] == t->nb[0] * t->ne[0] / bs && t->nb[2] == t->nb[1] * t->ne[1] &&
           t->nb[3] == t->nb[2] * t->ne[2];
}

bool on_device(const tensor *t) {
    return t && (t->backend == gabi::BACKEND_GPU || t->backend == gabi::BACKEND_GPU_SPLIT);
}

void split_range(int64_t nrows, int id, int64_t *lo, int64_t *hi) {
    // ggml-cuda.cu:2361-2368 / 2779-2786
    *lo = split_row_low(nrows, g_tensor_split, id);
    *hi = id == g_device_count - 1 ? nrows : split_row_low(nrows, g_tensor_split, id + 1);
}

bool supported_mul_mat(const tensor *src0, const tensor *src1, const tensor *dst) {
    return src0 && src1 && dst && src0->type == gabi::TYPE_Q4_0 && src1->type == gabi::TYPE_F32 &&
           dst->type == gabi::TYPE_F32 && src0->ne[0] % 64 == 0 && src0->ne[0] == src1->ne[0] &&
           dst->ne[0] == src0->ne[1] && dst->ne[1] == src1->ne[1] && src0->ne[2] == src1->ne[2] &&
           src0->ne[3] == src1->ne[3] && is_contiguous(src0) && is_contiguous(src1) && is_contiguous(dst);
}

// contiguous <type> x F32 -> F32 for a type with a row in weight_type()'s table.  Kept apart from supported_mul_mat,
// which gates everything q4_0-only (the q4_0 kernels, weight images, sibling groups, chains and the engine), so
// that no node of another type reaches those.  It looks at the operands only, not at the Q4_K switch.
bool supported_mul_mat_type(int type, const tensor *src0, const tensor *src1, const tensor *dst) {
    const WeightType *t = weight_type(type);
    return t && src0 && src1 && dst && src0->type == type && src1->type == gabi::TYPE_F32 &&
           dst->type == gabi::TYPE_F32 && src0->ne[0] > 0 && src0->ne[0] % t->k_granule == 0 &&
           src0->ne[0] == src1->ne[0] && dst->ne[0] == src0->ne[1] && dst->ne[1] == src1->ne[1] &&
           src0->ne[2] == src1->ne[2] && src0->ne[3] == src1->ne[3] && is_contiguous(src0) && is_contiguous(src1) &&
           is_contiguous(dst);
}

// Q4_K on the hook path is opt-in: GGML_HIP_Q4_K=1 or ggml_hip_debug_set_q4_K
std::atomic<int> g_q4k{-1};
bool q4k_enabled() {
    int v = g_q4k.load(std::memory_order_relaxed);
    if (v < 0) {
        const char *e = getenv("GGML_HIP_Q4_K");
        int want = (e && atoi(e) != 0) ? 1 : 0, expect = -1;
        g_q4k.compare_exchange_strong(expect, want);
        v = g_q4k.load(std::memory_order_relaxed);
    }
    return v != 0;
}
int q4k_set_enabled(int on) {
    const int prev = q4k_enabled() ? 1 : 0;
    g_q4k.store(on ? 1 : 0, std::memory_order_relaxed);
    return prev;
}

// The hook path's two questions about a weight type.  With the Q4_K switch off every entry point treats a
// host-resident Q4_K tensor as a type no device op reads; a Q4_K weight that transform_tensor uploaded while the
// switch was on keeps being served after it is turned off: its data is on the device, so ggml's CPU op could not
// read it.  The switch decides for all-host nodes only: in an offloaded layer of a Q4_K file the matrix stays on
// transform_tensor's host copy while src1 and dst are device tensors (llama.cpp's offload_func), and ggml.c's CPU
// mul_mat asserts host operands (ggml.c:15650), so such a node is served like any host weight of a served type
// (mul_mat_node's residency cache / upload branch), as the reference's backend never declines once an operand is on
// the device.
bool f16_weight(const tensor *t) {
    return t && t->type == gabi::TYPE_F16 && t->op == gabi::OP_NONE && t->ne[2] == 1 && t->ne[3] == 1 && t->ne[0] > 0 &&
           t->ne[0] % ROW_F16.k_granule == 0 && is_contiguous(t);
}
// F32 weights: a contiguous 2-D F32 leaf with K % 32 == 0.  All-host F32 mul_mats are taken only with this switch on
// (GGML_HIP_F32_W=1 / ggml_hip_debug_set_f32_w; default off: the small F32 matrices of the arch frontends stay on
// ggml's CPU op); a matrix transform_tensor uploaded, or a host one between device operands, is served regardless,
// like Q4_K with its switch off.
std::atomic<int> g_f32w{-1};
bool f32w_enabled() {
    int v = g_f32w.load(std::memory_order_relaxed);
    if (v < 0) {
        const char *e = getenv("GGML_HIP_F32_W");
        int want = (e && atoi(e) != 0) ? 1 : 0, expect = -1;
        g_f32w.compare_exchange_strong(expect, want);
        v = g_f32w.load(std::memory_order_relaxed);
    }
    return v != 0;
}
int f32w_set_enabled(int on) {
    const int prev = f32w_enabled() ? 1 : 0;
    g_f32w.store(on ? 1 : 0, std::memory_order_relaxed);
    return prev;
}
bool f32_weight(const tensor *t) {
    return t && t->type == gabi::TYPE_F32 && t->op == gabi::OP_NONE && t->ne[2] == 1 && t->ne[3] == 1 && t->ne[0] > 0 &&
           t->ne[0] % ROW_F32.k_granule == 0 && is_contiguous(t);
}
bool hook_takes_type(int type) {
    if (type == gabi::TYPE_F32) return f32w_enabled();
    return type == gabi::TYPE_Q4_0 || (weight_type(type) && (type != gabi::TYPE_Q4_K || q4k_enabled()));
}
int hook_weight_type(const tensor *src0, const tensor *src1, const tensor *dst) {
    if (supported_mul_mat(src0, src1, dst)) return gabi::TYPE_Q4_0;
    if (!src0 || !supported_mul_mat_type(src0->type, src0, src1, dst)) return gabi::TYPE_COUNT;
    // an F16 src0 is a weight only as a 2-D leaf: the K and V views of the attention (permuted, transposed, 3-D, never
    // leaves) keep the F16 x F32 device op and its fusions
    if (src0->type == gabi::TYPE_F16 && !f16_weight(src0)) return gabi::TYPE_COUNT;
    // an F32 src0 likewise (an F32 KV cache's views, activations); off the switch an all-host node is ggml's
    if (src0->type == gabi::TYPE_F32 &&
        (!f32_weight(src0) || (!f32w_enabled() && !(on_device(src0) && src0->extra) && !on_device(src1) && !on_device(dst))))
        return gabi::TYPE_COUNT;
    if (src0->type == gabi::TYPE_Q4_K && !q4k_enabled() && !(on_device(src0) && src0->extra) && !on_device(src1) &&
        !on_device(dst))
        return gabi::TYPE_COUNT;
    return src0->type;
}

[[noreturn]] void op_abort(const tensor *t, const char *why) {
    // the reference asserts the same way (GGML_ASSERT in ggml-cuda.cu's op wrappers): a node that
    // reaches a device op must be computable there, ggml.c cannot fall back once an operand is on
    // the device (ggml.c:15650)
    fprintf(stderr, "ggml_hip_compute_forward: op %d (%s): %s\n", t->op, t->name, why);
    abort();
}

}  // namespace ghh
