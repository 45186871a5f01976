// launch.h — every kernel launch of libggml_hip.so goes through ghip::launch_k.
//
// Eager by default (hipLaunchKernel).  While the launch recorder is active on the stream (full
// offload through ggml_hip_compute_forward, one device: a decode eval issues ~375 small launches
// at ~2.6 us of host time each, measured by tools/host_costs2.hip), a launch is only recorded
// (function, grid, block, LDS bytes, a copy of the argument values); the recorded run is submitted
// as one HIP graph at the next sync point (any memcpy / event / synchronize / free of the backend,
// ggml-hip-graph.cpp).  A run with the same kernels as a cached graph is submitted by updating the
// nodes whose grid or arguments changed (hipGraphExecKernelNodeSetParams, ~0.6 us per changed node)
// and one hipGraphLaunch (~0.03 us per kernel of host time).
#pragma once
#include <atomic>
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <new>
#include <type_traits>
#include <utility>

namespace ghip {

template <class T> struct type_tag { using type = T; };

// true while launches on s are recorded instead of issued
bool rec_active(hipStream_t s);
// launches recorded but not yet submitted
bool rec_pending();
// records one launch; args[i] points at the value of parameter i (copied before returning)
void rec_kernel(const void *fn, dim3 grid, dim3 block, size_t lds, hipStream_t s, int nargs, void *const *args,
                const size_t *sizes, const size_t *aligns);
// submits the recorded launches (no-op when none are pending); every backend HIP call that is not
// a kernel launch calls it first (GHIP_SYNC, ggml-hip-internal.h)
void rec_flush();
void rec_flush_at(const char *why);      // the same, naming the caller (GGML_HIP_TRACE_GRAPH=1 prints it)
// recording on / off for stream s (switching stream or turning it off submits what is pending)
void rec_enable(hipStream_t s, bool on);
// 1: runs submitted as cached HIP graphs; 2: a launcher thread issues the launches in order; 3: each launch
// goes straight into an own AQL queue (ggml-hip-aql.cpp)
void rec_set_mode(int mode);
// mode 3 (ggml-hip-aql.cpp): dispatch (false: the caller launches through HIP), drain, pending, HIP-work marker
bool aql_dispatch(const void *fn, dim3 grid, dim3 block, size_t lds, hipStream_t s, int nargs, void *const *args,
                  const size_t *sizes, const size_t *aligns);
void aql_drain();
bool aql_pending();
void aql_stream_dirty();
void aql_fallback_counted();
void aql_counts(long long *out);   // dispatches, fallbacks, drains, stream syncs
// counters: submitted runs, kernels in them, nodes updated in place, graphs instantiated, host ns
// spent submitting (mode 2: waits for the launcher thread to drain, and the ns spent waiting)
void rec_stats(long long *runs, long long *kernels, long long *updated, long long *built, long long *submit_ns);
// submits what is pending and destroys every cached graph
void rec_clear_cache();
// host-cost profile of eager launches (ggml_hip_debug_launch_stats): count and ns inside hipLaunchKernel
extern std::atomic<bool> g_launch_prof;   // read by the launcher thread, written by the API
void launch_prof_add(long long ns);
long long launch_prof_now();
void launch_prof_read(long long *count, long long *ns, bool reset);
// diagnostic (GGML_HIP_LAUNCH_PAD_NS): a busy wait of this many ns after every eager launch, to measure how
// the end-to-end token time depends on the host's per-launch cost (tools/run.sh PARTS=e2e_pad)
extern std::atomic<int> g_launch_pad_ns;
void launch_pad();

template <typename... P, typename... A>
inline void launch_k(void (*k)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t s, A &&...a) {
    static_assert(sizeof...(P) == sizeof...(A), "launch_k: argument count");
    if (!rec_active(s)) {
        if (rec_pending()) rec_flush_at("eager launch");   // never overtakes recorded launches
        if (__builtin_expect(g_launch_prof.load(std::memory_order_relaxed), 0)) {
            const long long t0 = launch_prof_now();
            hipLaunchKernelGGL(k, grid, block, lds, s, std::forward<A>(a)...);
            launch_prof_add(launch_prof_now() - t0);
            return;
        }
        hipLaunchKernelGGL(k, grid, block, lds, s, std::forward<A>(a)...);
        if (__builtin_expect(g_launch_pad_ns.load(std::memory_order_relaxed) > 0, 0)) launch_pad();
        return;
    }
    // convert every argument to the parameter's exact type, then hand the recorder their addresses
    struct Holder {
        alignas(16) unsigned char raw[(sizeof(std::decay_t<P>) + ... + 0) + 16 * sizeof...(P) + 1];
    } h;
    void *ptrs[sizeof...(P) + 1];
    size_t sizes[sizeof...(P) + 1], aligns[sizeof...(P) + 1];
    size_t off = 0;
    int i = 0;
    auto put = [&](auto &&v, auto tag) {
        using T = typename decltype(tag)::type;
        static_assert(std::is_trivially_copyable<T>::value, "kernel arguments are copied bytewise");
        off = (off + alignof(T) - 1) & ~(alignof(T) - 1);
        new (h.raw + off) T(static_cast<T>(v));
        ptrs[i] = h.raw + off;
        sizes[i] = sizeof(T);
        aligns[i] = alignof(T);
        off += sizeof(T);
        i++;
    };
    (put(std::forward<A>(a), type_tag<std::decay_t<P>>{}), ...);
    rec_kernel((const void *)k, grid, block, lds, s, (int)sizeof...(P), ptrs, sizes, aligns);
}

// ---- launch scaffolding shared by the kernel files' host halves

// hipFuncAttributeMaxDynamicSharedMemorySize of Kernel raised to `bytes`, once per device: every instantiation
// has its own flag word, one bit per device (16 max), thread-safe
template <auto Kernel>
inline hipError_t raise_dynamic_lds(int bytes) {
    static std::atomic<uint32_t> done{0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev > 15) dev = 0;
    if (done.load(std::memory_order_acquire) & (1u << dev)) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute((const void *)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess) done.fetch_or(1u << dev, std::memory_order_acq_rel);
    return e;
}

// the columns per workgroup (64, 128 or 256) of the int8-MFMA GEMMs that decode 64 weight rows in place per
// workgroup.  One workgroup per CU (LDS), and with fit_rule a workgroup's time is mostly its per-superblock load and
// decode, not its MFMAs: 256 columns only where the grid of 128-column tiles would not fit on the device at once
// (256 CUs where the count is unknown).  Without it, 256 columns for every N > 128.  y does not depend on the choice.
inline int gemm_tile_columns(int64_t M, int64_t N, int num_cus, bool fit_rule) {
    if (N <= 64) return 64;
    if (N <= 128) return 128;
    const int64_t grid128 = ((M + 63) / 64) * ((N + 127) / 128);
    return fit_rule && grid128 <= (int64_t)(num_cus > 0 ? num_cus : 256) ? 128 : 256;
}

// the 1-D launch of a quantizer or dequantizer: blocks of 256 threads, `per_block` of the `items` each; nothing
// to do is success
template <typename... P, typename... A>
inline hipError_t launch_1d(void (*k)(P...), int64_t items, int per_block, hipStream_t s, A &&...a) {
    if (items == 0) return hipSuccess;
    (void)hipGetLastError();  // report only this launch's error
    launch_k(k, dim3((unsigned)((items + per_block - 1) / per_block)), dim3(256), 0, s, std::forward<A>(a)...);
    return hipGetLastError();
}

// a GEMV's run-time token tile nt in 1 .. 8 as a template argument: f(std::integral_constant<int, nt>)
template <class F>
inline hipError_t with_token_tile(int nt, F &&f) {
    switch (nt) {
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 3: return f(std::integral_constant<int, 3>{});
        case 4: return f(std::integral_constant<int, 4>{});
        case 5: return f(std::integral_constant<int, 5>{});
        case 6: return f(std::integral_constant<int, 6>{});
        case 7: return f(std::integral_constant<int, 7>{});
        case 8: return f(std::integral_constant<int, 8>{});
    }
    return hipErrorInvalidValue;
}

// any N through a GEMV of at most `tile` tokens per launch: f(n0, nt) on the column tiles in order, up to the
// first error (each tile is exactly the call on those columns)
template <class F>
inline hipError_t for_column_tiles(int64_t N, int tile, F &&f) {
    for (int64_t n0 = 0; n0 < N; n0 += tile) {
        const hipError_t e = f(n0, (int)(N - n0 < tile ? N - n0 : tile));
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// an exact kernel's columns on grid.y, at most 65535 per launch: launch(n0, nn) issues columns [n0, n0 + nn)
template <class F>
inline hipError_t launch_column_chunks(int64_t N, F &&launch) {
    (void)hipGetLastError();  // report only these launches' error
    for (int64_t n0 = 0; n0 < N; n0 += 65535) launch(n0, (unsigned)(N - n0 < 65535 ? N - n0 : 65535));
    return hipGetLastError();
}

}  // namespace ghip
