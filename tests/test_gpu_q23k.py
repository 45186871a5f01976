"""Q3_K / Q2_K x F32 mul_mat on the device (csrc/q23_k.hip): the dequantizers bit for bit, the fused GEMV within
the parity bound and bitwise the numpy restatement of its own schedule, column tiling, exact mode bit-identical to
the reference's AVX2 ggml_vec_dot_q3_K_q8_K / ggml_vec_dot_q2_K_q8_K, graph capture, status codes, and the ggml hook
path on hand-built tensors (both types served by default).  References: the fixtures the compiled reference wrote
(tests/golden/q3k_*, q2k_*) and their numpy restatement tests/q23k_ref.py.  Q3_K rows of an odd number of
superblocks (K = 256, 768, 2304 with M > 1) put every second row at 2 mod 4."""
import ctypes

import numpy as np
import pytest

import q23k_ref as R
from golden_io import load
from hip_env import ggml_hip, gpu_available
from parity import check_y
from test_q23k_ref import TYPES, bits

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason="needs a HIP device and libggml_hip.so")]

DB = ggml_hip.DeviceBuffer
BOTH = pytest.mark.parametrize("variant", ["q3k", "q2k"])
GTYPE = {"q3k": ggml_hip.GGML_TYPE_Q3_K, "q2k": ggml_hip.GGML_TYPE_Q2_K}


def q3_of(variant):
    return TYPES[variant][0]


def assert_bitwise(got, ref):
    diff = np.flatnonzero(bits(got).ravel() != bits(ref).ravel())
    assert diff.size == 0, f"{diff.size} of {got.size} differ; first at {diff[:4]}: {np.ravel(got)[diff[:4]]} vs " \
                           f"{np.ravel(ref)[diff[:4]]}"


def rng_for(*key):
    return np.random.default_rng([0x23, *key])


def gpu_mul_mat(variant, wq, K, x, algo=0, ldy=None, fill=None):
    M, N = wq.shape[0], x.shape[0]
    ld = M if ldy is None else ldy
    wd, xd = DB.from_array(np.ascontiguousarray(wq)), DB.from_array(x)
    y0 = np.full((N, ld), np.float32(0 if fill is None else fill), np.float32)
    yd = DB.from_array(y0)
    f = ggml_hip.mul_mat_q3_K if q3_of(variant) else ggml_hip.mul_mat_q2_K
    f(wd, K, M, xd, N, yd, algo=algo, ldy=ld)
    return yd.download((N, ld), np.float32)


def gpu_dequantize(variant, wq, K):
    M = wq.shape[0]
    wd, od = DB.from_array(np.ascontiguousarray(wq)), DB(M * K * 4)
    (ggml_hip.dequantize_q3_K if q3_of(variant) else ggml_hip.dequantize_q2_K)(wd, K, M, od)
    return od.download((M, K), np.float32)


@pytest.fixture
def exact_off():
    L = ggml_hip.load()
    prev = L.ggml_hip_get_exact()
    L.ggml_hip_set_exact(0)
    yield L
    L.ggml_hip_set_exact(prev)


@pytest.fixture
def hook(request, exact_off):
    """(L, variant) for the hook-path tests: both types are served as the backend stands, no switch"""
    return exact_off, request.param


HOOK_BOTH = pytest.mark.parametrize("hook", ["q3k", "q2k"], indirect=True)


# ---- dequantize -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant,K", [(v, K) for v, (_, _, ks) in TYPES.items() for K in ks])
def test_dequantize_fixture_bitwise(variant, K):
    ref = load(variant, f"w{K}_dequant")
    wq = load(variant, f"w{K}_{TYPES[variant][1]}")[:ref.shape[0]]
    assert_bitwise(gpu_dequantize(variant, wq, K), ref)


@BOTH
@pytest.mark.parametrize("K,M", [(K, M) for K in (256, 2304) for M in (1, 7)])
def test_dequantize_random_bitwise(variant, K, M):
    q3 = q3_of(variant)
    wq = R.random_q23_K(rng_for(1, q3, K, M), M, K, q3)
    assert_bitwise(gpu_dequantize(variant, wq, K), R.dequantize(wq, K, q3))


# ---- fast GEMV --------------------------------------------------------------------------------------------

@BOTH
@pytest.mark.parametrize("K,M", [(K, M) for K in (256, 512, 768, 2304, 4096) for M in (1, 17, 100, 1000)])
def test_gemv_within_parity_bound(exact_off, variant, K, M):
    """N = 1, 2, 8 on the same weights; the bound is parity.check_y's default, 1e-3 |y| + 1e-6 S_abs with S_abs
    over superblocks.  K = 256: one superblock, three quarters of a step idle; K = 768, 2304: odd superblock count,
    so every second Q3_K row sits at 2 mod 4; M = 1, 17: ragged waves."""
    q3 = q3_of(variant)
    rng = rng_for(2, q3, K, M)
    wq = R.random_q23_K(rng, M, K, q3)
    x = rng.standard_normal((8, K)).astype(np.float32)
    y_ref, s_abs = R.block_terms(wq, R.quantize_q8_K(x), K, q3)
    for N in (1, 2, 8):
        y = gpu_mul_mat(variant, wq, K, x[:N], algo=1)
        check_y(y, y_ref[:N], s_abs[:N])


@BOTH
def test_gemv_lds_image_above_64k(exact_off, variant):
    """K = 16384, N = 8: the largest q8_K image of x, 149,504 bytes of dynamic LDS for Q2_K (the sub-block sums as
    int16) and 133,120 for Q3_K"""
    q3 = q3_of(variant)
    K, M, N = 16384, 33, 8
    rng = rng_for(3, q3)
    wq = R.random_q23_K(rng, M, K, q3)
    x = rng.standard_normal((N, K)).astype(np.float32)
    y_ref, s_abs = R.block_terms(wq, R.quantize_q8_K(x), K, q3)
    check_y(gpu_mul_mat(variant, wq, K, x, algo=1), y_ref, s_abs)


@BOTH
@pytest.mark.parametrize("K,N", [(K, N) for K in (256, 768, 2304) for N in (1, 8)])
def test_gemv_bitwise_own_schedule(exact_off, variant, K, N):
    """the exact integer sums and the kernel's fp32 order, not only a bound"""
    q3 = q3_of(variant)
    M = 37
    rng = rng_for(4, q3, K, N)
    wq = R.random_q23_K(rng, M, K, q3)
    x = rng.standard_normal((N, K)).astype(np.float32)
    assert_bitwise(gpu_mul_mat(variant, wq, K, x, algo=1), R.gemv_schedule(wq, x, K, q3))


# ---- column tiling ----------------------------------------------------------------------------------------

@BOTH
@pytest.mark.parametrize("N", [9, 17, 33])
def test_column_tiles_bitwise_per_tile_calls(exact_off, variant, N):
    q3 = q3_of(variant)
    K, M = 512, 37
    rng = rng_for(5, q3, N)
    wq = R.random_q23_K(rng, M, K, q3)
    x = rng.standard_normal((N, K)).astype(np.float32)
    y = gpu_mul_mat(variant, wq, K, x, algo=1)
    for n0 in range(0, N, 8):
        assert_bitwise(y[n0:n0 + 8], gpu_mul_mat(variant, wq, K, x[n0:n0 + 8], algo=1))
    assert_bitwise(y, gpu_mul_mat(variant, wq, K, x, algo=0))         # auto = GEMV outside exact mode


@BOTH
@pytest.mark.parametrize("algo", [1, 4])
def test_ldy_gap_untouched(exact_off, variant, algo):
    q3 = q3_of(variant)
    K, M, N, ld = 512, 37, 11, 48
    rng = rng_for(6, q3)
    wq = R.random_q23_K(rng, M, K, q3)
    x = rng.standard_normal((N, K)).astype(np.float32)
    y = gpu_mul_mat(variant, wq, K, x, algo=algo, ldy=ld, fill=-7.5)
    assert np.all(y[:, M:] == np.float32(-7.5))
    assert_bitwise(y[:, :M], gpu_mul_mat(variant, wq, K, x, algo=algo))


# ---- exact mode -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant,K", [(v, K) for v, (_, _, ks) in TYPES.items() for K in ks])
def test_exact_fixture_bitwise(exact_off, variant, K):
    wq, x, y = load(variant, f"w{K}_{TYPES[variant][1]}"), load(variant, f"x{K}_f32"), load(variant, f"y{K}_vec_dot")
    assert_bitwise(gpu_mul_mat(variant, wq, K, x, algo=4), y)
    assert_bitwise(gpu_mul_mat(variant, wq, K, x[:1], algo=4), y[:1])
    exact_off.ggml_hip_set_exact(1)
    assert_bitwise(gpu_mul_mat(variant, wq, K, x, algo=0), y)


@BOTH
@pytest.mark.parametrize("K,N", [(K, N) for K in (256, 2304, 4096) for N in (1, 3, 9)])
def test_exact_vs_ref_bitwise(exact_off, variant, K, N):
    q3 = q3_of(variant)
    M = 33
    rng = rng_for(7, q3, K, N)
    wq = R.random_q23_K(rng, M, K, q3)
    x = rng.standard_normal((N, K)).astype(np.float32)
    ref = R.vec_dot_avx2(wq, R.quantize_q8_K(x), K, q3)
    assert_bitwise(gpu_mul_mat(variant, wq, K, x, algo=4), ref)
    exact_off.ggml_hip_set_exact(1)
    assert_bitwise(gpu_mul_mat(variant, wq, K, x, algo=0), ref)


# ---- scaling ----------------------------------------------------------------------------------------------

@BOTH
@pytest.mark.parametrize("algo", [1, 4])
def test_doubling_x_doubles_y_bitwise(exact_off, variant, algo):
    """x -> 2x halves iscale exactly and leaves every integer unchanged, so y doubles bit for bit."""
    q3 = q3_of(variant)
    K, M, N = 2304, 50, 3
    rng = rng_for(8, q3)
    wq = R.random_q23_K(rng, M, K, q3, special=False)
    x = rng.standard_normal((N, K)).astype(np.float32)
    y1, y2 = gpu_mul_mat(variant, wq, K, x, algo=algo), gpu_mul_mat(variant, wq, K, 2 * x, algo=algo)
    assert_bitwise(y2, 2 * y1)


# ---- graph capture ----------------------------------------------------------------------------------------

@BOTH
def test_graph_capture_replays_gemv(exact_off, variant):
    q3 = q3_of(variant)
    K, M = 2304, 300
    rng = rng_for(9, q3)
    wq = R.random_q23_K(rng, M, K, q3)
    x = rng.standard_normal((1, K)).astype(np.float32)
    eager = gpu_mul_mat(variant, wq, K, x, algo=0)
    wd, xd, yd = DB.from_array(wq), DB.from_array(x), DB(M * 4)
    L = exact_off
    s = L.ggml_hip_default_stream()
    g = ggml_hip.Graph(s)
    with g:
        (ggml_hip.mul_mat_q3_K if q3 else ggml_hip.mul_mat_q2_K)(wd, K, M, xd, 1, yd, stream=s)
    for _ in range(2):
        ggml_hip.check(L.ggml_hip_memset(yd.ptr, 0xFF, M * 4, s))
        g.launch()
        ggml_hip.check(L.ggml_hip_stream_synchronize(s))
        assert_bitwise(yd.download((1, M), np.float32), eager)


# ---- status codes -----------------------------------------------------------------------------------------

@BOTH
def test_status_codes(exact_off, variant):
    L = exact_off
    mm = L.ggml_hip_mul_mat_q3_K if q3_of(variant) else L.ggml_hip_mul_mat_q2_K
    dq = L.ggml_hip_dequantize_q3_K if q3_of(variant) else L.ggml_hip_dequantize_q2_K
    b = DB(1 << 16)
    assert mm(b.ptr, 384, 4, b.ptr, 1, b.ptr, 4, 0, None) == ggml_hip.ERR_INVALID          # K % 256
    assert dq(b.ptr, 384, 1, b.ptr, None) == ggml_hip.ERR_INVALID
    assert mm(b.ptr, 256, 4, b.ptr, 1, b.ptr, 3, 0, None) == ggml_hip.ERR_INVALID          # ldy < M
    for algo in (2, 3, 5, 6, 7):
        assert mm(b.ptr, 256, 4, b.ptr, 1, b.ptr, 4, algo, None) == ggml_hip.ERR_INVALID
    assert mm(b.ptr + 2, 256, 4, b.ptr, 1, b.ptr, 4, 0, None) == ggml_hip.ERR_INVALID      # dev_w at 2 mod 4
    assert dq(b.ptr + 1, 256, 1, b.ptr, None) == ggml_hip.ERR_INVALID                      # rows not 2-byte aligned
    assert mm(b.ptr, 256, 4, b.ptr, 0, b.ptr, 4, 0, None) == ggml_hip.OK                   # N = 0
    for algo in (2, 3, 5, 6, 7, -1):
        assert mm(b.ptr, 256, 4, b.ptr, 0, b.ptr, 4, algo, None) == ggml_hip.ERR_INVALID   # the algo check comes first
    ggml_hip.check(L.ggml_hip_memset(b.ptr, 0, 1 << 16, None))
    assert mm(b.ptr + 4, 256, 4, b.ptr + 1024, 1, b.ptr + 8192, 4, 1, None) == ggml_hip.OK  # dev_w 4-byte aligned is enough
    assert mm(None, 256, 4, b.ptr, 1, b.ptr, 4, 0, None) == ggml_hip.ERR_INVALID
    assert mm(b.ptr, 256, 4, None, 1, b.ptr, 4, 0, None) == ggml_hip.ERR_INVALID
    assert mm(b.ptr, 256, 4, b.ptr, 1, None, 4, 0, None) == ggml_hip.ERR_INVALID
    assert mm(b.ptr, 256, 4, b.ptr + 4, 1, b.ptr, 4, 0, None) == ggml_hip.ERR_INVALID      # x not 16-byte aligned
    assert mm(b.ptr, 256, 4, b.ptr, 1, b.ptr + 2, 4, 0, None) == ggml_hip.ERR_INVALID      # y not 4-byte aligned
    assert mm(b.ptr, 16640, 4, b.ptr, 0, b.ptr, 4, 1, None) == ggml_hip.OK                 # K past the GEMV, nothing to run
    assert mm(b.ptr, 16640, 4, b.ptr, 1, b.ptr, 4, 1, None) == ggml_hip.ERR_UNSUPPORTED    # (refused before any launch)


# ---- hook path --------------------------------------------------------------------------------------------

def k_tensor(variant, wq, K, M, backend=ggml_hip.GGML_BACKEND_CPU):
    return ggml_hip.make_tensor(GTYPE[variant], (K, M), wq, backend=backend)


def mm_node(w, x_np, y_np):
    N, K = x_np.shape
    xt = ggml_hip.make_tensor(ggml_hip.GGML_TYPE_F32, (K, N), x_np)
    y = ggml_hip.make_tensor(ggml_hip.GGML_TYPE_F32, (y_np.shape[1], N), y_np)
    y.op = ggml_hip.GGML_OP_MUL_MAT
    y.src0 = ctypes.pointer(w)
    y.src1 = ctypes.pointer(xt)
    return y, xt


def forward(L, node):
    p = ggml_hip.GgmlComputeParams(ggml_hip.GGML_TASK_COMPUTE, 0, 1, 0, None)
    return L.ggml_hip_compute_forward(ctypes.byref(p), ctypes.byref(node))


def mul_mat_count(L):
    c = (ctypes.c_int64 * 68)()
    L.ggml_hip_debug_op_stats.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    L.ggml_hip_debug_op_stats(c, 68, 0)
    return c[ggml_hip.GGML_OP_MUL_MAT]


@HOOK_BOTH
def test_hook_host_tensors(hook):
    L, variant = hook
    q3 = q3_of(variant)
    K, M, N = 2304, 70, 40
    rng = rng_for(10, q3)
    wq = R.random_q23_K(rng, M, K, q3)
    x = rng.standard_normal((N, K)).astype(np.float32)
    y_np = np.zeros((N, M), np.float32)
    w = k_tensor(variant, wq, K, M)
    y, xt = mm_node(w, x, y_np)
    assert L.ggml_hip_can_mul_mat(ctypes.byref(w), ctypes.byref(xt), ctypes.byref(y))
    before = mul_mat_count(L)
    assert forward(L, y)
    assert mul_mat_count(L) == before + 1                      # op stats: one MUL_MAT per node
    assert_bitwise(y_np, gpu_mul_mat(variant, wq, K, x))
    L.ggml_hip_weight_cache_invalidate(wq.ctypes.data_as(ctypes.c_void_p), wq.nbytes)


@HOOK_BOTH
@pytest.mark.parametrize("backend", [ggml_hip.GGML_BACKEND_GPU, ggml_hip.GGML_BACKEND_GPU_SPLIT])
@pytest.mark.parametrize("N", [1, 40])
def test_hook_transformed_weight(hook, backend, N):
    """A layer matrix's operand placement: weight uploaded by transform_tensor, host x, host dst."""
    L, variant = hook
    q3 = q3_of(variant)
    K, M = 2304, 101
    rng = rng_for(11, q3, N)
    wq = R.random_q23_K(rng, M, K, q3)
    x = rng.standard_normal((N, K)).astype(np.float32)
    staged = wq.copy()
    w = k_tensor(variant, staged, K, M, backend)
    L.ggml_hip_transform_tensor(staged.ctypes.data_as(ctypes.c_void_p), ctypes.byref(w))
    assert w.extra and w.backend == backend
    staged[:] = 0                                              # the loader frees its buffer
    y_np = np.zeros((N, M), np.float32)
    y, _ = mm_node(w, x, y_np)
    before = mul_mat_count(L)
    assert forward(L, y)
    assert mul_mat_count(L) == before + 1
    assert_bitwise(y_np, gpu_mul_mat(variant, wq, K, x))
    L.ggml_hip_set_exact(1)
    y_np[:] = 0
    assert forward(L, y)
    assert_bitwise(y_np, R.vec_dot_avx2(wq, R.quantize_q8_K(x), K, q3))
    L.ggml_hip_free_data(ctypes.byref(w))
    assert not w.extra


@HOOK_BOTH
def test_hook_host_weight_residency_cache(hook):
    L, variant = hook
    q3 = q3_of(variant)
    K, M = 256, 2048                                           # 2^19 elements: taken at N = 1
    rng = rng_for(12, q3)
    wq = R.random_q23_K(rng, M, K, q3)
    x = rng.standard_normal((1, K)).astype(np.float32)
    y_np = np.zeros((1, M), np.float32)
    w = k_tensor(variant, wq, K, M)
    y, xt = mm_node(w, x, y_np)
    assert L.ggml_hip_can_mul_mat(ctypes.byref(w), ctypes.byref(xt), ctypes.byref(y))
    small = k_tensor(variant, wq, K, M // 2)                   # below the threshold: left to ggml's CPU op
    ys, xs = mm_node(small, x, np.zeros((1, M // 2), np.float32))
    assert not L.ggml_hip_can_mul_mat(ctypes.byref(small), ctypes.byref(xs), ctypes.byref(ys))
    h, m, r = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    assert forward(L, y)
    ggml_hip.check(L.ggml_hip_weight_cache_stats(ctypes.byref(h), ctypes.byref(m), ctypes.byref(r)))
    hits0 = h.value
    first = y_np.copy()
    y_np[:] = 0
    assert forward(L, y)
    ggml_hip.check(L.ggml_hip_weight_cache_stats(ctypes.byref(h), ctypes.byref(m), ctypes.byref(r)))
    assert h.value == hits0 + 1
    assert_bitwise(y_np, first)
    assert_bitwise(y_np, gpu_mul_mat(variant, wq, K, x))
    L.ggml_hip_weight_cache_invalidate(wq.ctypes.data_as(ctypes.c_void_p), wq.nbytes)


@HOOK_BOTH
def test_hook_host_weight_decode_odd_superblocks(hook):
    """N = 1 on a host-resident weight with three superblocks per row (the last step's second half idle), through
    the residency cache"""
    L, variant = hook
    q3 = q3_of(variant)
    K, M = 768, 700                                            # 537,600 elements: above the 2^19 decode threshold
    rng = rng_for(15, q3)
    wq = R.random_q23_K(rng, M, K, q3)
    x = rng.standard_normal((1, K)).astype(np.float32)
    y_np = np.zeros((1, M), np.float32)
    w = k_tensor(variant, wq, K, M)
    y, xt = mm_node(w, x, y_np)
    assert L.ggml_hip_can_mul_mat(ctypes.byref(w), ctypes.byref(xt), ctypes.byref(y))
    assert forward(L, y)
    assert_bitwise(y_np, R.gemv_schedule(wq, x, K, q3))
    L.ggml_hip_weight_cache_invalidate(wq.ctypes.data_as(ctypes.c_void_p), wq.nbytes)


# K above the GEMV's limit (w2 of a 30B model has K = 17920; 70 superblocks per row): auto takes the exact kernel in
# every mode, so the shapes the hook path accepts never fail in the mul_mat
K_LONG = 17920


@BOTH
@pytest.mark.parametrize("N", [1, 9])
def test_long_K_auto_takes_exact_kernel(exact_off, variant, N):
    q3 = q3_of(variant)
    M = 19
    rng = rng_for(16, q3, N)
    wq = R.random_q23_K(rng, M, K_LONG, q3)
    x = rng.standard_normal((N, K_LONG)).astype(np.float32)
    ref = R.vec_dot_avx2(wq, R.quantize_q8_K(x), K_LONG, q3)
    assert exact_off.ggml_hip_debug_q23k_auto_algo(GTYPE[variant], K_LONG, M, N) == 4
    assert exact_off.ggml_hip_debug_q23k_auto_algo(GTYPE[variant], 16384, M, N) == 1
    assert_bitwise(gpu_mul_mat(variant, wq, K_LONG, x, algo=0), ref)          # fast mode
    assert_bitwise(gpu_mul_mat(variant, wq, K_LONG, x, algo=4), ref)
    mm = exact_off.ggml_hip_mul_mat_q3_K if q3 else exact_off.ggml_hip_mul_mat_q2_K
    b = DB(1 << 20)
    assert mm(b.ptr, K_LONG, 4, b.ptr, 1, b.ptr, 4, 1, None) == ggml_hip.ERR_UNSUPPORTED   # the GEMV itself: K <= 16384
    exact_off.ggml_hip_set_exact(1)
    assert_bitwise(gpu_mul_mat(variant, wq, K_LONG, x, algo=0), ref)


@HOOK_BOTH
def test_hook_declines(hook):
    L, variant = hook
    bs = R.block_bytes(q3_of(variant))
    N = 64
    # K % 256 != 0
    K, M = 384, 64
    w = k_tensor(variant, np.zeros((M, bs * K // 256), np.uint8), K, M)
    y, xt = mm_node(w, np.zeros((N, K), np.float32), np.zeros((N, M), np.float32))
    assert not L.ggml_hip_can_mul_mat(ctypes.byref(w), ctypes.byref(xt), ctypes.byref(y))
    assert not forward(L, y)
    # non-contiguous src1
    K = 512
    x = np.zeros((N, K), np.float32)
    w = k_tensor(variant, np.zeros((M, bs * K // 256), np.uint8), K, M)
    y, xt = mm_node(w, x, np.zeros((N, M), np.float32))
    assert L.ggml_hip_can_mul_mat(ctypes.byref(w), ctypes.byref(xt), ctypes.byref(y))
    xt.nb[1] *= 2
    xt.nb[2] = xt.nb[1] * N
    xt.nb[3] = xt.nb[2]
    assert not L.ggml_hip_can_mul_mat(ctypes.byref(w), ctypes.byref(xt), ctypes.byref(y))
    assert not forward(L, y)


# ---- launch fusion ----------------------------------------------------------------------------------------

@HOOK_BOTH
def test_fusion_on_off_bitwise(hook):
    """A k-quant node between two device-resident q4_0 mul_mat nodes (which the hook's scheduler holds when fusion
    is on), all on disjoint buffers: the k-quant node joins no group or chain, the scheduler flushes around it, and
    every output is bitwise the same as with fusion off."""
    import oracle as O
    L, variant = hook
    q3 = q3_of(variant)
    L.ggml_hip_debug_set_fuse.argtypes = [ctypes.c_int]
    K, M4, MK = 256, 48, 40
    rng = rng_for(14, q3)
    w4q = [np.ascontiguousarray(O.quantize_q4_0((rng.standard_normal((M4, K)) * 0.02).astype(np.float32))[0])
           for _ in range(2)]
    wkq = R.random_q23_K(rng, MK, K, q3)
    x4 = [rng.standard_normal((1, K)).astype(np.float32) for _ in range(2)]
    xk = rng.standard_normal((1, K)).astype(np.float32)

    def run(fuse):
        ggml_hip.check(L.ggml_hip_debug_set_fuse(fuse))
        q4 = []
        for wq, x in zip(w4q, x4):
            w4 = ggml_hip.make_tensor(ggml_hip.GGML_TYPE_Q4_0, (K, M4), wq, backend=ggml_hip.GGML_BACKEND_GPU)
            L.ggml_hip_transform_tensor(wq.ctypes.data_as(ctypes.c_void_p), ctypes.byref(w4))
            y4_host = np.zeros((1, M4), np.float32)
            y4, x4t = mm_node(w4, x, y4_host)
            x4t.backend = ggml_hip.GGML_BACKEND_GPU
            L.ggml_hip_transform_tensor(x.ctypes.data_as(ctypes.c_void_p), ctypes.byref(x4t))
            L.ggml_hip_assign_buffers_no_scratch(ctypes.byref(y4))
            assert y4.backend == ggml_hip.GGML_BACKEND_GPU and y4.extra
            q4.append((w4, y4, x4t, y4_host))
        wk = k_tensor(variant, wkq, K, MK, ggml_hip.GGML_BACKEND_GPU)
        L.ggml_hip_transform_tensor(wkq.ctypes.data_as(ctypes.c_void_p), ctypes.byref(wk))
        yk_host = np.zeros((1, MK), np.float32)
        yk, _ = mm_node(wk, xk, yk_host)
        assert forward(L, q4[0][1])
        assert forward(L, yk)
        assert forward(L, q4[1][1])
        for w4, y4, x4t, y4_host in q4:
            dev = ctypes.cast(y4.extra, ctypes.POINTER(ctypes.c_void_p * 16)).contents[0]
            ggml_hip.check(L.ggml_hip_memcpy_d2h(y4_host.ctypes.data_as(ctypes.c_void_p), dev, y4_host.nbytes, None))
        for w4, y4, x4t, _ in q4:
            for t in (y4, x4t, w4):
                L.ggml_hip_free_data(ctypes.byref(t))
        L.ggml_hip_free_data(ctypes.byref(wk))
        return q4[0][3], q4[1][3], yk_host

    try:
        on = run(1)
        off = run(0)
    finally:
        L.ggml_hip_debug_set_fuse(1)
    for a, b in zip(on, off):
        assert_bitwise(a, b)
    assert_bitwise(on[2], gpu_mul_mat(variant, wkq, K, xk))
    assert np.any(on[0] != 0) and np.any(on[1] != 0)
