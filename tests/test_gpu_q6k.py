"""Q6_K x F32 mul_mat on the device (csrc/q6_k.hip): the q8_K quantizer and the Q6_K dequantizer bit for bit,
the fused GEMV within the parity bound, column tiling, exact mode bit-identical to the reference's AVX2
ggml_vec_dot_q6_K_q8_K, graph capture, and the ggml hook path on hand-built tensors.  References: the fixtures
the compiled reference wrote (tests/golden/q6k_*) and their numpy restatement tests/q6k_ref.py."""
import ctypes

import numpy as np
import pytest

import q6k_ref as R
from golden_io import load
from hip_env import ggml_hip, gpu_available
from parity import check_y
from test_q6k_ref import assert_q8k_equal, bits

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason="needs a HIP device and libggml_hip.so")]

DB = ggml_hip.DeviceBuffer
KS = (256, 2304, 4096)


def assert_bitwise(got, ref):
    diff = np.flatnonzero(bits(got).ravel() != bits(ref).ravel())
    assert diff.size == 0, f"{diff.size} of {got.size} differ; first at {diff[:4]}: {np.ravel(got)[diff[:4]]} vs " \
                           f"{np.ravel(ref)[diff[:4]]}"


def rng_for(*key):
    return np.random.default_rng([0x6B, *key])


def gpu_q8_K(x):
    N, K = x.shape
    xd, qd = DB.from_array(x), DB(N * K // 256 * 292)
    ggml_hip.quantize_q8_K(xd, K, N, qd)
    return qd.download((N, K // 256 * 292), np.uint8)


def gpu_mul_mat(wq, K, x, algo=0, ldy=None, fill=None):
    M, N = wq.shape[0], x.shape[0]
    ld = M if ldy is None else ldy
    wd, xd = DB.from_array(wq), DB.from_array(x)
    y0 = np.full((N, ld), np.float32(0 if fill is None else fill), np.float32)
    yd = DB.from_array(y0)
    ggml_hip.mul_mat_q6_K(wd, K, M, xd, N, yd, algo=algo, ldy=ld)
    return yd.download((N, ld), np.float32)


@pytest.fixture
def exact_off():
    L = ggml_hip.load()
    prev = L.ggml_hip_get_exact()
    L.ggml_hip_set_exact(0)
    yield L
    L.ggml_hip_set_exact(prev)


# ---- 4. q8_K quantizer ------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", KS)
def test_quantize_q8_K_fixture(K):
    assert_q8k_equal(gpu_q8_K(load("q6k", f"x{K}_f32")), load("q6k", f"x{K}_q8_K"), K)


@pytest.mark.parametrize("K,N", [(K, N) for K in (256, 768, 4096) for N in (1, 5)])
def test_quantize_q8_K_random_rows(K, N):
    x = (rng_for(4, K, N).standard_normal((N, K)) * 3).astype(np.float32)
    got = gpu_q8_K(x)
    assert np.array_equal(got, R.quantize_q8_K(x))           # every byte, bsums included


def test_quantize_q8_K_crafted_blocks():
    x = load("q6k", "craft_f32")
    got = gpu_q8_K(x)
    assert_q8k_equal(got, load("q6k", "craft_q8_K"), 256)
    assert np.array_equal(got, R.quantize_q8_K(x))           # zeros in the bsums of the all-zero block
    assert_q8k_equal(gpu_q8_K(x.reshape(1, -1)), load("q6k", "craft_q8_K").reshape(1, -1), x.size)   # as one row


# ---- 5. dequantize ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("K,M", [(K, M) for K in (256, 2304) for M in (1, 7)])
def test_dequantize_q6_K_bitwise(K, M):
    wq = R.random_q6_K(rng_for(5, K, M), M, K)
    wd, od = DB.from_array(wq), DB(M * K * 4)
    ggml_hip.dequantize_q6_K(wd, K, M, od)
    assert_bitwise(od.download((M, K), np.float32), R.dequantize_q6_K(wq, K))


def test_dequantize_q6_K_fixture():
    ref = load("q6k", "w2304_dequant")
    wq = np.ascontiguousarray(load("q6k", "w2304_q6_K")[:ref.shape[0]])
    wd, od = DB.from_array(wq), DB(ref.nbytes)
    ggml_hip.dequantize_q6_K(wd, 2304, ref.shape[0], od)
    assert_bitwise(od.download(ref.shape, np.float32), ref)


# ---- 6. fast GEMV -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("K,M", [(K, M) for K in (256, 512, 2304, 4096, 5120) for M in (1, 17, 100, 1000)])
def test_gemv_within_parity_bound(exact_off, K, M):
    """N = 1, 2, 8 on the same weights; the bound is parity.check_y's default, 1e-3 |y| + 1e-6 S_abs with S_abs
    over superblocks.  K = 2304: rows at 2 mod 4; K = 256: one superblock; M = 1, 17: ragged waves."""
    rng = rng_for(6, K, M)
    wq = R.random_q6_K(rng, M, K)
    x = rng.standard_normal((8, K)).astype(np.float32)
    y_ref, s_abs = R.block_terms(wq, R.quantize_q8_K(x), K)
    for N in (1, 2, 8):
        y = gpu_mul_mat(wq, K, x[:N], algo=1)
        check_y(y, y_ref[:N], s_abs[:N])


# ---- 7. column tiling -------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [9, 17, 33])
def test_column_tiles_bitwise_per_tile_calls(exact_off, N):
    K, M = 512, 37
    rng = rng_for(7, N)
    wq = R.random_q6_K(rng, M, K)
    x = rng.standard_normal((N, K)).astype(np.float32)
    y = gpu_mul_mat(wq, K, x, algo=1)
    for n0 in range(0, N, 8):
        assert_bitwise(y[n0:n0 + 8], gpu_mul_mat(wq, K, x[n0:n0 + 8], algo=1))
    assert_bitwise(y, gpu_mul_mat(wq, K, x, algo=0))         # auto = GEMV outside exact mode


@pytest.mark.parametrize("algo", [1, 4])
def test_ldy_gap_untouched(exact_off, algo):
    K, M, N, ld = 512, 37, 11, 48
    rng = rng_for(7, 99)
    wq = R.random_q6_K(rng, M, K)
    x = rng.standard_normal((N, K)).astype(np.float32)
    y = gpu_mul_mat(wq, K, x, algo=algo, ldy=ld, fill=-7.5)
    assert np.all(y[:, M:] == np.float32(-7.5))
    assert_bitwise(y[:, :M], gpu_mul_mat(wq, K, x, algo=algo))


# ---- 8. exact mode ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", KS)
def test_exact_fixture_bitwise(exact_off, K):
    wq, x, y = load("q6k", f"w{K}_q6_K"), load("q6k", f"x{K}_f32"), load("q6k", f"y{K}_vec_dot")
    assert_bitwise(gpu_mul_mat(wq, K, x, algo=4), y)
    assert_bitwise(gpu_mul_mat(wq, K, x[:1], algo=4), y[:1])
    exact_off.ggml_hip_set_exact(1)
    assert_bitwise(gpu_mul_mat(wq, K, x, algo=0), y)


@pytest.mark.parametrize("K,N", [(K, N) for K in KS for N in (1, 3, 9)])
def test_exact_vs_ref_bitwise(exact_off, K, N):
    M = 33
    rng = rng_for(8, K, N)
    wq = R.random_q6_K(rng, M, K)
    x = rng.standard_normal((N, K)).astype(np.float32)
    ref = R.vec_dot_avx2(wq, R.quantize_q8_K(x), K)
    assert_bitwise(gpu_mul_mat(wq, K, x, algo=4), ref)
    exact_off.ggml_hip_set_exact(1)
    assert_bitwise(gpu_mul_mat(wq, K, x, algo=0), ref)


# ---- 9. scaling -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("algo", [1, 4])
def test_doubling_x_doubles_y_bitwise(exact_off, algo):
    """x -> 2x halves iscale exactly and leaves every integer unchanged, so y doubles bit for bit."""
    K, M, N = 2304, 50, 3
    rng = rng_for(9)
    wq = R.random_q6_K(rng, M, K, special_d=False)
    x = rng.standard_normal((N, K)).astype(np.float32)
    y1, y2 = gpu_mul_mat(wq, K, x, algo=algo), gpu_mul_mat(wq, K, 2 * x, algo=algo)
    assert_bitwise(y2, 2 * y1)


# ---- 10. the lm_head shape --------------------------------------------------------------------------------

def test_lm_head_shape(exact_off):
    K, M = 4096, 32000
    rng = rng_for(10)
    wq = R.random_q6_K(rng, M, K)
    x = rng.standard_normal((1, K)).astype(np.float32)
    y = gpu_mul_mat(wq, K, x, algo=0)
    xq = R.quantize_q8_K(x)
    step = 4000
    for m0 in range(0, M, step):
        y_ref, s_abs = R.block_terms(wq[m0:m0 + step], xq, K)
        check_y(y[:, m0:m0 + step], y_ref, s_abs)


# ---- 11. graph capture ------------------------------------------------------------------------------------

def test_graph_capture_replays_q6_K_gemv(exact_off):
    K, M = 2304, 300
    rng = rng_for(11)
    wq = R.random_q6_K(rng, M, K)
    x = rng.standard_normal((1, K)).astype(np.float32)
    eager = gpu_mul_mat(wq, K, x, algo=0)
    wd, xd, yd = DB.from_array(wq), DB.from_array(x), DB(M * 4)
    L = exact_off
    s = L.ggml_hip_default_stream()
    g = ggml_hip.Graph(s)
    with g:
        ggml_hip.mul_mat_q6_K(wd, K, M, xd, 1, yd, stream=s)
    for _ in range(2):
        ggml_hip.check(L.ggml_hip_memset(yd.ptr, 0xFF, M * 4, s))
        g.launch()
        ggml_hip.check(L.ggml_hip_stream_synchronize(s))
        assert_bitwise(yd.download((1, M), np.float32), eager)


# ---- 12. hook path ----------------------------------------------------------------------------------------

def q6_tensor(wq, K, M, backend=ggml_hip.GGML_BACKEND_CPU):
    return ggml_hip.make_tensor(ggml_hip.GGML_TYPE_Q6_K, (K, M), wq, backend=backend)


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


def test_hook_host_tensors(exact_off):
    L = exact_off
    K, M, N = 2304, 70, 32
    rng = rng_for(12, 1)
    wq = R.random_q6_K(rng, M, K)
    x = rng.standard_normal((N, K)).astype(np.float32)
    y_np = np.zeros((N, M), np.float32)
    w = q6_tensor(wq, K, M)
    y, xt = mm_node(w, x, y_np)
    assert L.ggml_hip_can_mul_mat(ctypes.byref(w), ctypes.byref(xt), ctypes.byref(y))
    before = mul_mat_count(L)
    assert forward(L, y)
    assert mul_mat_count(L) == before + 1
    assert_bitwise(y_np, gpu_mul_mat(wq, K, x))


@pytest.mark.parametrize("backend", [ggml_hip.GGML_BACKEND_GPU, ggml_hip.GGML_BACKEND_GPU_SPLIT])
@pytest.mark.parametrize("N", [1, 40])
def test_hook_transformed_weight(exact_off, backend, N):
    """The lm_head's operand placement: weight uploaded by transform_tensor, host x, host dst."""
    L = exact_off
    K, M = 2304, 101
    rng = rng_for(12, 2, N)
    wq = R.random_q6_K(rng, M, K)
    x = rng.standard_normal((N, K)).astype(np.float32)
    staged = wq.copy()
    w = q6_tensor(staged, K, M, backend)
    L.ggml_hip_transform_tensor(staged.ctypes.data_as(ctypes.c_void_p), ctypes.byref(w))
    assert w.extra and w.backend == backend
    staged[:] = 0                                              # the loader frees its buffer
    y_np = np.zeros((N, M), np.float32)
    y, _ = mm_node(w, x, y_np)
    assert forward(L, y)
    assert_bitwise(y_np, gpu_mul_mat(wq, K, x))
    L.ggml_hip_set_exact(1)
    y_np[:] = 0
    assert forward(L, y)
    assert_bitwise(y_np, R.vec_dot_avx2(wq, R.quantize_q8_K(x), K))
    L.ggml_hip_free_data(ctypes.byref(w))
    assert not w.extra


def test_hook_host_weight_residency_cache(exact_off):
    L = exact_off
    K, M = 256, 2048                                           # 2^19 elements: taken at N = 1
    rng = rng_for(12, 3)
    wq = R.random_q6_K(rng, M, K)
    x = rng.standard_normal((1, K)).astype(np.float32)
    y_np = np.zeros((1, M), np.float32)
    w = q6_tensor(wq, K, M)
    y, xt = mm_node(w, x, y_np)
    assert L.ggml_hip_can_mul_mat(ctypes.byref(w), ctypes.byref(xt), ctypes.byref(y))
    small = q6_tensor(wq, K, M // 2)                           # below the threshold: left to ggml's CPU op
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
    assert_bitwise(y_np, gpu_mul_mat(wq, K, x))
    L.ggml_hip_weight_cache_invalidate(wq.ctypes.data_as(ctypes.c_void_p), wq.nbytes)


def test_hook_declines(exact_off):
    L = exact_off
    N = 64
    x = np.zeros((N, 512), np.float32)
    # K % 256 != 0
    K, M = 384, 64
    w = q6_tensor(np.zeros((M, 210 * K // 256), np.uint8), K, M)
    y, xt = mm_node(w, np.zeros((N, K), np.float32), np.zeros((N, M), np.float32))
    assert not L.ggml_hip_can_mul_mat(ctypes.byref(w), ctypes.byref(xt), ctypes.byref(y))
    assert not forward(L, y)
    # non-contiguous src1
    K = 512
    w = q6_tensor(np.zeros((M, 210 * K // 256), np.uint8), K, M)
    y, xt = mm_node(w, x, np.zeros((N, M), np.float32))
    assert L.ggml_hip_can_mul_mat(ctypes.byref(w), ctypes.byref(xt), ctypes.byref(y))
    xt.nb[1] *= 2
    xt.nb[2] = xt.nb[1] * N
    xt.nb[3] = xt.nb[2]
    assert not L.ggml_hip_can_mul_mat(ctypes.byref(w), ctypes.byref(xt), ctypes.byref(y))
    assert not forward(L, y)
    # Q4_K is still declined (with a correctly sized host copy from transform_tensor)
    w4 = ggml_hip.make_tensor(12, (K, M), np.zeros((M, 144 * K // 256), np.uint8))
    w4.nb[0], w4.nb[1] = 144, 144 * K // 256
    w4.nb[2] = w4.nb[3] = w4.nb[1] * M
    y, xt = mm_node(w4, x, np.zeros((N, M), np.float32))
    assert not L.ggml_hip_can_mul_mat(ctypes.byref(w4), ctypes.byref(xt), ctypes.byref(y))
    assert not forward(L, y)
    src = np.arange(M * 144 * K // 256, dtype=np.uint32).astype(np.uint8)
    w4.backend = ggml_hip.GGML_BACKEND_GPU
    L.ggml_hip_transform_tensor(src.ctypes.data_as(ctypes.c_void_p), ctypes.byref(w4))
    assert w4.backend == ggml_hip.GGML_BACKEND_CPU and not w4.extra
    held = np.ctypeslib.as_array(ctypes.cast(w4.data, ctypes.POINTER(ctypes.c_uint8)), shape=(src.size,))
    assert np.array_equal(held, src)
    del held
    L.ggml_hip_free_data(ctypes.byref(w4))


def test_status_codes(exact_off):
    L = exact_off
    b = DB(1 << 16)
    assert L.ggml_hip_mul_mat_q6_K(b.ptr, 384, 4, b.ptr, 1, b.ptr, 4, 0, None) == ggml_hip.ERR_INVALID
    assert L.ggml_hip_quantize_q8_K(b.ptr, 384, 1, b.ptr, None) == ggml_hip.ERR_INVALID
    assert L.ggml_hip_dequantize_q6_K(b.ptr, 384, 1, b.ptr, None) == ggml_hip.ERR_INVALID
    assert L.ggml_hip_mul_mat_q6_K(b.ptr, 256, 4, b.ptr, 1, b.ptr, 3, 0, None) == ggml_hip.ERR_INVALID    # ldy < M
    assert L.ggml_hip_mul_mat_q6_K(b.ptr, 256, 4, b.ptr, 1, b.ptr, 4, 2, None) == ggml_hip.ERR_INVALID    # algo
    assert L.ggml_hip_mul_mat_q6_K(b.ptr, 256, 4, b.ptr, 0, b.ptr, 4, 0, None) == ggml_hip.OK             # N = 0
    mm = L.ggml_hip_mul_mat_q6_K
    for algo in (2, 3, 6, -1):
        assert mm(b.ptr, 256, 4, b.ptr, 0, b.ptr, 4, algo, None) == ggml_hip.OK          # N = 0 returns before the algo check
    assert mm(None, 256, 4, b.ptr, 1, b.ptr, 4, 0, None) == ggml_hip.ERR_INVALID
    assert mm(b.ptr, 256, 4, None, 1, b.ptr, 4, 0, None) == ggml_hip.ERR_INVALID
    assert mm(b.ptr, 256, 4, b.ptr, 1, None, 4, 0, None) == ggml_hip.ERR_INVALID
    assert mm(b.ptr, 256, 4, b.ptr + 4, 1, b.ptr, 4, 0, None) == ggml_hip.ERR_INVALID    # x not 16-byte aligned
    assert mm(b.ptr, 256, 4, b.ptr, 1, b.ptr + 2, 4, 0, None) == ggml_hip.ERR_INVALID    # y not 4-byte aligned
    assert mm(b.ptr + 1, 256, 4, b.ptr, 1, b.ptr, 4, 0, None) == ggml_hip.ERR_INVALID    # W not 2-byte aligned
    assert mm(b.ptr, 16640, 4, b.ptr, 0, b.ptr, 4, 1, None) == ggml_hip.OK               # K past the GEMV, nothing to run
    assert mm(b.ptr, 16640, 4, b.ptr, 1, b.ptr, 4, 1, None) == ggml_hip.ERR_UNSUPPORTED  # (refused before any launch)


# ---- 13. launch fusion ------------------------------------------------------------------------------------

def test_fusion_on_off_bitwise(exact_off):
    """A device-resident q4_0 mul_mat node (held by the hook's scheduler when fusion is on) followed by a Q6_K
    node on disjoint buffers: the Q6_K node flushes the held node and both outputs are bitwise the same as with
    fusion off."""
    import oracle as O
    L = exact_off
    L.ggml_hip_debug_set_fuse.argtypes = [ctypes.c_int]
    K, M4, M6 = 256, 48, 40
    rng = rng_for(13)
    w4q, _ = O.quantize_q4_0((rng.standard_normal((M4, K)) * 0.02).astype(np.float32))
    w4q = np.ascontiguousarray(w4q)
    w6q = R.random_q6_K(rng, M6, K)
    x4 = rng.standard_normal((1, K)).astype(np.float32)
    x6 = rng.standard_normal((1, K)).astype(np.float32)

    def run(fuse):
        ggml_hip.check(L.ggml_hip_debug_set_fuse(fuse))
        w4 = ggml_hip.make_tensor(ggml_hip.GGML_TYPE_Q4_0, (K, M4), w4q, backend=ggml_hip.GGML_BACKEND_GPU)
        L.ggml_hip_transform_tensor(w4q.ctypes.data_as(ctypes.c_void_p), ctypes.byref(w4))
        y4_host = np.zeros((1, M4), np.float32)
        y4, x4t = mm_node(w4, x4, y4_host)
        x4t.backend = ggml_hip.GGML_BACKEND_GPU
        L.ggml_hip_transform_tensor(x4.ctypes.data_as(ctypes.c_void_p), ctypes.byref(x4t))
        L.ggml_hip_assign_buffers_no_scratch(ctypes.byref(y4))
        assert y4.backend == ggml_hip.GGML_BACKEND_GPU and y4.extra
        w6 = q6_tensor(w6q, K, M6, ggml_hip.GGML_BACKEND_GPU)
        L.ggml_hip_transform_tensor(w6q.ctypes.data_as(ctypes.c_void_p), ctypes.byref(w6))
        y6_host = np.zeros((1, M6), np.float32)
        y6, _ = mm_node(w6, x6, y6_host)
        assert forward(L, y4)
        assert forward(L, y6)
        dev = ctypes.cast(y4.extra, ctypes.POINTER(ctypes.c_void_p * 16)).contents[0]
        ggml_hip.check(L.ggml_hip_memcpy_d2h(y4_host.ctypes.data_as(ctypes.c_void_p), dev, y4_host.nbytes, None))
        for t in (y4, x4t, w4, w6):
            L.ggml_hip_free_data(ctypes.byref(t))
        return y4_host, y6_host

    try:
        on4, on6 = run(1)
        off4, off6 = run(0)
    finally:
        L.ggml_hip_debug_set_fuse(1)
    assert_bitwise(on4, off4)
    assert_bitwise(on6, off6)
    assert_bitwise(on6, gpu_mul_mat(w6q, K, x6))
    assert np.any(on4 != 0)
