"""The Q6_K prefill GEMM on the device (csrc/q6_k_gemm.hip, algo 5 of ggml_hip_mul_mat_q6_K): every y bit for bit
the GEMV schedule (tests/q6k_gemm_ref.gemv_order, independent of the device GEMV) and bit for bit the device
GEMV (algo 1), on random and crafted blocks, ragged tiles, misaligned weights, strided outputs, under graph
capture and through the ggml hook path with the auto rule."""
import ctypes

import numpy as np
import pytest

import q6k_gemm_ref as G
import q6k_ref as R
from hip_env import ggml_hip, gpu_available
from parity import check_y
from test_q6k_ref import bits

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason="needs a HIP device and libggml_hip.so")]

DB = ggml_hip.DeviceBuffer
GEMM, GEMV = 5, 1


def assert_bitwise(got, ref):
    diff = np.flatnonzero(bits(got).ravel() != bits(ref).ravel())
    assert diff.size == 0, f"{diff.size} of {got.size} differ; first at {diff[:4]}: {np.ravel(got)[diff[:4]]} vs " \
                           f"{np.ravel(ref)[diff[:4]]}"


def rng_for(*key):
    return np.random.default_rng([0x6D, *key])


def gpu_mul_mat(wq, K, x, algo, ldy=None, fill=None, w_off=0):
    """w_off: the rows start that many bytes into their buffer (two more bytes follow them, so that the
    aligned word holding the last row's end is inside the allocation)."""
    M, N = wq.shape[0], x.shape[0]
    ld = M if ldy is None else ldy
    raw = np.concatenate([np.full(w_off, 0xA5, np.uint8), np.ascontiguousarray(wq).ravel(), np.full(2, 0x5A, np.uint8)])
    wd, xd = DB.from_array(raw), DB.from_array(x)
    yd = DB.from_array(np.full((N, ld), np.float32(0 if fill is None else fill), np.float32))
    ggml_hip.mul_mat_q6_K(wd, K, M, xd, N, yd, algo=algo, ldy=ld, w_off=w_off)
    return yd.download((N, ld), np.float32)


@pytest.fixture
def L():
    lib = ggml_hip.load()
    prev = lib.ggml_hip_get_exact()
    lib.ggml_hip_set_exact(0)
    yield lib
    lib.ggml_hip_set_exact(prev)


# ---- 1. against the numpy schedule ------------------------------------------------------------------------

@pytest.mark.parametrize("K,M", [(K, M) for K in (256, 768) for M in (1, 33)])
def test_gemm_bitwise_gemv_order(L, K, M):
    """Asymmetric random integers in both operands: a wrong A / B lane map or a transposed C / D map cannot pass."""
    rng = rng_for(1, K, M)
    wq = R.random_q6_K(rng, M, K)
    x = (rng.standard_normal((33, K)) * 3).astype(np.float32)
    ref = G.gemv_order(wq, R.quantize_q8_K(x), K)
    for N in (1, 9, 33):
        assert_bitwise(gpu_mul_mat(wq, K, x[:N], GEMM), ref[:N])


def crafted():
    """K = 256 rows at the ends of the integer range, with ordinary, zero and subnormal d."""
    e = np.arange(256)
    rows = [
        (np.zeros(256, np.uint8), np.full(16, -128)),                       # w' = 4096 everywhere
        (np.full(256, 63, np.uint8), np.full(16, 127)),                     # w' = 3937
        (np.zeros(256, np.uint8), np.full(16, 127)),                        # w' = -4064
        (np.full(256, 63, np.uint8), np.full(16, -128)),                    # w' = -3968
        (np.where(e & 1, 63, 0).astype(np.uint8), np.where(np.arange(16) & 1, 127, -128)),   # alternating signs
        (np.where(e & 1, 0, 63).astype(np.uint8), np.where(np.arange(16) & 1, -128, 127)),
    ]
    ds = [np.float16(0.0123), np.float16(-1.5), np.float16(0.0), np.uint16(0x0001).view(np.float16),
          np.uint16(0x83FF).view(np.float16)]                               # zero and fp16 subnormals
    q6 = np.stack([r[0] for r in rows for _ in ds]).reshape(-1, 1, 256)
    sc = np.stack([r[1] for r in rows for _ in ds]).astype(np.int8).reshape(-1, 1, 16)
    d = np.array([dv for _ in rows for dv in ds], np.float16).reshape(-1, 1)
    return G.pack_q6_K(q6, sc, d)


def test_gemm_crafted_extremes_bitwise_gemv_order(L):
    wq = crafted()
    e = np.arange(256)
    rng = rng_for(2)
    x = np.stack([
        np.full(256, 0.75),                                                 # every q8 = -128
        np.full(256, -3.0),                                                 # every q8 = -128 (the sign is iscale's)
        np.where(e & 1, -2.0, 2.0),                                         # -128, +127 alternating
        np.where(e & 1, 1.0, -1.0) * (1 + (e % 7)),
        rng.standard_normal(256) * 1e-3,
        np.zeros(256),
    ]).astype(np.float32)
    xq = R.quantize_q8_K(x)
    _, q8, _ = R.split_q8_K(xq, 256)
    assert np.all(q8[0] == -128) and np.all(q8[1] == -128)
    _, _, lanes = R._lane_sums(wq, xq, 256)
    isum = lanes.sum(-1)
    assert isum.min() == -2 ** 27                                           # the range's end is reached
    ref = G.gemv_order(wq, xq, 256)
    assert_bitwise(gpu_mul_mat(wq, 256, x, GEMM), ref)
    assert_bitwise(gpu_mul_mat(wq, 256, x, GEMV), ref)


# ---- 2. against the device GEMV ---------------------------------------------------------------------------

M_MAX, N_MAX = 257, 257
MS = (1, 31, 33, 63, 64, 65, 100, 257)                # tile edges: 32 (wave), 64 (workgroup rows)
NS = (1, 8, 9, 33, 64, 65, 128, 129, 200, 256, 257)   # tiles of 64 columns up to N = 64, 128 up to 128, then 256


@pytest.fixture(scope="module")
def operands():
    out = {}
    for K in (256, 2304, 4096):
        rng = rng_for(3, K)
        out[K] = (R.random_q6_K(rng, M_MAX, K), rng.standard_normal((N_MAX, K)).astype(np.float32))
    return out


@pytest.mark.parametrize("K", [256, 2304, 4096])
def test_gemm_bitwise_gemv(L, operands, K):
    """K = 2304: rows are 1890 bytes, so odd rows sit at 2 mod 4.  One GEMV reference at the largest shape:
    an output depends on its own row and column only."""
    wq, x = operands[K]
    ref = gpu_mul_mat(wq, K, x, GEMV)
    for M in MS:
        for N in NS:
            assert_bitwise(gpu_mul_mat(wq[:M], K, x[:N], GEMM), ref[:N, :M])


@pytest.mark.parametrize("N", [1, 12])
def test_gemm_beyond_gemv_k(L, N):
    K, M = 16640, 5
    rng = rng_for(4, N)
    wq = R.random_q6_K(rng, M, K)
    x = rng.standard_normal((N, K)).astype(np.float32)
    xq = R.quantize_q8_K(x)
    ref = G.gemv_order(wq, xq, K)
    y = gpu_mul_mat(wq, K, x, GEMM)
    assert_bitwise(y, ref)
    y_exact, s_abs = R.block_terms(wq, xq, K)
    check_y(y, y_exact, s_abs)
    assert_bitwise(gpu_mul_mat(wq, K, x, 0), ref)             # auto: the GEMV cannot run here
    wd, xd, yd = DB.from_array(wq), DB.from_array(x), DB(N * M * 4)
    assert L.ggml_hip_mul_mat_q6_K(wd.ptr, K, M, xd.ptr, N, yd.ptr, M, GEMV, None) == ggml_hip.ERR_UNSUPPORTED


@pytest.mark.parametrize("K", [256, 2304])
def test_gemm_weight_at_2_mod_4(L, K):
    M, N = 70, 40
    rng = rng_for(5, K)
    wq = R.random_q6_K(rng, M, K)
    x = rng.standard_normal((N, K)).astype(np.float32)
    assert_bitwise(gpu_mul_mat(wq, K, x, GEMM, w_off=2), gpu_mul_mat(wq, K, x, GEMM))


def test_gemm_ldy_gap_untouched(L):
    K, M, N, ld = 512, 37, 70, 48
    rng = rng_for(6)
    wq = R.random_q6_K(rng, M, K)
    x = rng.standard_normal((N, K)).astype(np.float32)
    y = gpu_mul_mat(wq, K, x, GEMM, ldy=ld, fill=-7.5)
    assert np.all(y[:, M:] == np.float32(-7.5))
    assert_bitwise(y[:, :M], gpu_mul_mat(wq, K, x, GEMM))


def test_gemm_doubling_x_doubles_y_bitwise(L):
    K, M, N = 2304, 50, 70
    rng = rng_for(7)
    wq = R.random_q6_K(rng, M, K, special_d=False)
    x = rng.standard_normal((N, K)).astype(np.float32)
    assert_bitwise(gpu_mul_mat(wq, K, 2 * x, GEMM), 2 * gpu_mul_mat(wq, K, x, GEMM))


def test_gemm_graph_capture_replays(L):
    K, M, N = 2304, 300, 40
    rng = rng_for(8)
    wq = R.random_q6_K(rng, M, K)
    x = rng.standard_normal((N, K)).astype(np.float32)
    eager = gpu_mul_mat(wq, K, x, GEMM)                       # also reserves the stream's workspace
    wd, xd, yd = DB.from_array(wq), DB.from_array(x), DB(N * M * 4)
    s = L.ggml_hip_default_stream()
    g = ggml_hip.Graph(s)
    with g:
        ggml_hip.mul_mat_q6_K(wd, K, M, xd, N, yd, algo=GEMM, stream=s)
    for _ in range(3):
        ggml_hip.check(L.ggml_hip_memset(yd.ptr, 0xFF, N * M * 4, s))
        g.launch()
        ggml_hip.check(L.ggml_hip_stream_synchronize(s))
        assert_bitwise(yd.download((N, M), np.float32), eager)


def test_gemm_lm_head_rows(L):
    K, M, N = 4096, 32000, 24
    rng = rng_for(9)
    wq = R.random_q6_K(rng, M, K)
    x = rng.standard_normal((N, K)).astype(np.float32)
    wd, xd = DB.from_array(wq), DB.from_array(x)
    ys = []
    for algo in (GEMM, GEMV):
        yd = DB(N * M * 4)
        ggml_hip.mul_mat_q6_K(wd, K, M, xd, N, yd, algo=algo)
        ys.append(yd.download((N, M), np.float32))
    assert_bitwise(ys[0], ys[1])
    assert np.any(ys[0] != 0)


def test_gemm_status_codes(L):
    b = DB(1 << 16)
    assert L.ggml_hip_mul_mat_q6_K(b.ptr, 384, 4, b.ptr, 1, b.ptr, 4, GEMM, None) == ggml_hip.ERR_INVALID
    assert L.ggml_hip_mul_mat_q6_K(b.ptr, 256, 4, b.ptr, 1, b.ptr, 4, 3, None) == ggml_hip.ERR_INVALID
    assert L.ggml_hip_mul_mat_q6_K(b.ptr, 256, 4, b.ptr, 1, b.ptr, 3, GEMM, None) == ggml_hip.ERR_INVALID   # ldy < M
    assert L.ggml_hip_mul_mat_q6_K(b.ptr, 256, 4, b.ptr, 0, b.ptr, 4, GEMM, None) == ggml_hip.OK            # N = 0
    # Q6_K checks the operands before the algo: an empty call is OK whatever the algo
    assert L.ggml_hip_mul_mat_q6_K(b.ptr, 256, 4, b.ptr, 0, b.ptr, 4, 3, None) == ggml_hip.OK


def test_reserved_workspace_covers_the_gemm(L):
    """After ggml_hip_reserve_workspace(K, N) a capture (which forbids growing the workspace) takes the GEMM."""
    K, M, N = 4096, 20, 333
    rng = rng_for(10)
    wq = R.random_q6_K(rng, M, K)
    x = rng.standard_normal((N, K)).astype(np.float32)
    ggml_hip.check(L.ggml_hip_reserve_workspace(K, N))
    wd, xd, yd = DB.from_array(wq), DB.from_array(x), DB(N * M * 4)
    s = L.ggml_hip_default_stream()
    gpu_mul_mat(wq[:1], K, x[:130], GEMM)                     # (the wide tile's attributes are set outside the capture)
    g = ggml_hip.Graph(s)
    with g:
        ggml_hip.mul_mat_q6_K(wd, K, M, xd, N, yd, algo=GEMM, stream=s)
    g.launch()
    ggml_hip.check(L.ggml_hip_stream_synchronize(s))
    assert_bitwise(yd.download((N, M), np.float32), gpu_mul_mat(wq, K, x, GEMV))


# ---- 3. hook path -----------------------------------------------------------------------------------------

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


def forward(lib, node):
    p = ggml_hip.GgmlComputeParams(ggml_hip.GGML_TASK_COMPUTE, 0, 1, 0, None)
    return lib.ggml_hip_compute_forward(ctypes.byref(p), ctypes.byref(node))


@pytest.mark.parametrize("backend", [ggml_hip.GGML_BACKEND_GPU, ggml_hip.GGML_BACKEND_GPU_SPLIT])
@pytest.mark.parametrize("N", [40, 200])
def test_hook_takes_the_gemm(L, backend, N):
    """The lm_head's operand placement: weight uploaded by transform_tensor, host x, host dst; auto from N = 9."""
    K, M = 2304, 101
    rng = rng_for(11, N)
    wq = R.random_q6_K(rng, M, K)
    x = rng.standard_normal((N, K)).astype(np.float32)
    prev = L.ggml_hip_debug_set_q6k_gemm_min_n(9)
    try:
        assert L.ggml_hip_debug_q6k_auto_algo(K, M, N) == GEMM
        staged = wq.copy()
        w = q6_tensor(staged, K, M, backend)
        L.ggml_hip_transform_tensor(staged.ctypes.data_as(ctypes.c_void_p), ctypes.byref(w))
        assert w.extra and w.backend == backend
        staged[:] = 0                                          # the loader frees its buffer
        y_np = np.zeros((N, M), np.float32)
        y, _ = mm_node(w, x, y_np)
        assert forward(L, y)
        L.ggml_hip_free_data(ctypes.byref(w))
        assert_bitwise(y_np, gpu_mul_mat(wq, K, x, GEMM))
        assert_bitwise(y_np, gpu_mul_mat(wq, K, x, GEMV))
    finally:
        L.ggml_hip_debug_set_q6k_gemm_min_n(prev)


def test_hook_host_weight_takes_the_gemm(L):
    K, M, N = 2304, 70, 40
    rng = rng_for(12)
    wq = R.random_q6_K(rng, M, K)
    x = rng.standard_normal((N, K)).astype(np.float32)
    prev = L.ggml_hip_debug_set_q6k_gemm_min_n(9)
    try:
        y_np = np.zeros((N, M), np.float32)
        w = q6_tensor(wq, K, M)
        y, xt = mm_node(w, x, y_np)
        assert L.ggml_hip_can_mul_mat(ctypes.byref(w), ctypes.byref(xt), ctypes.byref(y))
        for _ in range(2):                                     # the second pass finds the weight in the residency cache
            y_np[:] = 0
            assert forward(L, y)
            assert_bitwise(y_np, gpu_mul_mat(wq, K, x, GEMM))
        assert_bitwise(y_np, gpu_mul_mat(wq, K, x, GEMV))
        L.ggml_hip_weight_cache_invalidate(wq.ctypes.data_as(ctypes.c_void_p), wq.nbytes)
    finally:
        L.ggml_hip_debug_set_q6k_gemm_min_n(prev)
