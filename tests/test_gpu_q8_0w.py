"""Q8_0 WEIGHTS x F32 mul_mat on the device (csrc/blk32_w.hip): exact mode bit-identical to the reference's AVX2
ggml_vec_dot_q8_0_q8_0, the fused GEMV within the parity bound under every launch policy and tiling, the
per-call int8 image + k_gemm8 prefill path (bitwise the q4_0 path's on equal values), the dequantizer, graph
capture, status codes and the ggml hook path on hand-built tensors.  References: the fixtures the compiled
reference wrote (tests/golden/q8w_*) and their numpy restatement tests/q8_0w_ref.py; weights beyond the fixtures
come from the oracle's bit-exact quantize_q8_0."""
import ctypes
import functools

import numpy as np
import pytest

import oracle as O
import q8_0w_ref as R
from golden_io import load
from hip_env import ggml_hip, gpu_available
from parity import check_y

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason="needs a HIP device and libggml_hip.so")]

DB = ggml_hip.DeviceBuffer
KS = (64, 2304, 4160)
GEMV, GEMM, EXACT = 1, 2, 4


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_bitwise(got, ref):
    diff = np.flatnonzero(bits(got).ravel() != bits(ref).ravel())
    assert diff.size == 0, f"{diff.size} of {got.size} differ; first at {diff[:4]}: {np.ravel(got)[diff[:4]]} vs " \
                           f"{np.ravel(ref)[diff[:4]]}"


def rng_for(*key):
    return np.random.default_rng([0x80, *key])


def quantized_weights(rng, M, K):
    """Q8_0 rows of N(0, 0.02) weights (the oracle's bit-exact quantize_row_q8_0)."""
    return np.ascontiguousarray(O.quantize_q8_0((rng.standard_normal((M, K)) * 0.02).astype(np.float32)))


def split(wq, x, K):
    """(y_ref f32 [N, M], S_abs f64 [N, M]) of Q8_0 weights against the q8_0 of x: y_ref is the restatement of the
    reference's AVX2 vec_dot, S_abs = sum_b |d_w d_x isum_b| from the Q8_0 block terms (parity.check_y's scale)."""
    xq = O.quantize_q8_0(x)
    _, s_abs = R.block_terms(wq, xq, K)
    return R.vec_dot_avx2(wq, xq, K), s_abs


def gpu_mul_mat(wq, K, x, algo=0, ldy=None, fill=None, w_off=0):
    M, N = wq.shape[0], x.shape[0]
    ld = M if ldy is None else ldy
    if w_off:
        host = np.zeros(w_off + wq.nbytes + 64, np.uint8)
        host[w_off:w_off + wq.nbytes] = wq.ravel()
        wd = DB.from_array(host)
    else:
        wd = DB.from_array(wq)
    xd = DB.from_array(x)
    yd = DB.from_array(np.full((N, ld), np.float32(0 if fill is None else fill), np.float32))
    ggml_hip.mul_mat_q8_0(wd, K, M, xd, N, yd, algo=algo, ldy=ld, w_off=w_off)
    return yd.download((N, ld), np.float32)


@pytest.fixture
def exact_off():
    L = ggml_hip.load()
    prev = L.ggml_hip_get_exact()
    L.ggml_hip_set_exact(0)
    yield L
    L.ggml_hip_set_exact(prev)


@pytest.fixture
def policy():
    L = ggml_hip.load()
    L.ggml_hip_debug_set_q8_0_gemv_policy.argtypes = [ctypes.c_int] * 3
    yield lambda mp, depth, wg: ggml_hip.check(L.ggml_hip_debug_set_q8_0_gemv_policy(mp, depth, wg), "policy")
    L.ggml_hip_debug_set_q8_0_gemv_policy(-1, 0, 0)


# ---- exact mode -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", KS)
def test_exact_fixture_bitwise(exact_off, K):
    wq, x, y = load("q8w", f"w{K}_q8_0"), load("q8w", f"x{K}_f32"), load("q8w", f"y{K}_vec_dot")
    assert_bitwise(gpu_mul_mat(wq, K, x, algo=EXACT), y)                    # N = 3
    assert_bitwise(gpu_mul_mat(wq, K, x[:1], algo=EXACT), y[:1])            # N = 1
    assert_bitwise(y, R.vec_dot_avx2(wq, load("q8w", f"x{K}_q8_0"), K))     # the restatement
    exact_off.ggml_hip_set_exact(1)
    assert_bitwise(gpu_mul_mat(wq, K, x, algo=0), y)


def test_exact_crafted_blocks_bitwise(exact_off):
    wq, x, y = load("q8w", "craft_q8_0"), load("q8w", "craft_x_f32"), load("q8w", "craft_y")
    assert_bitwise(gpu_mul_mat(wq, 64, x, algo=EXACT), y)
    assert_bitwise(gpu_mul_mat(wq, 64, x[2:3], algo=EXACT), y[2:3])


@pytest.mark.parametrize("N", [1, 3])
def test_exact_long_row_bitwise(exact_off, N):
    K, M = 11008, 5
    rng = rng_for(1, N)
    wq = quantized_weights(rng, M, K)
    x = rng.standard_normal((N, K)).astype(np.float32)
    assert_bitwise(gpu_mul_mat(wq, K, x, algo=EXACT), R.vec_dot_avx2(wq, O.quantize_q8_0(x), K))


def test_exact_full_range_weights_bitwise(exact_off):
    K, M, N = 2304, 33, 9
    rng = rng_for(2)
    wq = R.random_q8_0(rng, M, K)
    x = rng.standard_normal((N, K)).astype(np.float32)
    assert_bitwise(gpu_mul_mat(wq, K, x, algo=EXACT, ldy=40, fill=2.5)[:, :M], R.vec_dot_avx2(wq, O.quantize_q8_0(x), K))


# ---- GEMV -------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def gemv_pin_case(K, M):
    """Weights (quantized rows, the first min(M // 2, 64) of them full-range blocks with the crafted ones), 9
    activation rows and the restated GEMV order on them: computed once per shape, shared by the token counts."""
    rng = rng_for(20, K, M)
    wq = quantized_weights(rng, M, K)
    ns = min(M // 2, 64)
    if ns:
        wq[:ns] = R.random_q8_0(rng, ns, K, special=True)
    x = rng.standard_normal((9, K)).astype(np.float32)
    y = R.gemv_schedule(wq, x, K)
    for a in (wq, x, y):
        a.setflags(write=False)
    return wq, x, y


@pytest.mark.parametrize("N", [1, 3, 8, 9])
@pytest.mark.parametrize("K,M", [(64, 1), (64, 8209), (4160, 33)])
def test_gemv_bitwise_restated_schedule(exact_off, K, M, N):
    """algo = GEMV is bitwise q8_0w_ref.gemv_schedule.  K = 64: one pair and 63 idle lanes; 4160: 65 pairs, a second
    chunk of one pair; M = 8209 at K = 64: more rows than waves under the auto grid rule, so the ring crosses
    row ends; M = 33: the last workgroup holds one row; N = 8: the full token tile, 9: a tile of 8 and one of 1."""
    wq, x, y_ref = gemv_pin_case(K, M)
    assert_bitwise(gpu_mul_mat(wq, K, x[:N], algo=GEMV), y_ref[:N])


@functools.lru_cache(maxsize=None)
def gemv_case(K):
    """Weights (130 rows, the crafted extremes in rows 0 .. 2 at K = 64), 8 activation rows, and their reference:
    computed once per K and shared by the GEMV tests."""
    rng = rng_for(3, K)
    wq = quantized_weights(rng, 130, K)
    x = rng.standard_normal((8, K)).astype(np.float32)
    if K == 64:
        wq[:3] = load("q8w", "craft_q8_0")[:3]
        x[6:8] = load("q8w", "craft_x_f32")[1:3]
    y_ref, s_abs = split(wq, x, K)
    for a in (wq, x, y_ref, s_abs):
        a.setflags(write=False)
    return wq, x, y_ref, s_abs


@pytest.mark.parametrize("K,M", [(K, M) for K in (64, 4096, 4160, 11008) for M in (1, 65, 130)])
def test_gemv_within_parity_bound(exact_off, K, M):
    """N = 1, 2, 8; the project's bound 1e-3 |y| + 1e-6 S_abs.  K = 64: one pair; 4096: one full wave-load; 4160:
    65 pairs; 11008: two full loads and a ragged tail (and token tiles of 5).  M = 1, 65, 130: ragged waves and
    more than one workgroup."""
    wq, x, y_ref, s_abs = gemv_case(K)
    for N in (1, 2, 8):
        y = gpu_mul_mat(np.ascontiguousarray(wq[:M]), K, x[:N], algo=GEMV, ldy=M + 3, fill=-7.5)
        assert np.all(y[:, M:] == np.float32(-7.5))                          # ldy > M: the gap untouched
        check_y(y[:, :M], y_ref[:N, :M], s_abs[:N, :M], rtol=1e-3, atol_blocks=1e-6)


@pytest.mark.parametrize("k", [1, 2, 3])
def test_gemv_weight_base_offset_in_allocation(exact_off, k):
    """The weight at 16 k bytes inside a larger allocation, K = 64: rows of 68 bytes sit at 4, 8 and 12 mod 16."""
    K, M = 64, 37
    wq, x, y_ref, s_abs = gemv_case(K)
    w = np.ascontiguousarray(wq[:M])
    base = gpu_mul_mat(w, K, x, algo=GEMV)
    check_y(base, y_ref[:, :M], s_abs[:, :M], rtol=1e-3, atol_blocks=1e-6)
    assert_bitwise(gpu_mul_mat(w, K, x, algo=GEMV, w_off=16 * k), base)
    assert_bitwise(gpu_mul_mat(w, K, x[:3], algo=EXACT, w_off=16 * k), gpu_mul_mat(w, K, x[:3], algo=EXACT))


@pytest.mark.parametrize("K", [64, 4160, 11008])
def test_gemv_launch_policies_bitwise(exact_off, policy, K):
    M = 130
    wq, x, _, _ = gemv_case(K)
    ref = {N: gpu_mul_mat(wq, K, x[:N], algo=GEMV) for N in (1, 3)}
    for mp, depth, wg in ((0, 1, 1), (1, 2, 2), (2, 1, 2), (2, 2, 1), (1, 1, 1)):
        policy(mp, depth, wg)
        for N in (1, 3):
            assert_bitwise(gpu_mul_mat(wq, K, x[:N], algo=GEMV), ref[N])
    assert M == wq.shape[0]


@pytest.mark.parametrize("N", [9, 17])
def test_gemv_column_tiles_bitwise_per_tile_calls(exact_off, N):
    K, M = 4160, 37
    rng = rng_for(4, N)
    wq = quantized_weights(rng, M, K)
    x = rng.standard_normal((N, K)).astype(np.float32)
    y = gpu_mul_mat(wq, K, x, algo=GEMV)
    for n0 in range(0, N, 8):
        assert_bitwise(y[n0:n0 + 8], gpu_mul_mat(wq, K, x[n0:n0 + 8], algo=GEMV))
    y_ref, s_abs = split(wq, x, K)
    check_y(y, y_ref, s_abs, rtol=1e-3, atol_blocks=1e-6)


def test_gemv_doubling_x_doubles_y_bitwise(exact_off):
    K, M, N = 4160, 50, 3
    rng = rng_for(5)
    wq = quantized_weights(rng, M, K)
    x = rng.standard_normal((N, K)).astype(np.float32)
    for algo in (GEMV, GEMM, EXACT):
        assert_bitwise(gpu_mul_mat(wq, K, 2 * x, algo=algo), 2 * gpu_mul_mat(wq, K, x, algo=algo))


# ---- GEMM: small values, bitwise the q4_0 path on the same image --------------------------------------------

@pytest.mark.parametrize("K,N", [(K, N) for K in (64, 4160) for N in (9, 129, 200)])
def test_gemm_bitwise_q4_0_gemm8_on_equal_values(exact_off, K, N):
    """A q4_0 matrix and its Q8_0 twin (qs = nibble - 8, the same d) give byte-identical k_gemm8 images, so algo 2
    on the twin is bitwise ggml_hip_mul_mat_q4_0_ex(algo 2) under GEMM version 9 (k_gemm8 on a per-call image).
    M = 70: a ragged 64-row tile."""
    L = exact_off
    M = 70
    rng = rng_for(6, K, N)
    w4q, _ = O.quantize_q4_0((rng.standard_normal((M, K)) * 0.02).astype(np.float32))
    w4q = np.ascontiguousarray(w4q)
    w8q = R.q4_0_as_q8_0(w4q, K)
    x = rng.standard_normal((N, K)).astype(np.float32)
    y8 = gpu_mul_mat(w8q, K, x, algo=GEMM)
    ggml_hip.check(L.ggml_hip_debug_set_gemm_version(9), "gemm version")
    try:
        w4d, xd, yd = DB.from_array(w4q), DB.from_array(x), DB(N * M * 4)
        ggml_hip.mul_mat(w4d, K, M, xd, N, yd, algo=2)
        y4 = yd.download((N, M), np.float32)
    finally:
        L.ggml_hip_debug_set_gemm_version(-1)
    assert_bitwise(y8, y4)
    assert np.any(y8 != 0)


# ---- GEMM: full-range weights -----------------------------------------------------------------------------

@pytest.mark.parametrize("M,N", [(M, N) for M in (64, 70) for N in (9, 130)])
def test_gemm_full_range_within_parity_bound(exact_off, M, N):
    K = 4160
    rng = rng_for(7, M, N)
    wq = R.random_q8_0(rng, M, K, special=False)
    d = np.float16(0.0123).view(np.uint16)
    blocks = wq.reshape(M, K // 32, 34)
    blocks[0, :, 2:] = 0x80                                                  # a row of all -128
    blocks[1, :, 2:] = 0x7F                                                  # a row of all +127
    blocks[2, :, 2::2], blocks[2, :, 3::2] = 0x7F, 0x81                      # alternating +-127
    blocks[:3, :, 0:2] = np.array([d], np.uint16).view(np.uint8)
    x = rng.standard_normal((N, K)).astype(np.float32)
    x[0], x[1, ::2], x[1, 1::2] = 2.0, 2.0, -2.0                              # x at +-amax: every q = +-127
    y_ref, s_abs = split(wq, x, K)
    y = gpu_mul_mat(wq, K, x, algo=GEMM, ldy=M + 5, fill=-7.5)
    assert np.all(y[:, M:] == np.float32(-7.5))
    check_y(y[:, :M], y_ref, s_abs, rtol=1e-3, atol_blocks=1e-6)
    extreme = -128.0 * 127 * K * float(np.float16(0.0123)) * float(np.float16(np.float32(2.0) / np.float32(127)))
    assert abs(float(y_ref[0, 0]) / extreme - 1) < 1e-5                      # the all -128 row against all +127


def test_gemm_crafted_blocks_within_parity_bound(exact_off):
    wq, x = load("q8w", "craft_q8_0"), load("q8w", "craft_x_f32")
    xx = np.ascontiguousarray(np.tile(x, (3, 1))[:9])
    y_ref, s_abs = split(wq, xx, 64)
    for algo in (GEMM, GEMV):
        check_y(gpu_mul_mat(wq, 64, xx, algo=algo), y_ref, s_abs, rtol=1e-3, atol_blocks=1e-6)


def test_auto_switches_at_the_threshold(exact_off):
    L = exact_off
    K, M = 256, 70
    rng = rng_for(8)
    wq = quantized_weights(rng, M, K)
    x = rng.standard_normal((12, K)).astype(np.float32)
    prev = L.ggml_hip_debug_set_q8_0_gemm_min_n(12)
    try:
        assert L.ggml_hip_debug_q8_0_auto_algo(K, M, 11) == GEMV and L.ggml_hip_debug_q8_0_auto_algo(K, M, 12) == GEMM
        assert_bitwise(gpu_mul_mat(wq, K, x[:11], algo=0), gpu_mul_mat(wq, K, x[:11], algo=GEMV))
        assert_bitwise(gpu_mul_mat(wq, K, x, algo=0), gpu_mul_mat(wq, K, x, algo=GEMM))
    finally:
        L.ggml_hip_debug_set_q8_0_gemm_min_n(prev)


# ---- dequantize, capture, status ----------------------------------------------------------------------------

@pytest.mark.parametrize("K", KS)
def test_dequantize_fixture_bitwise(K):
    ref = load("q8w", f"w{K}_dequant")
    wq = np.ascontiguousarray(load("q8w", f"w{K}_q8_0")[:ref.shape[0]])
    wd, od = DB.from_array(wq), DB(ref.nbytes)
    ggml_hip.dequantize_q8_0(wd, K, ref.shape[0], od)
    assert_bitwise(od.download(ref.shape, np.float32), ref)


def test_dequantize_crafted_bitwise():
    wq, ref = load("q8w", "craft_q8_0"), load("q8w", "craft_dequant")
    wd, od = DB.from_array(wq), DB(ref.nbytes)
    ggml_hip.dequantize_q8_0(wd, 64, wq.shape[0], od)
    assert_bitwise(od.download(ref.shape, np.float32), ref)


def test_graph_capture_replays_gemv_and_gemm(exact_off):
    L = exact_off
    K, M, N = 2304, 70, 20
    rng = rng_for(9)
    wq = quantized_weights(rng, M, K)
    x = rng.standard_normal((N, K)).astype(np.float32)
    eager1, eagerN = gpu_mul_mat(wq, K, x[:1], algo=GEMV), gpu_mul_mat(wq, K, x, algo=GEMM)
    wd, xd, y1d, yNd = DB.from_array(wq), DB.from_array(x), DB(M * 4), DB(N * M * 4)
    ggml_hip.check(L.ggml_hip_reserve_workspace_mm(K, N, M), "reserve")
    s = L.ggml_hip_default_stream()
    g = ggml_hip.Graph(s)
    with g:
        ggml_hip.mul_mat_q8_0(wd, K, M, xd, 1, y1d, algo=GEMV, stream=s)
        ggml_hip.mul_mat_q8_0(wd, K, M, xd, N, yNd, algo=GEMM, stream=s)
    for _ in range(2):
        ggml_hip.check(L.ggml_hip_memset(y1d.ptr, 0xFF, M * 4, s))
        ggml_hip.check(L.ggml_hip_memset(yNd.ptr, 0xFF, N * M * 4, s))
        g.launch()
        ggml_hip.check(L.ggml_hip_stream_synchronize(s))
        assert_bitwise(y1d.download((1, M), np.float32), eager1)
        assert_bitwise(yNd.download((N, M), np.float32), eagerN)


def test_status_codes(exact_off):
    L = exact_off
    b = DB(1 << 16)
    mm = L.ggml_hip_mul_mat_q8_0
    assert mm(b.ptr, 96, 4, b.ptr, 1, b.ptr, 4, 0, None) == ggml_hip.ERR_INVALID        # K % 64
    assert mm(b.ptr, 32, 4, b.ptr, 1, b.ptr, 4, 0, None) == ggml_hip.ERR_INVALID
    assert L.ggml_hip_dequantize_q8_0(b.ptr, 48, 1, b.ptr, None) == ggml_hip.ERR_INVALID
    assert mm(b.ptr, 64, 4, b.ptr, 1, b.ptr, 3, 0, None) == ggml_hip.ERR_INVALID         # ldy < M
    for algo in (3, 5, -1, 9):
        assert mm(b.ptr, 64, 4, b.ptr, 1, b.ptr, 4, algo, None) == ggml_hip.ERR_INVALID  # algo
    assert mm(None, 64, 4, b.ptr, 1, b.ptr, 4, 0, None) == ggml_hip.ERR_INVALID
    assert mm(b.ptr, 64, 4, b.ptr, 0, b.ptr, 4, 0, None) == ggml_hip.OK                  # N = 0
    for algo in (3, 5, 6, -1):
        assert mm(b.ptr, 64, 4, b.ptr, 0, b.ptr, 4, algo, None) == ggml_hip.OK           # N = 0 returns before the algo check
    assert mm(b.ptr, 64, 4, None, 1, b.ptr, 4, 0, None) == ggml_hip.ERR_INVALID
    assert mm(b.ptr, 64, 4, b.ptr, 1, None, 4, 0, None) == ggml_hip.ERR_INVALID
    assert mm(b.ptr, 64, 4, b.ptr + 4, 1, b.ptr, 4, 0, None) == ggml_hip.ERR_INVALID     # x not 16-byte aligned
    assert mm(b.ptr, 64, 4, b.ptr, 1, b.ptr + 2, 4, 0, None) == ggml_hip.ERR_INVALID     # y not 4-byte aligned
    assert mm(b.ptr + 2, 64, 4, b.ptr, 1, b.ptr, 4, 0, None) == ggml_hip.ERR_INVALID     # W not 4-byte aligned
    # K = 58304: 1822 blocks, one token's q8_0 (36 bytes per block) is past the GEMV's 64 KiB of LDS
    assert mm(b.ptr, 58304, 4, b.ptr, 0, b.ptr, 4, 1, None) == ggml_hip.OK               # nothing to run
    assert mm(b.ptr, 58304, 4, b.ptr, 1, b.ptr, 4, 1, None) == ggml_hip.ERR_UNSUPPORTED  # (refused before any launch)
    for algo in (0, 1, 2, 4):
        assert mm(b.ptr, 64, 4, b.ptr, 1, b.ptr, 4, algo, None) == ggml_hip.OK
    ggml_hip.synchronize()


# ---- hook path ----------------------------------------------------------------------------------------------

def q8_tensor(wq, K, M, backend=ggml_hip.GGML_BACKEND_CPU):
    return ggml_hip.make_tensor(ggml_hip.GGML_TYPE_Q8_0, (K, M), wq, backend=backend)


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


def test_hook_can_mul_mat(exact_off):
    L = exact_off
    N, M = 64, 64
    # a large host weight at prefill and at decode (2^19 elements: the residency cache's threshold)
    K = 256
    w = q8_tensor(np.zeros((2048, 34 * K // 32), np.uint8), K, 2048)
    for n in (N, 1):
        y, xt = mm_node(w, np.zeros((n, K), np.float32), np.zeros((n, 2048), np.float32))
        assert L.ggml_hip_can_mul_mat(ctypes.byref(w), ctypes.byref(xt), ctypes.byref(y))
    small = q8_tensor(np.zeros((1024, 34 * K // 32), np.uint8), K, 1024)          # below it: ggml's CPU op at N = 1
    ys, xs = mm_node(small, np.zeros((1, K), np.float32), np.zeros((1, 1024), np.float32))
    assert not L.ggml_hip_can_mul_mat(ctypes.byref(small), ctypes.byref(xs), ctypes.byref(ys))
    # K % 64 != 0
    K = 96
    w = q8_tensor(np.zeros((M, 34 * K // 32), np.uint8), K, M)
    y, xt = mm_node(w, np.zeros((N, K), np.float32), np.zeros((N, M), np.float32))
    assert not L.ggml_hip_can_mul_mat(ctypes.byref(w), ctypes.byref(xt), ctypes.byref(y))
    assert not forward(L, y)
    # non-contiguous src1
    K = 128
    w = q8_tensor(np.zeros((M, 34 * K // 32), np.uint8), K, M)
    y, xt = mm_node(w, np.zeros((N, 2 * K), np.float32), np.zeros((N, M), np.float32))
    xt.ne[0] = K
    xt.nb[2] = xt.nb[3] = xt.nb[1] * N
    assert not L.ggml_hip_can_mul_mat(ctypes.byref(w), ctypes.byref(xt), ctypes.byref(y))
    assert not forward(L, y)
    xt.nb[1] = 4 * K
    xt.nb[2] = xt.nb[3] = xt.nb[1] * N
    assert L.ggml_hip_can_mul_mat(ctypes.byref(w), ctypes.byref(xt), ctypes.byref(y))


@pytest.mark.parametrize("backend", [ggml_hip.GGML_BACKEND_GPU, ggml_hip.GGML_BACKEND_GPU_SPLIT])
@pytest.mark.parametrize("N", [1, 40])
def test_hook_transformed_weight(exact_off, backend, N):
    """A layer matrix's operand placement: weight uploaded by transform_tensor (device weight: can_mul_mat holds),
    host x, host dst; fast mode bitwise the direct call, exact mode bitwise the restatement."""
    L = exact_off
    K, M = 2304, 101
    rng = rng_for(12, 2, N)
    wq = quantized_weights(rng, M, K)
    x = rng.standard_normal((N, K)).astype(np.float32)
    staged = wq.copy()
    w = q8_tensor(staged, K, M, backend)
    L.ggml_hip_transform_tensor(staged.ctypes.data_as(ctypes.c_void_p), ctypes.byref(w))
    assert w.extra and w.backend == backend
    staged[:] = 0                                              # the loader frees its buffer
    y_np = np.zeros((N, M), np.float32)
    y, xt = mm_node(w, x, y_np)
    assert bool(L.ggml_hip_can_mul_mat(ctypes.byref(w), ctypes.byref(xt), ctypes.byref(y))) == (N >= 32)
    before = mul_mat_count(L)
    assert forward(L, y)
    assert mul_mat_count(L) == before + 1
    assert_bitwise(y_np, gpu_mul_mat(wq, K, x))
    L.ggml_hip_set_exact(1)
    y_np[:] = 0
    assert forward(L, y)
    assert_bitwise(y_np, R.vec_dot_avx2(wq, O.quantize_q8_0(x), K))
    L.ggml_hip_free_data(ctypes.byref(w))
    assert not w.extra


def test_hook_host_weight_residency_cache(exact_off):
    L = exact_off
    K, M = 256, 2048                                           # 2^19 elements: taken at N = 1
    rng = rng_for(12, 3)
    wq = quantized_weights(rng, M, K)
    x = rng.standard_normal((1, K)).astype(np.float32)
    y_np = np.zeros((1, M), np.float32)
    w = q8_tensor(wq, K, M)
    y, xt = mm_node(w, x, y_np)
    assert L.ggml_hip_can_mul_mat(ctypes.byref(w), ctypes.byref(xt), ctypes.byref(y))
    h, m, r = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    ggml_hip.check(L.ggml_hip_weight_cache_stats(ctypes.byref(h), ctypes.byref(m), ctypes.byref(r)))
    hits0, miss0 = h.value, m.value
    assert forward(L, y)
    ggml_hip.check(L.ggml_hip_weight_cache_stats(ctypes.byref(h), ctypes.byref(m), ctypes.byref(r)))
    assert (h.value, m.value) == (hits0, miss0 + 1)            # one miss ...
    first = y_np.copy()
    y_np[:] = 0
    assert forward(L, y)
    ggml_hip.check(L.ggml_hip_weight_cache_stats(ctypes.byref(h), ctypes.byref(m), ctypes.byref(r)))
    assert (h.value, m.value) == (hits0 + 1, miss0 + 1)        # ... then one hit
    assert_bitwise(y_np, first)
    assert_bitwise(y_np, gpu_mul_mat(wq, K, x))
    L.ggml_hip_weight_cache_invalidate(wq.ctypes.data_as(ctypes.c_void_p), wq.nbytes)


def test_fusion_on_off_bitwise(exact_off):
    """A small graph on the device: a q4_0 mul_mat (held by the hook's scheduler when fusion is on), an add on its
    output, and a Q8_0 mul_mat on disjoint buffers.  The Q8_0 node joins no group or chain; every output is bitwise
    the same with fusion on and off."""
    L = exact_off
    L.ggml_hip_debug_set_fuse.argtypes = [ctypes.c_int]
    GGML_OP_ADD = 2
    K, M4, M8 = 256, 48, 40
    rng = rng_for(13)
    w4q, _ = O.quantize_q4_0((rng.standard_normal((M4, K)) * 0.02).astype(np.float32))
    w4q = np.ascontiguousarray(w4q)
    w8q = quantized_weights(rng, M8, K)
    x4 = rng.standard_normal((1, K)).astype(np.float32)
    x8 = rng.standard_normal((1, K)).astype(np.float32)
    bias = rng.standard_normal((1, M4)).astype(np.float32)

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
        bt = ggml_hip.make_tensor(ggml_hip.GGML_TYPE_F32, (M4, 1), bias, backend=ggml_hip.GGML_BACKEND_GPU)
        L.ggml_hip_transform_tensor(bias.ctypes.data_as(ctypes.c_void_p), ctypes.byref(bt))
        sum_host = np.zeros((1, M4), np.float32)
        st = ggml_hip.make_tensor(ggml_hip.GGML_TYPE_F32, (M4, 1), sum_host)
        st.op = GGML_OP_ADD
        st.src0, st.src1 = ctypes.pointer(y4), ctypes.pointer(bt)
        L.ggml_hip_assign_buffers_no_scratch(ctypes.byref(st))
        assert st.backend == ggml_hip.GGML_BACKEND_GPU and st.extra
        w8 = q8_tensor(w8q, K, M8, ggml_hip.GGML_BACKEND_GPU)
        L.ggml_hip_transform_tensor(w8q.ctypes.data_as(ctypes.c_void_p), ctypes.byref(w8))
        y8_host = np.zeros((1, M8), np.float32)
        y8, _ = mm_node(w8, x8, y8_host)
        assert forward(L, y4)
        assert forward(L, st)
        assert forward(L, y8)
        for t, host in ((y4, y4_host), (st, sum_host)):
            dev = ctypes.cast(t.extra, ctypes.POINTER(ctypes.c_void_p * 16)).contents[0]
            ggml_hip.check(L.ggml_hip_memcpy_d2h(host.ctypes.data_as(ctypes.c_void_p), dev, host.nbytes, None))
        for t in (st, y4, x4t, bt, w4, w8):
            L.ggml_hip_free_data(ctypes.byref(t))
        return y4_host, sum_host, y8_host

    try:
        on = run(1)
        off = run(0)
    finally:
        L.ggml_hip_debug_set_fuse(1)
    for a, b in zip(on, off):
        assert_bitwise(a, b)
    assert_bitwise(on[2], gpu_mul_mat(w8q, K, x8))
    assert_bitwise(on[1], on[0] + bias)
    assert np.any(on[0] != 0)
