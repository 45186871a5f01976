"""The Q3_K / Q2_K prefill GEMM on the device (csrc/q23_k_gemm.hip, algo 8 of ggml_hip_mul_mat_q3_K / _q2_K): every
y bit for bit the GEMV schedule (tests/q23k_ref.gemv_schedule, independent of the device) and bit for bit the device
GEMV (algo 1), on random and crafted blocks, ragged tiles, every tile shape, beyond the GEMV's K, strided outputs,
under graph capture, across the auto threshold and through the ggml hook path.  Q3_K rows of an odd number of
superblocks (K = 256, 768, 2304 with M > 1) put every second row at 2 mod 4."""
import ctypes

import numpy as np
import pytest

import q23k_gemm_ref as G
import q23k_ref as R
from hip_env import ggml_hip, gpu_available
from parity import check_y
from test_gpu_q23k import (BOTH, GTYPE, HOOK_BOTH, assert_bitwise, exact_off, forward, gpu_mul_mat,   # noqa: F401
                           hook, k_tensor, mm_node, q3_of)

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason="needs a HIP device and libggml_hip.so")]

DB = ggml_hip.DeviceBuffer
GEMM, GEMV = 8, 1


def rng_for(*key):
    return np.random.default_rng([0x49, *key])


@pytest.fixture
def min_n(exact_off):
    """the setter of the auto threshold; the value found is put back afterwards, also when the test fails"""
    setter = exact_off.ggml_hip_debug_set_q23k_gemm_min_n
    prev = setter(-1)
    setter(prev)
    yield setter
    setter(prev)


# ---- 1. against the numpy schedule ------------------------------------------------------------------------

@BOTH
@pytest.mark.parametrize("K", [256, 768, 2304])
def test_gemm_bitwise_gemv_schedule(exact_off, variant, K):
    """Asymmetric random integers in both operands: a wrong A / B lane map or a transposed C / D map cannot pass.
    One numpy reference at the largest shape: an output depends on its own row and column only.  K: one superblock
    and odd counts (every second Q3_K row at 2 mod 4); M: ragged and several row tiles; N: one column, a ragged
    32-tile, two MFMA tiles."""
    q3 = q3_of(variant)
    rng = rng_for(1, q3, K)
    wq = R.random_q23_K(rng, 130, K, q3)
    x = (rng.standard_normal((33, K)) * 3).astype(np.float32)
    ref = R.gemv_schedule(wq, x, K, q3)
    for M in (1, 37, 64, 65, 130):
        for N in (1, 9, 33):
            assert_bitwise(gpu_mul_mat(variant, wq[:M], K, x[:N], algo=GEMM), ref[:N, :M])


def extreme_rows(q3):
    """Q3_K: the four corners (sc, q) in {-32, 31} x {-4, 3}, the first being sc q = 128 in every element; Q2_K: sc =
    m = 15, q = 3; each with ordinary, negative, zero and fp16-subnormal d (and, Q2_K, every pair with dmin)."""
    ds = [np.float16(0.0123), np.float16(-1.5), np.float16(0.0), np.uint16(0x0001).view(np.float16),
          np.uint16(0x83FF).view(np.float16)]
    if q3:
        rows = [(s, v, d, d) for (s, v) in ((-32, -4), (-32, 3), (31, -4), (31, 3)) for d in ds]
    else:
        rows = [(15, 3, a, b) for a in ds for b in ds]
    n = len(rows)
    q = np.empty((n, 1, 16, 16), np.int64)
    sc = np.empty((n, 1, 16), np.int64)
    for r, (s, v, _, _) in enumerate(rows):
        q[r], sc[r] = v, s
    return G.pack_q23_K(q, sc, None if q3 else sc, np.array([r[2] for r in rows], np.float16).reshape(n, 1),
                        np.array([r[3] for r in rows], np.float16).reshape(n, 1), q3)


@BOTH
def test_gemm_extremes_bitwise_gemv_schedule(exact_off, variant):
    """q8_K gives a block's extreme element -128 whatever its sign, so the rows of all +1 and of all -1 are both all
    -128: bsum16 = -2048 and, against the Q3_K rows of sc q = 128, isum = -2^22.  bsum16 = 2032 = 16 * 127 needs
    +128s clamped to 127, the extreme elsewhere: the rows whose first element has the other sign.  The integer
    bounds are asserted on the CPU before the device is touched."""
    q3 = q3_of(variant)
    wq = extreme_rows(q3)
    x = np.stack([np.full(256, 1.0), np.full(256, -1.0), np.full(256, 1.0), np.full(256, -1.0),
                  np.where(np.arange(256) & 1, -2.0, 2.0)]).astype(np.float32)
    x[2, 0], x[3, 0] = -1.0, 1.0
    xq = R.quantize_q8_K(x)
    s = G.bsum16(xq, 256)
    assert np.all(s[0] == -2048) and np.all(s[1] == -2048)
    assert np.all(s[2, 0, 1:] == 2032) and np.all(s[3, 0, 1:] == 2032)
    w = G.scaled_weights(wq, 256, q3)
    isum, msum = G.sums_from_planes(wq, xq, 256, q3)
    if q3:
        assert w.min() == -128 and w.max() == 124
        assert isum.min() == -2 ** 22                              # the ranges' ends are reached
    else:
        assert w.min() == 45 and isum.min() == -45 * 128 * 256
        assert msum.min() == -16 * 15 * 2048
    ref = R.gemv_schedule(wq, x, 256, q3)
    assert_bitwise(gpu_mul_mat(variant, wq, 256, x, algo=GEMM), ref)
    assert_bitwise(gpu_mul_mat(variant, wq, 256, x, algo=GEMV), ref)
    assert_bitwise(gpu_mul_mat(variant, wq, 256, x, algo=GEMM), gpu_mul_mat(variant, wq, 256, x, algo=GEMV))


# ---- 2. against the device GEMV ---------------------------------------------------------------------------

@BOTH
def test_gemm_every_tile_shape_bitwise_gemv(exact_off, variant):
    """tiles of 64 columns up to N = 64, 128 up to 128, then 256; full and ragged, one and two column tiles"""
    q3 = q3_of(variant)
    K, M = 512, 70
    rng = rng_for(2, q3)
    wq = R.random_q23_K(rng, M, K, q3)
    x = rng.standard_normal((300, K)).astype(np.float32)
    ref = gpu_mul_mat(variant, wq, K, x, algo=GEMV)
    for N in (64, 65, 128, 129, 257, 300):
        assert_bitwise(gpu_mul_mat(variant, wq, K, x[:N], algo=GEMM), ref[:N])


@BOTH
def test_gemm_widest_tile_bitwise_gemv(exact_off, variant):
    """The 256-column tile is taken only where the grid of 128-column tiles is larger than the device (one
    workgroup per CU): 131 row tiles (the last ragged) x 3 column tiles, more than any supported device's CUs."""
    q3 = q3_of(variant)
    K, M = 256, 8321
    rng = rng_for(9, q3)
    wq = R.random_q23_K(rng, M, K, q3)
    x = rng.standard_normal((300, K)).astype(np.float32)
    ref = gpu_mul_mat(variant, wq, K, x, algo=GEMV)
    for N in (257, 300):
        assert_bitwise(gpu_mul_mat(variant, wq, K, x[:N], algo=GEMM), ref[:N])


@BOTH
def test_gemm_beyond_gemv_k(exact_off, variant):
    """K = 16640: the GEMM runs where the GEMV cannot; auto keeps taking the exact kernel there."""
    q3 = q3_of(variant)
    K, M, N = 16640, 19, 9
    rng = rng_for(3, q3)
    wq = R.random_q23_K(rng, M, K, q3)
    x = rng.standard_normal((N, K)).astype(np.float32)
    xq = R.quantize_q8_K(x)
    y = gpu_mul_mat(variant, wq, K, x, algo=GEMM)
    assert_bitwise(y, R.gemv_schedule(wq, x, K, q3))
    y_exact, s_abs = R.block_terms(wq, xq, K, q3)
    check_y(y, y_exact, s_abs)
    assert_bitwise(gpu_mul_mat(variant, wq, K, x, algo=0), R.vec_dot_avx2(wq, xq, K, q3))


@BOTH
def test_gemm_ldy_gap_untouched(exact_off, variant):
    q3 = q3_of(variant)
    K, M, N, ld = 512, 37, 70, 48
    rng = rng_for(4, q3)
    wq = R.random_q23_K(rng, M, K, q3)
    x = rng.standard_normal((N, K)).astype(np.float32)
    y = gpu_mul_mat(variant, wq, K, x, algo=GEMM, ldy=ld, fill=-7.5)
    assert np.all(y[:, M:] == np.float32(-7.5))
    assert_bitwise(y[:, :M], gpu_mul_mat(variant, wq, K, x, algo=GEMM))


@BOTH
def test_gemm_doubling_x_doubles_y_bitwise(exact_off, variant):
    q3 = q3_of(variant)
    K, M, N = 2304, 50, 70
    rng = rng_for(5, q3)
    wq = R.random_q23_K(rng, M, K, q3, special=False)
    x = rng.standard_normal((N, K)).astype(np.float32)
    assert_bitwise(gpu_mul_mat(variant, wq, K, 2 * x, algo=GEMM), 2 * gpu_mul_mat(variant, wq, K, x, algo=GEMM))


@BOTH
def test_gemm_graph_capture_after_reserve(exact_off, variant):
    """After ggml_hip_reserve_workspace(K, N) a capture (which forbids growing the workspace) takes the GEMM."""
    L = exact_off
    q3 = q3_of(variant)
    K, M, N = 2304, 150, 133
    rng = rng_for(6, q3)
    wq = R.random_q23_K(rng, M, K, q3)
    x = rng.standard_normal((N, K)).astype(np.float32)
    gpu_mul_mat(variant, wq[:1], K, x, algo=GEMM)               # (the tile's attributes are set outside the capture)
    eager = gpu_mul_mat(variant, wq, K, x, algo=GEMV)
    ggml_hip.check(L.ggml_hip_reserve_workspace(K, N))
    wd, xd, yd = DB.from_array(wq), DB.from_array(x), DB(N * M * 4)
    s = L.ggml_hip_default_stream()
    g = ggml_hip.Graph(s)
    with g:
        (ggml_hip.mul_mat_q3_K if q3 else ggml_hip.mul_mat_q2_K)(wd, K, M, xd, N, yd, algo=GEMM, stream=s)
    for _ in range(2):
        ggml_hip.check(L.ggml_hip_memset(yd.ptr, 0xFF, N * M * 4, s))
        g.launch()
        ggml_hip.check(L.ggml_hip_stream_synchronize(s))
        assert_bitwise(yd.download((N, M), np.float32), eager)


@BOTH
def test_auto_threshold_switches_kernel_not_bits(exact_off, min_n, variant):
    L = exact_off
    q3 = q3_of(variant)
    K, M, N = 768, 70, 33
    rng = rng_for(7, q3)
    wq = R.random_q23_K(rng, M, K, q3)
    x = rng.standard_normal((N, K)).astype(np.float32)
    min_n(9)
    assert L.ggml_hip_debug_q23k_auto_algo(GTYPE[variant], K, M, N) == GEMM
    y_gemm = gpu_mul_mat(variant, wq, K, x, algo=0)
    min_n(1 << 30)
    assert L.ggml_hip_debug_q23k_auto_algo(GTYPE[variant], K, M, N) == GEMV
    y_gemv = gpu_mul_mat(variant, wq, K, x, algo=0)
    assert_bitwise(y_gemm, y_gemv)
    assert_bitwise(y_gemm, gpu_mul_mat(variant, wq, K, x, algo=GEMM))
    assert_bitwise(y_gemv, gpu_mul_mat(variant, wq, K, x, algo=GEMV))


@BOTH
def test_gemm_status_codes(exact_off, variant):
    L = exact_off
    mm = L.ggml_hip_mul_mat_q3_K if q3_of(variant) else L.ggml_hip_mul_mat_q2_K
    b = DB(1 << 16)
    for algo in (2, 3, 5, 6, 7):
        assert mm(b.ptr, 256, 4, b.ptr, 1, b.ptr, 4, algo, None) == ggml_hip.ERR_INVALID
    assert mm(b.ptr, 384, 4, b.ptr, 1, b.ptr, 4, GEMM, None) == ggml_hip.ERR_INVALID       # K % 256
    assert mm(b.ptr, 256, 4, b.ptr, 1, b.ptr, 3, GEMM, None) == ggml_hip.ERR_INVALID       # ldy < M
    assert mm(b.ptr, 256, 4, b.ptr, 0, b.ptr, 4, GEMM, None) == ggml_hip.OK                # N = 0
    # an algo the types reject is refused before anything else, an empty call included
    assert mm(b.ptr, 256, 4, b.ptr, 0, b.ptr, 4, 3, None) == ggml_hip.ERR_INVALID


# ---- 3. hook path -----------------------------------------------------------------------------------------

@HOOK_BOTH
@pytest.mark.parametrize("backend", [ggml_hip.GGML_BACKEND_GPU, ggml_hip.GGML_BACKEND_GPU_SPLIT])
def test_hook_takes_the_gemm(hook, min_n, backend):
    """A layer matrix's operand placement: weight uploaded by transform_tensor, host x, host dst; auto from N = 9."""
    L, variant = hook
    q3 = q3_of(variant)
    K, M, N = 768, 101, 33
    rng = rng_for(8, q3)
    wq = R.random_q23_K(rng, M, K, q3)
    x = rng.standard_normal((N, K)).astype(np.float32)
    min_n(9)
    assert L.ggml_hip_debug_q23k_auto_algo(GTYPE[variant], K, M, N) == GEMM
    staged = wq.copy()
    w = k_tensor(variant, staged, K, M, backend)
    L.ggml_hip_transform_tensor(staged.ctypes.data_as(ctypes.c_void_p), ctypes.byref(w))
    assert w.extra and w.backend == backend
    staged[:] = 0                                              # the loader frees its buffer
    y_np = np.zeros((N, M), np.float32)
    y, _ = mm_node(w, x, y_np)
    assert forward(L, y)
    L.ggml_hip_free_data(ctypes.byref(w))
    assert not w.extra
    assert_bitwise(y_np, R.gemv_schedule(wq, x, K, q3))
    assert_bitwise(y_np, gpu_mul_mat(variant, wq, K, x, algo=0))
    assert_bitwise(y_np, gpu_mul_mat(variant, wq, K, x, algo=GEMM))
