"""The Q5_K / Q4_K prefill GEMM on the device (csrc/q45_k_gemm.hip, algo 6 of ggml_hip_mul_mat_q5_K / _q4_K): every
y bit for bit the GEMV schedule (tests/q45k_ref.gemv_schedule, independent of the device) and bit for bit the device
GEMV (algo 1), on random and crafted blocks, ragged tiles, every tile shape, beyond the GEMV's K, strided outputs,
under graph capture, across the auto threshold and through the ggml hook path."""
import ctypes

import numpy as np
import pytest

import q45k_gemm_ref as G
import q45k_ref as R
from hip_env import ggml_hip, gpu_available
from parity import check_y
from test_gpu_q45k import (BOTH, GTYPE, HOOK_BOTH, assert_bitwise, exact_off, forward, gpu_mul_mat,   # noqa: F401
                           hook, k_tensor, mm_node, qh_of)

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason="needs a HIP device and libggml_hip.so")]

DB = ggml_hip.DeviceBuffer
GEMM, GEMV = 6, 1


def rng_for(*key):
    return np.random.default_rng([0x46, *key])


@pytest.fixture
def min_n(exact_off):
    """the setter of the auto threshold; the value found is put back afterwards, also when the test fails"""
    setter = exact_off.ggml_hip_debug_set_q45k_gemm_min_n
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
    and odd counts; M: ragged and several row tiles; N: one column, a ragged 32-tile, two MFMA tiles."""
    qh = qh_of(variant)
    rng = rng_for(1, qh, K)
    wq = R.random_q45_K(rng, 130, K, qh)
    x = (rng.standard_normal((33, K)) * 3).astype(np.float32)
    ref = R.gemv_schedule(wq, x, K, qh)
    for M in (1, 37, 64, 65, 130):
        for N in (1, 9, 33):
            assert_bitwise(gpu_mul_mat(variant, wq[:M], K, x[:N], algo=GEMM), ref[:N, :M])


@BOTH
def test_gemm_extremes_bitwise_gemv_schedule(exact_off, variant):
    """Every sc = m = 63 and every q at its maximum, with ordinary, zero and subnormal d / dmin.  q8_K gives a
    block's extreme element -128 whatever its sign, so the rows of all +1 and of all -1 are both all -128: bsum32 =
    -4096 and isum at its bound.  bsum32 = 4064 = 32 * 127 needs +128s clamped to 127, the extreme elsewhere: the
    rows whose first element has the other sign."""
    qh = qh_of(variant)
    qmax = G.Q_MAX[qh]
    ds = [np.float16(0.0123), np.float16(-1.5), np.float16(0.0), np.uint16(0x0001).view(np.float16),
          np.uint16(0x83FF).view(np.float16)]
    pairs = [(a, b) for a in ds for b in ds]
    n = len(pairs)
    wq = G.pack_q45_K(np.full((n, 1, 8, 32), qmax), np.full((n, 1, 8), 63), np.full((n, 1, 8), 63),
                      np.array([p[0] for p in pairs], np.float16).reshape(n, 1),
                      np.array([p[1] for p in pairs], np.float16).reshape(n, 1), qh)
    x = np.stack([np.full(256, 1.0), np.full(256, -1.0), np.full(256, 1.0), np.full(256, -1.0),
                  np.where(np.arange(256) & 1, -2.0, 2.0)]).astype(np.float32)
    x[2, 0], x[3, 0] = -1.0, 1.0
    xq = R.quantize_q8_K(x)
    s = G.bsum32(xq, 256)
    assert np.all(s[0] == -4096) and np.all(s[1] == -4096)
    assert np.all(s[2, 0, 1:] == 4064) and np.all(s[3, 0, 1:] == 4064)
    isum, msum = G.sums_from_digits(wq, xq, 256, qh)
    assert isum.min() == -63 * qmax * 128 * 256 and msum.min() == -8 * 63 * 4096      # the ranges' ends are reached
    ref = R.gemv_schedule(wq, x, 256, qh)
    assert_bitwise(gpu_mul_mat(variant, wq, 256, x, algo=GEMM), ref)
    assert_bitwise(gpu_mul_mat(variant, wq, 256, x, algo=GEMV), ref)


# ---- 2. against the device GEMV ---------------------------------------------------------------------------

@BOTH
def test_gemm_every_tile_shape_bitwise_gemv(exact_off, variant):
    """tiles of 64 columns up to N = 64, 128 up to 128, then 256; full and ragged, one and two column tiles"""
    qh = qh_of(variant)
    K, M = 512, 70
    rng = rng_for(2, qh)
    wq = R.random_q45_K(rng, M, K, qh)
    x = rng.standard_normal((300, K)).astype(np.float32)
    ref = gpu_mul_mat(variant, wq, K, x, algo=GEMV)
    for N in (64, 65, 128, 129, 257, 300):
        assert_bitwise(gpu_mul_mat(variant, wq, K, x[:N], algo=GEMM), ref[:N])


@BOTH
def test_gemm_widest_tile_bitwise_gemv(exact_off, variant):
    """The 256-column tile is taken only where the grid of 128-column tiles is larger than the device (one
    workgroup per CU): 131 row tiles (the last ragged) x 3 column tiles, more than any supported device's CUs."""
    qh = qh_of(variant)
    K, M = 256, 8321
    rng = rng_for(9, qh)
    wq = R.random_q45_K(rng, M, K, qh)
    x = rng.standard_normal((300, K)).astype(np.float32)
    ref = gpu_mul_mat(variant, wq, K, x, algo=GEMV)
    for N in (257, 300):
        assert_bitwise(gpu_mul_mat(variant, wq, K, x[:N], algo=GEMM), ref[:N])


@BOTH
def test_gemm_beyond_gemv_k(exact_off, variant):
    """K = 16640: the GEMM runs where the GEMV cannot; auto keeps taking the exact kernel there."""
    qh = qh_of(variant)
    K, M, N = 16640, 19, 9
    rng = rng_for(3, qh)
    wq = R.random_q45_K(rng, M, K, qh)
    x = rng.standard_normal((N, K)).astype(np.float32)
    xq = R.quantize_q8_K(x)
    y = gpu_mul_mat(variant, wq, K, x, algo=GEMM)
    assert_bitwise(y, R.gemv_schedule(wq, x, K, qh))
    y_exact, s_abs = R.block_terms(wq, xq, K, qh)
    check_y(y, y_exact, s_abs)
    assert_bitwise(gpu_mul_mat(variant, wq, K, x, algo=0), R.vec_dot_avx2(wq, xq, K, qh))


@BOTH
def test_gemm_ldy_gap_untouched(exact_off, variant):
    qh = qh_of(variant)
    K, M, N, ld = 512, 37, 70, 48
    rng = rng_for(4, qh)
    wq = R.random_q45_K(rng, M, K, qh)
    x = rng.standard_normal((N, K)).astype(np.float32)
    y = gpu_mul_mat(variant, wq, K, x, algo=GEMM, ldy=ld, fill=-7.5)
    assert np.all(y[:, M:] == np.float32(-7.5))
    assert_bitwise(y[:, :M], gpu_mul_mat(variant, wq, K, x, algo=GEMM))


@BOTH
def test_gemm_doubling_x_doubles_y_bitwise(exact_off, variant):
    qh = qh_of(variant)
    K, M, N = 2304, 50, 70
    rng = rng_for(5, qh)
    wq = R.random_q45_K(rng, M, K, qh, special=False)
    x = rng.standard_normal((N, K)).astype(np.float32)
    assert_bitwise(gpu_mul_mat(variant, wq, K, 2 * x, algo=GEMM), 2 * gpu_mul_mat(variant, wq, K, x, algo=GEMM))


@BOTH
def test_gemm_graph_capture_after_reserve(exact_off, variant):
    """After ggml_hip_reserve_workspace(K, N) a capture (which forbids growing the workspace) takes the GEMM."""
    L = exact_off
    qh = qh_of(variant)
    K, M, N = 2304, 150, 133
    rng = rng_for(6, qh)
    wq = R.random_q45_K(rng, M, K, qh)
    x = rng.standard_normal((N, K)).astype(np.float32)
    gpu_mul_mat(variant, wq[:1], K, x, algo=GEMM)               # (the tile's attributes are set outside the capture)
    eager = gpu_mul_mat(variant, wq, K, x, algo=GEMV)
    ggml_hip.check(L.ggml_hip_reserve_workspace(K, N))
    wd, xd, yd = DB.from_array(wq), DB.from_array(x), DB(N * M * 4)
    s = L.ggml_hip_default_stream()
    g = ggml_hip.Graph(s)
    with g:
        (ggml_hip.mul_mat_q5_K if qh else ggml_hip.mul_mat_q4_K)(wd, K, M, xd, N, yd, algo=GEMM, stream=s)
    for _ in range(2):
        ggml_hip.check(L.ggml_hip_memset(yd.ptr, 0xFF, N * M * 4, s))
        g.launch()
        ggml_hip.check(L.ggml_hip_stream_synchronize(s))
        assert_bitwise(yd.download((N, M), np.float32), eager)


@BOTH
def test_auto_threshold_switches_kernel_not_bits(exact_off, min_n, variant):
    L = exact_off
    qh = qh_of(variant)
    K, M, N = 768, 70, 33
    rng = rng_for(7, qh)
    wq = R.random_q45_K(rng, M, K, qh)
    x = rng.standard_normal((N, K)).astype(np.float32)
    min_n(9)
    assert L.ggml_hip_debug_q45k_auto_algo(GTYPE[variant], K, M, N) == GEMM
    y_gemm = gpu_mul_mat(variant, wq, K, x, algo=0)
    min_n(1 << 30)
    assert L.ggml_hip_debug_q45k_auto_algo(GTYPE[variant], K, M, N) == GEMV
    y_gemv = gpu_mul_mat(variant, wq, K, x, algo=0)
    assert_bitwise(y_gemm, y_gemv)
    assert_bitwise(y_gemm, gpu_mul_mat(variant, wq, K, x, algo=GEMM))
    assert_bitwise(y_gemv, gpu_mul_mat(variant, wq, K, x, algo=GEMV))


@BOTH
def test_gemm_status_codes(exact_off, variant):
    L = exact_off
    mm = L.ggml_hip_mul_mat_q5_K if qh_of(variant) else L.ggml_hip_mul_mat_q4_K
    b = DB(1 << 16)
    for algo in (2, 3, 5):
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
    qh = qh_of(variant)
    K, M, N = 768, 101, 33
    rng = rng_for(8, qh)
    wq = R.random_q45_K(rng, M, K, qh)
    x = rng.standard_normal((N, K)).astype(np.float32)
    min_n(9)
    assert L.ggml_hip_debug_q45k_auto_algo(GTYPE[variant], K, M, N) == GEMM
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
    assert_bitwise(y_np, R.gemv_schedule(wq, x, K, qh))
    assert_bitwise(y_np, gpu_mul_mat(variant, wq, K, x, algo=0))
    assert_bitwise(y_np, gpu_mul_mat(variant, wq, K, x, algo=GEMM))
