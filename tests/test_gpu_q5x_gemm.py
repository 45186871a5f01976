"""The Q4_1 / Q5_1 prefill GEMM on the device (csrc/q5x_gemm.hip, algo 7 of ggml_hip_mul_mat_q4_1 / _q5_1): every y
bit for bit the numpy schedule tests/q5x_gemm_ref.chain (independent of the device) on full-range and quantizer
weights, ragged stages, rows and columns, every tile shape, unaligned weights, beyond the GEMV's K, strided outputs,
under graph capture, across the types' own auto threshold, through the ggml hook path and through the reference's
llama.cpp end to end."""
import ctypes
import functools
import os

import numpy as np
import pytest

import q5x_gemm_ref as G
import q5x_ref as R
from conftest import ROOT
from hip_env import ggml_hip, gpu_available
from test_gpu_q5x import (GTYPE, NAME, assert_bitwise, exact_off, forward, gpu_mul_mat, mm_node,   # noqa: F401
                          mul_mat_count, quantized_weights, w_tensor)

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason="needs a HIP device and libggml_hip.so")]

DB = ggml_hip.DeviceBuffer
HIP_LIB = os.path.join(ROOT, "oracle", "_ref", "libllama_ref_hip.so")
GEMV, EXACT, GEMM = 1, 4, 7
TYPES = ("q41", "q51")
BOTH = pytest.mark.parametrize("t", TYPES)


def rng_for(*key):
    return np.random.default_rng([0x57, *key])


def activations(rng, N, K):
    """N(0, 1) rows; the first two (one where N = 1) at +-amax, so every q8 of them is +-127"""
    x = rng.standard_normal((N, K)).astype(np.float32)
    x[0] = 2.0
    if N > 1:
        x[1, ::2], x[1, 1::2] = 2.0, -2.0
    return x


@functools.lru_cache(maxsize=None)
def case(t, K, M, N):
    """(wq, x, chain) of a shape, computed once and shared: random_blocks weights for K <= 256 and at K = 4160 and
    above, quantizer weights at K = 2304."""
    rng = rng_for(1, GTYPE[t], K, M, N)
    wq = quantized_weights(t, rng, M, K) if K == 2304 else R.random_blocks(rng, M, K, R.has_qh(t), True)
    x = activations(rng, N, K)
    ref = G.chain(t, wq, R.quantize_x(t, x), K)
    for a in (wq, x, ref):
        a.setflags(write=False)
    return wq, x, ref


@pytest.fixture
def min_n(exact_off):
    """the setter of the types' auto threshold; the value found is put back afterwards, also when the test fails"""
    setter = exact_off.ggml_hip_debug_set_q41_q51_gemm_min_n
    prev = setter(-1)
    setter(prev)
    yield setter
    setter(prev)


def gemm_checked(t, wq, K, x, ref):
    """algo 7 into ldy = M + 5 over a fill value: the gap untouched, y not all zero, y bitwise ref"""
    M = wq.shape[0]
    y = gpu_mul_mat(t, np.ascontiguousarray(wq), K, np.ascontiguousarray(x), algo=GEMM, ldy=M + 5, fill=-7.5)
    assert np.all(y[:, M:] == np.float32(-7.5))
    assert np.any(y[:, :M] != 0)
    assert_bitwise(y[:, :M], ref)
    return y[:, :M]


# ---- 1. bitwise the numpy schedule --------------------------------------------------------------------------

@BOTH
@pytest.mark.parametrize("K,M,N", [(64, 70, 9),          # one pair, shorter than a stage
                                   (2304, 64, 33),       # whole stages, exact row tile
                                   (4160, 70, 130)])     # 65 pairs: a ragged stage; ragged rows; two column tiles
def test_gemm_bitwise_chain(exact_off, t, K, M, N):
    wq, x, ref = case(t, K, M, N)
    gemm_checked(t, wq, K, x, ref)
    if K == 4160:
        gemm_checked(t, wq, K, x[:1], ref[:1])           # N = 1


@BOTH
def test_gemm_every_tile_shape_bitwise_chain(exact_off, t):
    """K = 256, M = 130: three row tiles, the last ragged.  The launcher's column tiles: N <= 64 takes 64 columns
    ((WN, TN) = (2, 1): N = 9, 64), N <= 128 takes 128 ((4, 1): N = 65, 128), and above it 128 as long as the grid of
    128-column tiles fits on the device at once, as it does here ((4, 1) with two and three column tiles: N = 129,
    300).  The 256-column tile (4, 2) is test_gemm_widest_tile's."""
    K, M = 256, 130
    wq, x, ref = case(t, K, M, 300)
    for N in (9, 64, 65, 128, 129, 300):
        gemm_checked(t, wq, K, x[:N], ref[:N])


@BOTH
def test_gemm_widest_tile(exact_off, t):
    """(WN, TN) = (4, 2) is taken only where the grid of 128-column tiles is larger than the device: 131 row tiles
    (the last ragged) x 3 column tiles, more than any supported device's CUs.  y is bitwise the calls on 64-column
    slices, which run the (2, 1) tile, and its first and last rows are bitwise the numpy schedule."""
    K, M, N = 64, 8321, 300
    rng = rng_for(2, GTYPE[t])
    wq = R.random_blocks(rng, M, K, R.has_qh(t), True)
    x = activations(rng, N, K)
    y = gpu_mul_mat(t, wq, K, x, algo=GEMM)
    for n0 in range(0, N, 64):
        assert_bitwise(y[n0:n0 + 64], gpu_mul_mat(t, wq, K, x[n0:n0 + 64], algo=GEMM))
    xq = R.quantize_x(t, x)
    for rows in (slice(0, 70), slice(8256, 8321)):
        assert_bitwise(y[:, rows], G.chain(t, wq[rows], xq, K))


# ---- 2. independence, 3. doubling, 4. alignment --------------------------------------------------------------

@BOTH
def test_gemm_columns_and_rows_do_not_depend_on_the_call(exact_off, t):
    K, M, N = 4160, 70, 130
    wq, x, ref = case(t, K, M, N)
    y = gpu_mul_mat(t, wq, K, x, algo=GEMM)
    assert_bitwise(y, ref)
    for cols in (slice(9, 41), slice(129, 130)):
        assert_bitwise(y[cols], gpu_mul_mat(t, wq, K, np.ascontiguousarray(x[cols]), algo=GEMM))
    assert_bitwise(y[:, 64:70], gpu_mul_mat(t, np.ascontiguousarray(wq[64:70]), K, x, algo=GEMM))


@BOTH
def test_gemm_doubling_x_doubles_y_bitwise(exact_off, t):
    K, M, N = 2304, 50, 70
    rng = rng_for(3, GTYPE[t])
    wq = quantized_weights(t, rng, M, K)
    x = rng.standard_normal((N, K)).astype(np.float32)
    y = gpu_mul_mat(t, wq, K, x, algo=GEMM)
    assert np.any(y != 0)
    assert_bitwise(gpu_mul_mat(t, wq, K, 2 * x, algo=GEMM), 2 * y)


@BOTH
@pytest.mark.parametrize("K", [64, 192])
def test_gemm_weight_base_offset_in_allocation(exact_off, t, K):
    """W at 4, 8 and 12 bytes inside a larger allocation: nothing relies on more than 4-byte alignment"""
    M, N = 37, 9
    rng = rng_for(4, GTYPE[t], K)
    wq = R.random_blocks(rng, M, K, R.has_qh(t), True)
    x = activations(rng, N, K)
    base = gpu_mul_mat(t, wq, K, x, algo=GEMM)
    assert_bitwise(base, G.chain(t, wq, R.quantize_x(t, x), K))
    for off in (4, 8, 12):
        assert_bitwise(gpu_mul_mat(t, wq, K, x, algo=GEMM, w_off=off), base)


# ---- 5. K past the GEMV's LDS, 6. status codes ---------------------------------------------------------------

@BOTH
def test_gemm_k_past_the_gemv_lds(exact_off, t):
    """K = 52480 (1640 blocks): the GEMM has no K limit; auto still takes the exact kernel there."""
    K, M, N = 52480, 3, 9
    wq, x, ref = case(t, K, M, N)
    gemm_checked(t, wq, K, x, ref)
    assert getattr(exact_off, f"ggml_hip_debug_{NAME[t]}_auto_algo")(K, M, N) == EXACT


def test_gemm_status_codes(exact_off):
    L = exact_off
    b = DB(1 << 16)
    for t in TYPES:
        mm = getattr(L, "ggml_hip_mul_mat_" + NAME[t])
        assert mm(b.ptr, 64, 4, b.ptr, 1, b.ptr, 4, GEMM, None) == ggml_hip.OK             # N = 1
        assert mm(b.ptr, 64, 4, b.ptr, 1, b.ptr, 4, 8, None) == ggml_hip.ERR_INVALID
        assert mm(b.ptr, 64, 4, b.ptr, 0, b.ptr, 4, GEMM, None) == ggml_hip.OK             # N = 0
        assert mm(b.ptr, 96, 4, b.ptr, 1, b.ptr, 4, GEMM, None) == ggml_hip.ERR_INVALID    # K % 64
        assert mm(b.ptr, 64, 4, b.ptr, 1, b.ptr, 3, GEMM, None) == ggml_hip.ERR_INVALID    # ldy < M
        assert mm(b.ptr + 2, 64, 4, b.ptr, 1, b.ptr, 4, GEMM, None) == ggml_hip.ERR_INVALID
    mm = L.ggml_hip_mul_mat_q5_0
    assert mm(b.ptr, 64, 4, b.ptr, 1, b.ptr, 4, GEMM, None) == ggml_hip.ERR_INVALID
    assert mm(b.ptr, 64, 4, b.ptr, 1, b.ptr, 4, 8, None) == ggml_hip.ERR_INVALID
    assert mm(b.ptr, 64, 4, b.ptr, 0, b.ptr, 4, GEMM, None) == ggml_hip.OK
    ggml_hip.synchronize()


# ---- 7. threshold and auto, 8. graph capture -------------------------------------------------------------------

@BOTH
def test_auto_switches_at_the_threshold(exact_off, min_n, t):
    L = exact_off
    K, M = 256, 70
    rng = rng_for(5, GTYPE[t])
    wq = quantized_weights(t, rng, M, K)
    x = rng.standard_normal((40, K)).astype(np.float32)
    auto = getattr(L, f"ggml_hip_debug_{NAME[t]}_auto_algo")
    try:
        min_n(12)
        assert auto(K, M, 11) == GEMV and auto(K, M, 12) == GEMM
        assert_bitwise(gpu_mul_mat(t, wq, K, x[:11], algo=0), gpu_mul_mat(t, wq, K, x[:11], algo=GEMV))
        assert_bitwise(gpu_mul_mat(t, wq, K, x[:12], algo=0), gpu_mul_mat(t, wq, K, x[:12], algo=GEMM))
        min_n(-1)
        assert auto(K, M, 40) == GEMV
        assert_bitwise(gpu_mul_mat(t, wq, K, x, algo=0), gpu_mul_mat(t, wq, K, x, algo=GEMV))
    finally:
        min_n(-1)


@BOTH
def test_gemm_graph_capture_after_reserve(exact_off, t):
    L = exact_off
    K, M, N = 2304, 70, 20
    rng = rng_for(6, GTYPE[t])
    wq = quantized_weights(t, rng, M, K)
    x = rng.standard_normal((N, K)).astype(np.float32)
    eager = gpu_mul_mat(t, wq, K, x, algo=GEMM)          # (the tile's attributes are set outside the capture)
    ggml_hip.check(L.ggml_hip_reserve_workspace_mm(K, N, M), "reserve")
    wd, xd, yd = DB.from_array(wq), DB.from_array(x), DB(N * M * 4)
    s = L.ggml_hip_default_stream()
    g = ggml_hip.Graph(s)
    with g:
        getattr(ggml_hip, "mul_mat_" + NAME[t])(wd, K, M, xd, N, yd, algo=GEMM, stream=s)
    for _ in range(2):
        ggml_hip.check(L.ggml_hip_memset(yd.ptr, 0xFF, N * M * 4, s))
        g.launch()
        ggml_hip.check(L.ggml_hip_stream_synchronize(s))
        assert_bitwise(yd.download((N, M), np.float32), eager)


# ---- 9. hook path ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("backend", [ggml_hip.GGML_BACKEND_GPU, ggml_hip.GGML_BACKEND_GPU_SPLIT])
@BOTH
def test_hook_takes_the_gemm_from_the_threshold(exact_off, min_n, t, backend):
    """A layer matrix's operand placement (weight uploaded by transform_tensor, host x, host dst).  The hook calls
    the type's mul_mat with algo 0: with the threshold at 9 it runs the GEMM, with the default the GEMV."""
    L = exact_off
    K, M, N = 2304, 101, 33
    rng = rng_for(7, GTYPE[t])
    wq = quantized_weights(t, rng, M, K)
    x = rng.standard_normal((N, K)).astype(np.float32)
    ref = G.chain(t, wq, R.quantize_x(t, x), K)
    y_gemv = gpu_mul_mat(t, wq, K, x, algo=GEMV)
    assert np.any(y_gemv.view(np.uint32) != ref.view(np.uint32))      # else the next assertions would show nothing
    staged = wq.copy()
    w = w_tensor(t, staged, K, M, backend)
    L.ggml_hip_transform_tensor(staged.ctypes.data_as(ctypes.c_void_p), ctypes.byref(w))
    assert w.extra and w.backend == backend
    staged[:] = 0                                              # the loader frees its buffer
    y_np = np.zeros((N, M), np.float32)
    y, _ = mm_node(w, x, y_np)
    try:
        min_n(9)
        before = mul_mat_count(L)
        assert forward(L, y)
        assert mul_mat_count(L) == before + 1
        assert_bitwise(y_np, ref)
        min_n(-1)
        y_np[:] = 0
        assert forward(L, y)
        assert_bitwise(y_np, y_gemv)
    finally:
        min_n(-1)
        L.ggml_hip_free_data(ctypes.byref(w))
    assert not w.extra


# ---- 10. end to end -------------------------------------------------------------------------------------------

@pytest.mark.skipif(not os.path.exists(HIP_LIB), reason="oracle/_ref/libllama_ref_hip.so not built")
@BOTH
def test_llama_full_offload_gemm_prefill(tmp_path, min_n, t):
    """The tiny "mostly Q4_1" / "mostly Q5_1" LLaMAs through the reference's own llama.cpp, fully offloaded, fast
    kernels, threshold 9: the 40-token prompt's layer matrices run the GEMM, the decode steps the GEMV."""
    from test_gpu_llama_q5x import assert_layer_mul_mats_on_device, run_llama
    try:
        min_n(9)
        got, dec, ran, (gold, dgold) = run_llama(tmp_path, t, exact=False)
    finally:
        min_n(-1)
    assert np.isfinite(got).all() and np.isfinite(dec).all()
    assert_layer_mul_mats_on_device(ran)
    scale = np.abs(gold).max()
    assert np.abs(got - gold).max() / scale < 2e-2 and np.abs(dec - dgold).max() / scale < 2e-2
