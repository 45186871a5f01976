"""F32 weights on the ggml hook path (hand-built nodes: ggml_hip.make_tensor, ggml_hip_transform_tensor,
ggml_hip_can_mul_mat, ggml_hip_compute_forward).  A 2-D contiguous F32 leaf with K % 32 == 0 is a weight: uploaded
row-split like every other weight type, its mul_mat one launch of the F32 row (the GEMV's order at decode, bit for bit
tests/f32w_ref.py; ggml_vec_dot_f32's in exact mode).  A host matrix between host operands is ggml's unless the switch
(GGML_HIP_F32_W / ggml_hip_debug_set_f32_w) is on; between device operands it is served from the residency cache."""
import ctypes

import numpy as np
import pytest

import f32w_ref as R
import ggml_ops_ref as G
import hook_nodes as H
from hip_env import ggml_hip, gpu_available

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason="needs a HIP device and libggml_hip.so")]

F32 = ggml_hip.GGML_TYPE_F32


def assert_bitwise(got, ref):
    diff = np.flatnonzero(G.bits(got).ravel() != G.bits(ref).ravel())
    assert diff.size == 0, f"{diff.size} of {got.size} differ; first at {diff[:4]}: {np.ravel(got)[diff[:4]]} vs " \
                           f"{np.ravel(ref)[diff[:4]]}"


def f32_tensor(w, backend=ggml_hip.GGML_BACKEND_CPU):
    M, K = w.shape
    return ggml_hip.make_tensor(F32, (K, M), w, backend=backend)


def mm_node(w, x_np, y_np):
    N, K = x_np.shape
    xt = ggml_hip.make_tensor(F32, (K, N), x_np)
    y = ggml_hip.make_tensor(F32, (y_np.shape[1], N), y_np)
    y.op = ggml_hip.GGML_OP_MUL_MAT
    y.src0 = ctypes.pointer(w)
    y.src1 = ctypes.pointer(xt)
    return y, xt


def forward(L, node):
    p = ggml_hip.GgmlComputeParams(ggml_hip.GGML_TASK_COMPUTE, 0, 1, 0, None)
    return L.ggml_hip_compute_forward(ctypes.byref(p), ctypes.byref(node))


def can(L, w, xt, y):
    return bool(L.ggml_hip_can_mul_mat(ctypes.byref(w), ctypes.byref(xt), ctypes.byref(y)))


def cache_stats(L):
    h, m, r = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    ggml_hip.check(L.ggml_hip_weight_cache_stats(ctypes.byref(h), ctypes.byref(m), ctypes.byref(r)))
    return h.value, m.value


@pytest.fixture
def lib():
    """exact mode off, the F32 switch off; both as found afterwards"""
    L = ggml_hip.load()
    L.ggml_hip_debug_set_decode_min_weights.restype = ctypes.c_int64
    L.ggml_hip_debug_set_decode_min_weights.argtypes = [ctypes.c_int64]
    with H.restore_switches(L):
        L.ggml_hip_set_exact(0)
        prev = L.ggml_hip_debug_set_f32_w(0)
        try:
            yield L
        finally:
            L.ggml_hip_debug_set_f32_w(prev)


@pytest.mark.parametrize("backend", [ggml_hip.GGML_BACKEND_GPU_SPLIT, ggml_hip.GGML_BACKEND_GPU])
@pytest.mark.parametrize("N", [1, 8])
def test_uploaded_matrix(lib, backend, N):
    """transform_tensor keeps GPU_SPLIT for an F32 matrix; its node at N = 1 and 8 is the GEMV's order bit for bit, and
    ggml_vec_dot_f32's in exact mode; one MUL_MAT per node; free_data clears extra"""
    L = lib
    i = 4                                                    # K = 11008, M = 65, N = 8
    w0, x = R.case(i)
    x, ref, exact = x[:N], R.ref(i, "gemv")[:N], R.ref(i, "exact")[:N]
    assert (G.bits(ref) != G.bits(exact)).any()
    K, M = w0.shape[1], w0.shape[0]
    staged = w0.copy()
    w = f32_tensor(staged, backend)
    L.ggml_hip_transform_tensor(staged.ctypes.data_as(ctypes.c_void_p), ctypes.byref(w))
    assert w.extra and w.backend == backend
    staged[:] = 0                                            # the loader frees its buffer
    y_np = np.zeros((N, M), np.float32)
    y, xt = mm_node(w, x, y_np)
    before = H.op_stats(L, reset=False)[0][H.OP_MUL_MAT]
    assert forward(L, y)
    assert H.op_stats(L, reset=False)[0][H.OP_MUL_MAT] == before + 1
    assert_bitwise(y_np, ref)
    L.ggml_hip_set_exact(1)
    y_np[:] = 0
    assert forward(L, y)
    assert_bitwise(y_np, exact)
    L.ggml_hip_free_data(ctypes.byref(w))
    assert not w.extra


def test_non_weights_are_not_row_split(lib):
    """a 3-D F32 tensor, an F32 matrix with K = 48 and a 1-D norm weight are no weights: GPU_SPLIT is demoted to GPU as
    before, a GPU tensor stays GPU; a mul_mat on the K = 48 matrix is nobody's here (ggml's CPU op asserts host
    operands: the reference's loader never uploads such a matrix)"""
    L = lib
    rng = np.random.default_rng([0xF32, 201])
    for shape in ((2, 5, 64), (5, 48)):
        a = rng.standard_normal(shape).astype(np.float32)
        t = H._tensor(F32, shape[::-1])
        t.backend, t.data = ggml_hip.GGML_BACKEND_GPU_SPLIT, a.ctypes.data
        L.ggml_hip_transform_tensor(a.ctypes.data_as(ctypes.c_void_p), ctypes.byref(t))
        assert t.backend == ggml_hip.GGML_BACKEND_GPU and t.extra
        if len(shape) == 2:
            x = rng.standard_normal((3, 48)).astype(np.float32)
            y, xt = mm_node(t, x, np.zeros((3, 5), np.float32))
            assert not can(L, t, xt, y) and not forward(L, y)
        L.ggml_hip_free_data(ctypes.byref(t))
        assert not t.extra
    a = rng.standard_normal((64,)).astype(np.float32)
    t = H._tensor(F32, (64,))
    t.backend, t.data = ggml_hip.GGML_BACKEND_GPU, a.ctypes.data
    L.ggml_hip_transform_tensor(a.ctypes.data_as(ctypes.c_void_p), ctypes.byref(t))
    assert t.backend == ggml_hip.GGML_BACKEND_GPU and t.extra
    L.ggml_hip_free_data(ctypes.byref(t))


def test_host_matrix_switch_off(lib):
    """all-host: declined (ggml's CPU op runs it).  The same matrix with a device src1 cannot run on the CPU any more:
    it is served from the residency cache, one miss and then hits."""
    L = lib
    rng = np.random.default_rng([0xF32, 202])
    K, M, N = 288, 130, 40
    w0, x = R.random_case(rng, M, K, N)
    w = f32_tensor(w0)
    y_np = np.zeros((N, M), np.float32)
    y, xt = mm_node(w, x, y_np)
    prev = L.ggml_hip_debug_set_decode_min_weights(0)
    try:
        assert not can(L, w, xt, y) and not forward(L, y)
        y1, xt1 = mm_node(w, x[:1].copy(), np.zeros((1, M), np.float32))
        assert not can(L, w, xt1, y1) and not forward(L, y1)
        # x on the device (an offloaded layer's activation)
        staged = x.copy()
        xd = ggml_hip.make_tensor(F32, (K, N), staged, backend=ggml_hip.GGML_BACKEND_GPU)
        L.ggml_hip_transform_tensor(staged.ctypes.data_as(ctypes.c_void_p), ctypes.byref(xd))
        assert xd.extra and xd.backend == ggml_hip.GGML_BACKEND_GPU
        y.src1 = ctypes.pointer(xd)
        L.ggml_hip_weight_cache_invalidate(w0.ctypes.data_as(ctypes.c_void_p), w0.nbytes)
        hits0, miss0 = cache_stats(L)
        assert forward(L, y)
        assert cache_stats(L) == (hits0, miss0 + 1)          # one upload ...
        first = y_np.copy()
        y_np[:] = 0
        assert forward(L, y)
        assert cache_stats(L) == (hits0 + 1, miss0 + 1)      # ... for two calls
        assert_bitwise(y_np, first)
        s64, sab = R.exact_terms(w0, x)
        assert (np.abs(y_np.astype(np.float64) - s64) <= R.bound(K, sab)).all()
        L.ggml_hip_set_exact(1)
        y_np[:] = 0
        assert forward(L, y)
        assert_bitwise(y_np, R.mul_mat_f32(w0, x))
        L.ggml_hip_free_data(ctypes.byref(xd))
    finally:
        L.ggml_hip_debug_set_decode_min_weights(prev)
        L.ggml_hip_weight_cache_invalidate(w0.ctypes.data_as(ctypes.c_void_p), w0.nbytes)


def test_host_matrix_switch_on(lib):
    """switch on, a host F32 weight follows the other types' rule: taken at N = 40 (ne0, ne1, ne10 >= 32), and at N = 1
    from GGML_HIP_DECODE_MIN_WEIGHTS elements through the residency cache, not below"""
    L = lib
    rng = np.random.default_rng([0xF32, 203])
    K, M = 288, 130                                          # 37,440 elements
    w0, x40 = R.random_case(rng, M, K, 40)
    w = f32_tensor(w0)
    y40_np = np.zeros((40, M), np.float32)
    y40, xt40 = mm_node(w, x40, y40_np)
    x1 = x40[:1].copy()
    y1_np = np.zeros((1, M), np.float32)
    y1, xt1 = mm_node(w, x1, y1_np)
    prev = L.ggml_hip_debug_set_decode_min_weights(M * K + 1)
    try:
        assert not can(L, w, xt40, y40)
        assert L.ggml_hip_debug_set_f32_w(1) == 0
        assert can(L, w, xt40, y40)
        assert not can(L, w, xt1, y1) and not forward(L, y1)  # below the threshold: ggml's CPU op
        L.ggml_hip_debug_set_decode_min_weights(M * K)
        assert can(L, w, xt1, y1)
        L.ggml_hip_weight_cache_invalidate(w0.ctypes.data_as(ctypes.c_void_p), w0.nbytes)
        hits0, miss0 = cache_stats(L)
        assert forward(L, y1)
        assert cache_stats(L) == (hits0, miss0 + 1)
        assert_bitwise(y1_np, R.gemv_schedule(w0, x1))
        assert forward(L, y40)                               # N = 40, from the same cached copy
        assert cache_stats(L) == (hits0 + 1, miss0 + 1)
        s64, sab = R.exact_terms(w0, x40)
        assert (np.abs(y40_np.astype(np.float64) - s64) <= R.bound(K, sab)).all()
        # a matrix with K = 48, a 3-D src0 and a view stay declined, switch on
        wk = f32_tensor(np.zeros((64, 48), np.float32))
        y, xt = mm_node(wk, np.zeros((64, 48), np.float32), np.zeros((64, 64), np.float32))
        assert not can(L, wk, xt, y) and not forward(L, y)
        wv = f32_tensor(np.zeros((64, 128), np.float32))
        wv.op = H._OPS["VIEW"]
        y, xt = mm_node(wv, np.zeros((64, 128), np.float32), np.zeros((64, 64), np.float32))
        assert not can(L, wv, xt, y) and not forward(L, y)
        assert L.ggml_hip_debug_set_f32_w(0) == 1
        assert not can(L, w, xt40, y40)
    finally:
        L.ggml_hip_debug_set_f32_w(0)
        L.ggml_hip_debug_set_decode_min_weights(prev)
        L.ggml_hip_weight_cache_invalidate(w0.ctypes.data_as(ctypes.c_void_p), w0.nbytes)
