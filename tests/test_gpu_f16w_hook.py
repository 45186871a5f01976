"""F16 weights on the ggml hook path (hand-built nodes: ggml_hip.make_tensor, ggml_hip_transform_tensor,
ggml_hip_can_mul_mat, ggml_hip_compute_forward).  A 2-D contiguous F16 leaf with K % 32 == 0 is a weight: uploaded
row-split like every other weight type, its mul_mat one launch of the F16 row (the GEMV's order at decode, bit for bit
tests/f16w_ref.py; ggml_vec_dot_f16's in exact mode), and host-resident weights are taken through the residency cache.
Every other F16 src0 keeps the attention's F16 x F32 device op, and what was declined stays declined."""
import ctypes

import numpy as np
import pytest

import f16w_ref as R
import ggml_ops_ref as G
import hook_nodes as H
from hip_env import ggml_hip, gpu_available

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason="needs a HIP device and libggml_hip.so")]

F16 = ggml_hip.GGML_TYPE_F16


def assert_bitwise(got, ref):
    diff = np.flatnonzero(G.bits(got).ravel() != G.bits(ref).ravel())
    assert diff.size == 0, f"{diff.size} of {got.size} differ; first at {diff[:4]}: {np.ravel(got)[diff[:4]]} vs " \
                           f"{np.ravel(ref)[diff[:4]]}"


def f16_tensor(w16, backend=ggml_hip.GGML_BACKEND_CPU):
    M, K = w16.shape
    return ggml_hip.make_tensor(F16, (K, M), w16, backend=backend)


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


def can(L, w, xt, y):
    return bool(L.ggml_hip_can_mul_mat(ctypes.byref(w), ctypes.byref(xt), ctypes.byref(y)))


def cache_stats(L):
    h, m, r = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    ggml_hip.check(L.ggml_hip_weight_cache_stats(ctypes.byref(h), ctypes.byref(m), ctypes.byref(r)))
    return h.value, m.value


@pytest.fixture
def lib():
    L = ggml_hip.load()
    L.ggml_hip_debug_set_decode_min_weights.restype = ctypes.c_int64
    L.ggml_hip_debug_set_decode_min_weights.argtypes = [ctypes.c_int64]
    with H.restore_switches(L):
        L.ggml_hip_set_exact(0)
        yield L


@pytest.mark.parametrize("backend", [ggml_hip.GGML_BACKEND_GPU_SPLIT, ggml_hip.GGML_BACKEND_GPU])
@pytest.mark.parametrize("N", [1, 8])
def test_uploaded_matrix(lib, backend, N):
    """transform_tensor keeps GPU_SPLIT for an F16 matrix; its node at N = 1 and 8 is the GEMV's order bit for bit (the
    attention kernel this node ran on before gives ggml_vec_dot_f16's bits, which differ: tests/test_f16w_ref.py), and
    ggml_vec_dot_f16's in exact mode; one MUL_MAT per node"""
    L = lib
    i = 10                                                   # K = 11008, M = 65, N = 8
    w16, x, ref = R.case(i)
    x, ref = x[:N], ref[:N]
    K, M = w16.shape[1], w16.shape[0]
    staged = w16.copy()
    w = f16_tensor(staged, backend)
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
    assert_bitwise(y_np, G.mul_mat_f16_f32(w16, x))
    L.ggml_hip_free_data(ctypes.byref(w))
    assert not w.extra


def test_non_matrix_f16_tensors_are_not_row_split(lib):
    """a 3-D F16 tensor and an F16 matrix with K % 32 != 0 are no weights: GPU_SPLIT is demoted to GPU as before, and
    their mul_mats stay on the F16 x F32 device op (ggml_vec_dot_f16's bits outside exact mode too)"""
    L = lib
    rng = np.random.default_rng([0xF16, 201])
    for shape in ((2, 5, 64), (5, 48)):
        a = (rng.standard_normal(shape) * 0.5).astype(np.float16).view(np.uint16)
        t = H._tensor(F16, shape[::-1])
        t.backend, t.data = ggml_hip.GGML_BACKEND_GPU_SPLIT, a.ctypes.data
        L.ggml_hip_transform_tensor(a.ctypes.data_as(ctypes.c_void_p), ctypes.byref(t))
        assert t.backend == ggml_hip.GGML_BACKEND_GPU and t.extra
        if len(shape) == 2:
            x = rng.standard_normal((3, 48)).astype(np.float32)
            y_np = np.zeros((3, 5), np.float32)
            y, xt = mm_node(t, x, y_np)
            assert not can(L, t, xt, y)
            assert forward(L, y)
            assert_bitwise(y_np, G.mul_mat_f16_f32(a, x))
        L.ggml_hip_free_data(ctypes.byref(t))


def test_host_resident_weights(lib):
    L = lib
    rng = np.random.default_rng([0xF16, 202])
    K, M = 544, 130                                          # 70,720 elements
    w16, x40 = R.random_case(rng, M, K, 40)
    w = f16_tensor(w16)
    # prefill: ne0, ne1, ne10 >= 32, as in the reference
    y40_np = np.zeros((40, M), np.float32)
    y40, xt40 = mm_node(w, x40, y40_np)
    assert can(L, w, xt40, y40)
    # decode: through the residency cache, for weights of at least GGML_HIP_DECODE_MIN_WEIGHTS elements
    x1 = x40[:1].copy()
    y1_np = np.zeros((1, M), np.float32)
    y1, xt1 = mm_node(w, x1, y1_np)
    prev = L.ggml_hip_debug_set_decode_min_weights(M * K + 1)
    try:
        assert not can(L, w, xt1, y1)                        # below the threshold: ggml's CPU op
        assert not forward(L, y1)
        L.ggml_hip_debug_set_decode_min_weights(M * K)
        assert can(L, w, xt1, y1)
        L.ggml_hip_weight_cache_invalidate(w16.ctypes.data_as(ctypes.c_void_p), w16.nbytes)
        hits0, miss0 = cache_stats(L)
        assert forward(L, y1)
        assert cache_stats(L) == (hits0, miss0 + 1)          # one upload ...
        first = y1_np.copy()
        y1_np[:] = 0
        assert forward(L, y1)
        assert cache_stats(L) == (hits0 + 1, miss0 + 1)      # ... for two calls
        assert_bitwise(y1_np, first)
        assert_bitwise(y1_np, R.gemv_schedule(w16, x1))
        assert forward(L, y40)                               # N = 40: the MFMA kernel, from the same cached copy
        assert cache_stats(L) == (hits0 + 2, miss0 + 1)
        ref, sab = R.exact_terms(w16, x40)
        assert (np.abs(y40_np.astype(np.float64) - ref) <= 1e-5 * sab + 1e-30).all()
        L.ggml_hip_set_exact(1)
        y1_np[:] = 0
        assert forward(L, y1)
        assert_bitwise(y1_np, G.mul_mat_f16_f32(w16, x1))
    finally:
        L.ggml_hip_debug_set_decode_min_weights(prev)
        L.ggml_hip_weight_cache_invalidate(w16.ctypes.data_as(ctypes.c_void_p), w16.nbytes)


def test_declines_stay_declines(lib):
    L = lib
    N, M = 64, 64
    prev = L.ggml_hip_debug_set_decode_min_weights(0)
    try:
        # K = 48
        K = 48
        w = f16_tensor(np.zeros((M, K), np.uint16))
        y, xt = mm_node(w, np.zeros((N, K), np.float32), np.zeros((N, M), np.float32))
        assert not can(L, w, xt, y) and not forward(L, y)
        # non-contiguous src1
        K = 128
        w = f16_tensor(np.zeros((M, K), np.uint16))
        y, xt = mm_node(w, np.zeros((N, 2 * K), np.float32), np.zeros((N, M), np.float32))
        xt.ne[0] = K
        xt.nb[2] = xt.nb[3] = xt.nb[1] * N
        assert not can(L, w, xt, y) and not forward(L, y)
        xt.nb[1] = 4 * K
        xt.nb[2] = xt.nb[3] = xt.nb[1] * N
        assert can(L, w, xt, y)
        # a 3-D F16 src0 on the host (the attention's K of a CPU graph)
        a = np.zeros((2, M, K), np.uint16)
        w3 = H._tensor(F16, (K, M, 2))
        w3.data = a.ctypes.data
        x3 = np.zeros((2, N, K), np.float32)
        xt3 = H._tensor(H.TYPE_F32, (K, N, 2))
        xt3.data = x3.ctypes.data
        y3_np = np.zeros((2, N, M), np.float32)
        y3 = H._tensor(H.TYPE_F32, (M, N, 2))
        y3.data, y3.op = y3_np.ctypes.data, ggml_hip.GGML_OP_MUL_MAT
        y3.src0, y3.src1 = ctypes.pointer(w3), ctypes.pointer(xt3)
        assert not can(L, w3, xt3, y3) and not forward(L, y3)
        # a 2-D F16 src0 that is no leaf (a view of the cache) on the host
        wv = f16_tensor(np.zeros((M, K), np.uint16))
        wv.op = H._OPS["VIEW"]
        y, xt = mm_node(wv, np.zeros((N, K), np.float32), np.zeros((N, M), np.float32))
        assert not can(L, wv, xt, y) and not forward(L, y)
    finally:
        L.ggml_hip_debug_set_decode_min_weights(prev)
