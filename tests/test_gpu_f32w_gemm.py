"""The F32-weight prefill GEMM on the device (csrc/f32_w_gemm.hip, algo 12 of ggml_hip_mul_mat_f32, on
v_mfma_f32_32x32x2_f32): with the K split S pinned it is bit for bit tests/f32w_ref.py gemm_schedule(w, x, S), one
fmaf chain per slice in natural order and the slices added in order, for S = 1, 2 and 4 on one chunk, ragged rows and
columns over more than one tile each way and a K whose quarter is no whole number of chunks; auto S on the device is the
one ggml_hip_debug_f32w_gemm_ksplit names; a column and a row slice of a pinned call are the calls on the slices; the
derived bound and the row pitch; graph capture after a reservation; the ggml hook path at N = 40."""
import ctypes

import numpy as np
import pytest

import f32w_ref as R
import ggml_ops_ref as G
import hook_nodes as H
from hip_env import ggml_hip, gpu_available
from test_gpu_f32w import assert_bitwise, assert_within_bound, exact_off, gpu_mul_mat        # noqa: F401

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason="needs a HIP device and libggml_hip.so")]

DB = ggml_hip.DeviceBuffer
GEMV, EXACT, GEMM = 1, 4, 12
NG = len(R.GEMV_CASES)
GEMM_IDX = list(range(NG, len(R.CASES)))
IDS = ["K%d_M%d_N%d%s%s" % (c[0], c[1], c[2], "_ldy" if c[3] else "", "_special" if c[4] else "") for c in R.CASES]
FILL = np.float32(-7.5)


@pytest.fixture
def switches(exact_off):
    """exact mode off; the threshold and the split pin as found are put back afterwards, also when the test fails"""
    L = exact_off
    prev_n, prev_s = L.ggml_hip_debug_set_f32w_gemm_min_n(-1), L.ggml_hip_debug_set_f32w_gemm_ksplit(0)
    L.ggml_hip_debug_set_f32w_gemm_min_n(prev_n)
    yield L
    L.ggml_hip_debug_set_f32w_gemm_min_n(prev_n)
    L.ggml_hip_debug_set_f32w_gemm_ksplit(prev_s)


@pytest.mark.parametrize("S", [1, 2, 4])
@pytest.mark.parametrize("i", GEMM_IDX, ids=[IDS[i] for i in GEMM_IDX])
def test_gemm_bitwise_the_restatement(switches, i, S):
    """(a request of S for which K / S is no multiple of 32 runs as the next smaller split: gemm_schedule restates
    that too, as the header says)"""
    K, M, N, pad, special = R.CASES[i]
    w, x = R.case(i)
    assert switches.ggml_hip_debug_set_f32w_gemm_ksplit(S) == 0
    y = gpu_mul_mat(w, x, GEMM, ldy=M + pad + 5, fill=FILL)
    assert (y[:, M:] == FILL).all()                          # the pitch columns are untouched
    assert_bitwise(y[:, :M], R.ref(i, "gemm", R.gemm_ksplit(K, S)))
    assert_within_bound(y[:, :M], w, x)
    if special:
        assert (y[:, 0] == np.float32(2.0 ** -110)).all()    # survives only if subnormal operands are kept


def test_auto_split_is_the_named_one(switches):
    """on the device auto runs the split ggml_hip_debug_f32w_gemm_ksplit names; the shapes cover 1, 2 and 4"""
    L = switches
    seen = set()
    for i in (NG + 2, NG + 3, NG + 4):                       # (1024, 200, 130), (4544, 73, 33), (2048, 96, 48)
        K, M, N = R.CASES[i][:3]
        w, x = R.case(i)
        S = L.ggml_hip_debug_f32w_gemm_ksplit(K, M, N)
        assert S in (1, 2, 4)
        seen.add(S)
        assert_bitwise(gpu_mul_mat(w, x, GEMM), R.ref(i, "gemm", S))
    K, M, N = R.CASES[NG][:3]                                # one chunk: never split
    assert L.ggml_hip_debug_f32w_gemm_ksplit(K, M, N) == 1
    assert_bitwise(gpu_mul_mat(*R.case(NG), GEMM), R.ref(NG, "gemm", 1))
    assert len(seen) >= 2
    # the three orders differ on these inputs: the assertions above would show nothing otherwise
    i = NG + 4
    assert (G.bits(R.ref(i, "gemm", 1)) != G.bits(R.ref(i, "gemm", 2))).any()
    assert (G.bits(R.ref(i, "gemm", 2)) != G.bits(R.ref(i, "gemm", 4))).any()


@pytest.mark.parametrize("S", [1, 4])
def test_slices_are_the_calls_on_the_slices(switches, S):
    i = NG + 2                                               # K = 1024, M = 200, N = 130: tiles of 128 x 64
    w, x = R.case(i)
    switches.ggml_hip_debug_set_f32w_gemm_ksplit(S)
    y = gpu_mul_mat(w, x, GEMM)
    assert_bitwise(y, R.ref(i, "gemm", S))
    assert_bitwise(gpu_mul_mat(w, x, GEMM), y)               # the same bits twice
    for cols in (slice(9, 41), slice(129, 130), slice(0, 70)):     # other token tiles: 32, 32, 128 x 64 over two
        assert_bitwise(y[cols], gpu_mul_mat(w, np.ascontiguousarray(x[cols]), GEMM))
    assert_bitwise(y[:, 120:135], gpu_mul_mat(np.ascontiguousarray(w[120:135]), x, GEMM))


@pytest.mark.parametrize("S", [2, 4])
def test_graph_capture_after_reserve(switches, S):
    """a split call's slabs are rewritten by every replay, nothing carries over"""
    L = switches
    i = NG + 4                                               # K = 2048, M = 96, N = 48
    K, M, N = R.CASES[i][:3]
    w, x = R.case(i)
    L.ggml_hip_debug_set_f32w_gemm_ksplit(S)
    eager = gpu_mul_mat(w, x, GEMM)                          # (the kernels' attributes are set outside the capture)
    assert_bitwise(eager, R.ref(i, "gemm", S))
    ggml_hip.check(L.ggml_hip_reserve_workspace_mm(K, N, M), "reserve")
    wd, xd, yd = DB.from_array(w), DB.from_array(x), DB(N * M * 4)
    s = L.ggml_hip_default_stream()
    g = ggml_hip.Graph(s)
    with g:
        ggml_hip.mul_mat_f32(wd, K, M, xd, N, yd, algo=GEMM, stream=s)
    for _ in range(2):
        ggml_hip.check(L.ggml_hip_memset(yd.ptr, 0xFF, N * M * 4, s))
        g.launch()
        ggml_hip.check(L.ggml_hip_stream_synchronize(s))
        assert_bitwise(yd.download((N, M), np.float32), eager)
    for b in (wd, xd, yd):
        b.free()


@pytest.mark.parametrize("backend", [ggml_hip.GGML_BACKEND_GPU, ggml_hip.GGML_BACKEND_GPU_SPLIT])
def test_hook_runs_the_gemm_at_40_tokens(switches, backend):
    """A layer matrix's operand placement (weight uploaded by transform_tensor, host x, host dst) at N = 40, above the
    threshold: the hook calls the F32 row with algo 0, which runs algo 12 at the split auto names."""
    from test_gpu_f32w_hook import f32_tensor, forward, mm_node
    L = switches
    L.ggml_hip_debug_set_f32w_gemm_min_n(32)
    i = NG                                                   # K = 32, M = 130, N = 40
    w0, x = R.case(i)
    K, M, N = R.CASES[i][:3]
    assert L.ggml_hip_debug_f32w_auto_algo(K, M, N) == GEMM
    staged = w0.copy()
    w = f32_tensor(staged, backend)
    L.ggml_hip_transform_tensor(staged.ctypes.data_as(ctypes.c_void_p), ctypes.byref(w))
    assert w.extra and w.backend == backend
    staged[:] = 0                                            # the loader frees its buffer
    y_np = np.zeros((N, M), np.float32)
    y, _xt = mm_node(w, x, y_np)
    try:
        before = H.op_stats(L, reset=False)[0][H.OP_MUL_MAT]
        assert forward(L, y)
        assert H.op_stats(L, reset=False)[0][H.OP_MUL_MAT] == before + 1
        assert_bitwise(y_np, R.ref(i, "gemm", L.ggml_hip_debug_f32w_gemm_ksplit(K, M, N)))
        assert (G.bits(y_np) != G.bits(R.ref(i, "gemv"))).any()          # not the GEMV's order
    finally:
        L.ggml_hip_free_data(ctypes.byref(w))
    assert not w.extra
