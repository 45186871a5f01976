"""The F16-weight prefill GEMM on the device (csrc/f16_w_gemm.hip, algo 11 of ggml_hip_mul_mat_f16): every y within
|y - S| <= 1e-5 * sum |W * fp16(x)| of the float64 sum S of the exact products (algo 9's bound, tests/test_gpu_f16w.py;
what it asks of the inputs: tests/test_f16w_gemm_inputs.py) on ragged chunks, rows and columns with a row pitch; every
plan of the launcher, named and pinned; the same bits twice, and with the plan pinned a column or row slice bitwise the
call on that slice; guard bytes; status codes; the threshold of its own; graph capture after a reservation; the ggml
hook path; and the reference's llama.cpp end to end under every launch mode."""
import ctypes
import os

import numpy as np
import pytest

import f16w_gemm_cases as C
import f16w_ref as R
import ggml_ops_ref as G
from conftest import ROOT
from hip_env import ggml_hip, gpu_available
from test_gpu_f16w import assert_bitwise, exact_off, gpu_mul_mat        # noqa: F401
from test_gpu_f16w_hook import cache_stats, f16_tensor, forward, lib, mm_node   # noqa: F401
import hook_nodes as H

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason="needs a HIP device and libggml_hip.so")]

DB = ggml_hip.DeviceBuffer
HIP_LIB = os.path.join(ROOT, "oracle", "_ref", "libllama_ref_hip.so")
GEMV, EXACT, MFMA, WGEMM = 1, 4, 9, 11
FILL = np.float32(-7.5)


@pytest.fixture
def switches(exact_off):
    """exact mode off; the threshold and the plan pin as found are put back afterwards, also when the test fails"""
    L = exact_off
    min_n, pin = L.ggml_hip_debug_set_f16w_wgemm_min_n, L.ggml_hip_debug_set_f16w_wgemm_plan
    prev_n, prev_p = min_n(-1), pin(0)
    min_n(prev_n)
    yield L
    min_n(prev_n)
    pin(prev_p)


def wgemm_checked(w16, x, ref, sab):
    """algo 11 into ldy = M + 5 over a fill value: the gap untouched, y not all zero, finite and within the bound"""
    M = w16.shape[0]
    y = gpu_mul_mat(np.ascontiguousarray(w16), np.ascontiguousarray(x), WGEMM, ldy=M + 5, fill=FILL)
    assert np.all(y[:, M:] == FILL)
    y = y[:, :M]
    assert np.any(y != 0) and np.isfinite(y).all()
    ok, share = C.within_bound(y, ref, sab)
    print("error / sum of magnitudes", share)
    assert ok, share
    return y


# ---- 1. within the bound ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("i", range(len(C.CASES)), ids=C.IDS)
def test_wgemm_within_bound(switches, i):
    w16, x, ref, sab = C.case(i)
    wgemm_checked(w16, x, ref, sab)
    if i == C.WIDE:
        wgemm_checked(w16, x[:1], ref[:1], sab[:1])          # N = 1


# ---- 2. every plan ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K,M,N,plan", C.PLAN_CASES, ids=["K%d_M%d_N%d_plan%d" % c for c in C.PLAN_CASES])
def test_every_plan_named_and_pinned(switches, K, M, N, plan):
    L = switches
    assert L.ggml_hip_debug_f16w_wgemm_plan(K, M, N) == plan
    w16, x = C.inputs(K, M, N)
    ref, sab = C.terms(K, M, N)
    auto = wgemm_checked(w16, x, ref, sab)
    assert L.ggml_hip_debug_set_f16w_wgemm_plan(plan) == 0
    assert_bitwise(wgemm_checked(w16, x, ref, sab), auto)    # auto took the plan it names
    if N == 300:
        # the two 300-column shapes, C.BIG's grid larger than the device: bitwise the calls on 64-column slices under
        # the same pinned plan
        for n0 in range(0, N, 64):
            assert_bitwise(auto[n0:n0 + 64], gpu_mul_mat(w16, np.ascontiguousarray(x[n0:n0 + 64]), WGEMM))


@pytest.mark.parametrize("plan", [1, 2, 3])
def test_every_plan_on_the_ragged_wide_case(switches, plan):
    """(4160, 70, 130) under each pinned plan, whatever auto takes: ragged chunk, ragged rows, ragged columns"""
    w16, x, ref, sab = C.case(C.WIDE)
    switches.ggml_hip_debug_set_f16w_wgemm_plan(plan)
    wgemm_checked(w16, x, ref, sab)


# ---- 3. determinism and independence ----------------------------------------------------------------------------

@pytest.mark.parametrize("plan", [1, 2, 3])
def test_same_bits_twice_and_slices_are_the_calls_on_the_slices(switches, plan):
    w16, x, ref, sab = C.case(C.WIDE)                        # K = 4160, M = 70, N = 130
    switches.ggml_hip_debug_set_f16w_wgemm_plan(plan)
    y = gpu_mul_mat(w16, x, WGEMM)
    assert C.within_bound(y, ref, sab)[0]
    assert_bitwise(gpu_mul_mat(w16, x, WGEMM), y)
    for cols in (slice(9, 41), slice(129, 130)):
        assert_bitwise(y[cols], gpu_mul_mat(w16, np.ascontiguousarray(x[cols]), WGEMM))
    assert_bitwise(y[:, 64:70], gpu_mul_mat(np.ascontiguousarray(w16[64:70]), x, WGEMM))


# ---- 4. guard bytes ---------------------------------------------------------------------------------------------

def test_guard_bytes(switches):
    """w, x and y inside one buffer each with 4 KiB of a fixed pattern on both sides (NaN halves around w, NaN floats
    around x): the patterns stay, y's pitch columns stay, and the poison does not reach y"""
    K, M, N = 1504, 65, 9
    w16, x = R.random_case(np.random.default_rng([0xF16, 99]), M, K, N)
    G4 = 4096
    ld = M + 3
    wb = np.full(G4 // 2 + M * K + G4 // 2, 0x7E00, np.uint16)          # fp16 NaN
    wb[G4 // 2:G4 // 2 + M * K] = w16.ravel()
    xb = np.full(G4 // 4 + N * K + G4 // 4, np.nan, np.float32)
    xb[G4 // 4:G4 // 4 + N * K] = x.ravel()
    yb = np.full(G4 // 4 + N * ld + G4 // 4, -7.25, np.float32)
    wd, xd, yd = DB.from_array(wb), DB.from_array(xb), DB.from_array(yb)
    ggml_hip.mul_mat_f16(wd, K, M, xd, N, yd, algo=WGEMM, ldy=ld, w_off=G4, x_off=G4, y_off=G4)
    assert np.array_equal(wd.download(wb.shape, np.uint16), wb)
    assert np.array_equal(G.bits(xd.download(xb.shape, np.float32)), G.bits(xb))
    got = yd.download(yb.shape, np.float32)
    assert (got[:G4 // 4] == -7.25).all() and (got[-G4 // 4:] == -7.25).all()
    y = got[G4 // 4:-G4 // 4].reshape(N, ld)
    assert (y[:, M:] == -7.25).all()
    assert np.isfinite(y[:, :M]).all()
    assert C.within_bound(y[:, :M], *R.exact_terms(w16, x))[0]
    for b in (wd, xd, yd):
        b.free()


# ---- 5. status codes --------------------------------------------------------------------------------------------

def test_status_codes(switches):
    L = switches
    K, M, N = 64, 4, 2
    wd, xd, yd = DB(M * K * 2 + 64), DB(N * K * 4), DB(N * (M + 1) * 4)
    call = lambda *a: L.ggml_hip_mul_mat_f16(*a)
    ok, inv = ggml_hip.OK, ggml_hip.ERR_INVALID
    assert call(wd.ptr, K, M, xd.ptr, N, yd.ptr, M, WGEMM, None) == ok
    assert call(wd.ptr, K, M, xd.ptr, N, yd.ptr, M + 1, WGEMM, None) == ok           # a row pitch
    assert call(wd.ptr, K, M, xd.ptr, 0, yd.ptr, M, WGEMM, None) == ok               # N == 0: nothing to do
    assert call(wd.ptr, 48, M, xd.ptr, N, yd.ptr, M, WGEMM, None) == inv             # K % 32
    assert call(wd.ptr + 2, K, M, xd.ptr, N, yd.ptr, M, WGEMM, None) == inv          # w off its 16-byte alignment
    assert call(wd.ptr, K, M, xd.ptr, N, yd.ptr, M - 1, WGEMM, None) == inv          # ldy < M
    assert call(None, K, M, xd.ptr, N, yd.ptr, M, WGEMM, None) == inv
    assert call(wd.ptr, K, M, None, N, yd.ptr, M, WGEMM, None) == inv
    assert call(wd.ptr, K, M, xd.ptr, N, yd.ptr, M, 10, None) == inv                 # still no algo
    assert call(wd.ptr, K, M, xd.ptr, 0, yd.ptr, M, 10, None) == inv
    ggml_hip.check(L.ggml_hip_device_synchronize(), "sync")
    for b in (wd, xd, yd):
        b.free()


# ---- 6. the threshold -------------------------------------------------------------------------------------------

def test_auto_switches_at_the_threshold(switches):
    L = switches
    min_n, auto = L.ggml_hip_debug_set_f16w_wgemm_min_n, L.ggml_hip_debug_f16w_auto_algo
    w16, x = C.inputs(544, 130, 40, key=6)
    K, M = 544, 130
    min_n(12)
    assert auto(K, M, 11) == GEMV and auto(K, M, 12) == WGEMM
    assert_bitwise(gpu_mul_mat(w16, x[:11], 0), gpu_mul_mat(w16, x[:11], GEMV))
    assert_bitwise(gpu_mul_mat(w16, x[:12], 0), gpu_mul_mat(w16, x[:12], WGEMM))
    min_n(-1)
    assert auto(K, M, 40) == MFMA
    assert_bitwise(gpu_mul_mat(w16, x, 0), gpu_mul_mat(w16, x, MFMA))
    # the three are different orders: the assertions above would show nothing otherwise
    assert np.any(G.bits(gpu_mul_mat(w16, x, WGEMM)) != G.bits(gpu_mul_mat(w16, x, MFMA)))
    assert np.any(G.bits(gpu_mul_mat(w16, x[:12], WGEMM)) != G.bits(gpu_mul_mat(w16, x[:12], GEMV)))


# ---- 7. graph capture -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K,M,N", [(2304, 70, 20), (96, 8200, 129)], ids=["plan1_k_split_4", "plan2_k_split_2"])
def test_graph_capture_after_reserve(switches, K, M, N):
    """both shapes take a plan with a K split: the slabs are rewritten by every replay, nothing carries over"""
    L = switches
    w16, x = C.inputs(K, M, N, key=7)
    eager = gpu_mul_mat(w16, x, WGEMM)                       # (the kernels' attributes are set outside the capture)
    assert C.within_bound(eager, *C.terms(K, M, N, key=7))[0]
    ggml_hip.check(L.ggml_hip_reserve_workspace_mm(K, N, M), "reserve")
    wd, xd, yd = DB.from_array(w16), DB.from_array(x), DB(N * M * 4)
    s = L.ggml_hip_default_stream()
    g = ggml_hip.Graph(s)
    with g:
        ggml_hip.mul_mat_f16(wd, K, M, xd, N, yd, algo=WGEMM, stream=s)
    for _ in range(2):
        ggml_hip.check(L.ggml_hip_memset(yd.ptr, 0xFF, N * M * 4, s))
        g.launch()
        ggml_hip.check(L.ggml_hip_stream_synchronize(s))
        assert_bitwise(yd.download((N, M), np.float32), eager)
    for b in (wd, xd, yd):
        b.free()


# ---- 8. hook path -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("backend", [ggml_hip.GGML_BACKEND_GPU, ggml_hip.GGML_BACKEND_GPU_SPLIT])
def test_hook_takes_the_gemm_from_the_threshold(lib, switches, backend):
    """A layer matrix's operand placement (weight uploaded by transform_tensor, host x, host dst).  The hook calls the
    F16 row with algo 0: with the threshold at 9 it runs algo 11, with the default algo 9."""
    L = switches
    K, M, N = 2304, 101, 33
    w16, x = C.inputs(K, M, N, key=8)
    ref, sab = C.terms(K, M, N, key=8)
    y11, y9 = gpu_mul_mat(w16, x, WGEMM), gpu_mul_mat(w16, x, MFMA)
    assert np.any(G.bits(y11) != G.bits(y9))                 # else the next assertions would show nothing
    staged = w16.copy()
    w = f16_tensor(staged, backend)
    L.ggml_hip_transform_tensor(staged.ctypes.data_as(ctypes.c_void_p), ctypes.byref(w))
    assert w.extra and w.backend == backend
    staged[:] = 0                                            # the loader frees its buffer
    y_np = np.zeros((N, M), np.float32)
    y, _xt = mm_node(w, x, y_np)
    try:
        L.ggml_hip_debug_set_f16w_wgemm_min_n(9)
        before = H.op_stats(L, reset=False)[0][H.OP_MUL_MAT]
        assert forward(L, y)
        assert H.op_stats(L, reset=False)[0][H.OP_MUL_MAT] == before + 1
        assert C.within_bound(y_np, ref, sab)[0]
        assert_bitwise(y_np, y11)
        L.ggml_hip_debug_set_f16w_wgemm_min_n(-1)
        y_np[:] = 0
        assert forward(L, y)
        assert_bitwise(y_np, y9)
    finally:
        L.ggml_hip_debug_set_f16w_wgemm_min_n(-1)
        L.ggml_hip_free_data(ctypes.byref(w))
    assert not w.extra


def test_hook_host_resident_weight(lib, switches):
    """a host-resident weight at N = 40 goes through the residency cache: one upload for two calls"""
    L = switches
    K, M, N = 544, 130, 40
    w16, x = R.random_case(C.rng_for(K, M, N, 9), M, K, N)   # a buffer of its own: the cache is keyed by the host address
    ref, sab = R.exact_terms(w16, x)
    w = f16_tensor(w16)
    y_np = np.zeros((N, M), np.float32)
    y, _xt = mm_node(w, x, y_np)
    try:
        L.ggml_hip_debug_set_f16w_wgemm_min_n(9)
        L.ggml_hip_weight_cache_invalidate(w16.ctypes.data_as(ctypes.c_void_p), w16.nbytes)
        hits0, miss0 = cache_stats(L)
        assert forward(L, y)
        assert cache_stats(L) == (hits0, miss0 + 1)          # one upload ...
        first = y_np.copy()
        y_np[:] = 0
        assert forward(L, y)
        assert cache_stats(L) == (hits0 + 1, miss0 + 1)      # ... for two calls
        assert_bitwise(y_np, first)
        assert C.within_bound(y_np, ref, sab)[0]
        assert_bitwise(y_np, gpu_mul_mat(w16, x, WGEMM))
    finally:
        L.ggml_hip_debug_set_f16w_wgemm_min_n(-1)
        L.ggml_hip_weight_cache_invalidate(w16.ctypes.data_as(ctypes.c_void_p), w16.nbytes)


# ---- 9. end to end ----------------------------------------------------------------------------------------------

@pytest.mark.skipif(not os.path.exists(HIP_LIB), reason="oracle/_ref/libllama_ref_hip.so not built")
def test_llama_full_offload_wgemm_prefill(tmp_path, switches):
    """The tiny "mostly F16" LLaMA through the reference's own llama.cpp, fully offloaded, fast kernels, threshold 9:
    the 40-token prompt's layer matrices run algo 11, the decode steps the GEMV.  The launch recorder (1 HIP graphs, 2
    launcher thread) and the own-AQL-queue mode (3) give the logits of eager launches bit for bit."""
    from test_gpu_llama_f16 import assert_layer_mul_mats_on_device, run_llama
    L = switches
    L.ggml_hip_debug_set_graph.argtypes = [ctypes.c_int]
    out = {}
    try:
        L.ggml_hip_debug_set_f16w_wgemm_min_n(9)
        for mode in (0, 1, 2, 3):
            ggml_hip.check(L.ggml_hip_debug_set_graph(mode), "set_graph")
            out[mode] = run_llama(tmp_path, exact=False)
    finally:
        L.ggml_hip_debug_set_graph(0)
        L.ggml_hip_debug_set_f16w_wgemm_min_n(-1)
    got, dec, ran, (gold, dgold) = out[0]
    assert np.isfinite(got).all() and np.isfinite(dec).all()
    assert_layer_mul_mats_on_device(ran)
    scale = np.abs(gold).max()
    print("threshold 9: max |logit - gold| / max |gold|", float(np.abs(got - gold).max() / scale),
          float(np.abs(dec - dgold).max() / scale))
    assert np.abs(got - gold).max() / scale < 2e-2 and np.abs(dec - dgold).max() / scale < 2e-2
    for mode in (1, 2, 3):
        assert np.array_equal(G.bits(out[mode][0]), G.bits(got)), mode
        assert np.array_equal(G.bits(out[mode][1]), G.bits(dec)), mode
    # the prompt did take another kernel than with the default threshold
    base = run_llama(tmp_path, exact=False)[0]
    assert np.any(G.bits(base) != G.bits(got))
