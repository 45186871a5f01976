"""The fused launches the hook's scheduler builds from back-to-back nodes (csrc/ggml-hip-fuse.cpp try_fuse,
csrc/ggml_ops.hip) against the numpy restatement of ggml.c's CPU ops (tests/ggml_ops_ref.py), bit for bit, every
tensor of the chain included: scale -> diag_mask_inf -> soft_max on both sides of each switch among
k_scale_mask_soft_max_reg<8>, <32> and the two-pass kernel, with separate buffers and in place; [add ->] rms_norm ->
mul through k_row_norm4 and k_add_rms_norm_mul; silu -> mul; and the decode attention (op_softmax_kqv /
op_kq_softmax_kqv) on both sides of the 512 / 1024-thread switch and of the KQ-fold limit.  Fusion is on; the fused
counters (the last slots of ggml_hip_debug_op_stats) show that the chain ran as one fused launch of its kind.  Which
kernel of a kind ran is not observed: it follows from the widths and the bounds in ggml_ops.hip.  Exact mode and
fast mode."""
import ctypes

import numpy as np
import pytest

import ggml_ops_ref as R
import hook_nodes as H
from ggml_ops_ref import assert_bits
from hip_env import ggml_hip, gpu_available

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason="needs a HIP device and libggml_hip.so")]

DB = ggml_hip.DeviceBuffer
FUSED_NORM, FUSED_SOFT_MAX, FUSED_SILU = 0, 1, 2             # g_fused slots (csrc/ggml-hip-ops.cpp)


@pytest.fixture(scope="module")
def tabs():
    return R.tables()


@pytest.fixture(params=[1, 0], ids=["exact", "fast"])
def g(request):
    """a node builder with fusion on, in exact or fast mode, the counters reset"""
    L = ggml_hip.load()
    prev = L.ggml_hip_get_exact()
    ggml_hip.check(L.ggml_hip_set_exact(request.param), "set_exact")
    H.set_fuse(L, 1)
    H.op_stats(L)
    n = H.Nodes(L)
    try:
        yield n
    finally:
        n.close()
        L.ggml_hip_set_exact(prev)
        H.set_fuse(L, H.FUSE_DEFAULT)


def ran(g, slot, ops):
    """the chain ran as one fused launch of kind `slot`, and exactly the nodes `ops` were taken (the slot names the
    chain, not the kernel the width selected)"""
    got, fused = H.op_stats(g.L)
    want = np.zeros_like(got)
    for op in ops:
        want[op] += 1
    assert np.array_equal(got, want), got.nonzero()
    assert fused[slot] == 1 and fused.sum() == 1, fused


@pytest.mark.parametrize("ncols", [3, 64, 65, 511, 512, 513, 2047, 2048, 2049, 2500])
@pytest.mark.parametrize("inplace", [False, True], ids=["separate", "inplace"])
def test_scale_mask_soft_max(g, tabs, ncols, inplace):
    """the prefill form: 2 heads x 3 tokens, n_past = ncols - 3, scale 1 / sqrt(128); row 0's scaled range exceeds
    65504, the last row carries -inf entries, the visible entries of row 1 (one masked) are all negative, so a
    maximum started at 0 changes its bits (asserted on the CPU).  Which kernel runs is implied by ncols and the
    bounds in op_scale_mask_soft_max_f32 (<= 512, <= 2048, above); the counters show only that the chain fused."""
    v = np.array([1.0 / np.sqrt(128.0)], np.float32)
    n_past = ncols - 3
    x = R.soft_max_rows(np.random.default_rng(ncols), ncols, 6, float(v[0])).reshape(2, 3, ncols)
    sc_ref = R.scale(x, v[0])
    assert sc_ref[0, 0].max() - sc_ref[0, 0].min() > 65504
    mk_ref = R.diag_mask_inf(sc_ref, n_past)
    sm_ref = R.soft_max(mk_ref, tabs[1])
    assert np.isfinite(sm_ref).all() and (sm_ref[:, 0, -2:] == 0).all() and (sm_ref[:, 2, 0] > 0).all()
    tx = g.dev(x)
    sc = g.node(H.OP_SCALE, tx, g.host(v, H.TYPE_F32), inplace)
    mk = g.node(H.OP_DIAG_MASK_INF, sc, g.host(np.array([n_past, int(inplace)], np.int32), H.TYPE_I32), inplace)
    sm = g.node(H.OP_SOFT_MAX, mk, None, inplace)
    for t in (sc, mk, sm):
        g.forward(t)
    assert_bits(g.read(sm, x.shape), sm_ref)                 # (the read flushes the held chain)
    if not inplace:
        assert_bits(g.read(sc, x.shape), sc_ref)
        assert_bits(g.read(mk, x.shape), mk_ref)
        assert_bits(g.read(tx, x.shape), x)
    ran(g, FUSED_SOFT_MAX, [H.OP_SCALE, H.OP_DIAG_MASK_INF, H.OP_SOFT_MAX])


@pytest.mark.parametrize("ncols,nrows", R.RMS_CHAIN_CASES)
@pytest.mark.parametrize("with_add", [True, False], ids=["add", "noadd"])
def test_add_rms_norm_mul(g, ncols, nrows, with_add):
    """k_row_norm4 (ncols % 4 == 0, <= 16384) and k_add_rms_norm_mul (the rest); one row of 64 n values in fast mode
    is held for a GEMV and runs as its own launch when the read-back flushes it.  The rows satisfy rms_order_free."""
    a, b, _ = R.rms_rows(ncols, nrows, R.rms_seed(ncols, nrows), with_add)
    w = np.random.default_rng(ncols).standard_normal((1, ncols)).astype(np.float32)
    ta, tb, tw = g.dev(a), g.dev(b), g.dev(w)
    nodes = []
    if with_add:
        nodes.append(g.node(H.OP_ADD, ta, tb))
    nodes.append(g.node(H.OP_RMS_NORM, nodes[-1] if with_add else tb))
    nodes.append(g.node(H.OP_MUL, nodes[-1], tw))
    for t in nodes:
        g.forward(t)
    x = R.add(a, b) if with_add else b
    nrm = R.rms_norm(x)
    assert_bits(g.read(nodes[-1], x.shape), R.mul(nrm, w))
    assert_bits(g.read(nodes[-2], x.shape), nrm)
    if with_add:
        assert_bits(g.read(nodes[0], x.shape), x)
    ran(g, FUSED_NORM, ([H.OP_ADD] if with_add else []) + [H.OP_RMS_NORM, H.OP_MUL])


@pytest.mark.parametrize("ncols,with_add", sorted(R.RMS_SQ_SEEDS))
def test_rms_norm_mul_rounds_each_square_to_float(g, ncols, with_add):
    """one row on which (double)(x * x) and (double)x * x give different output bits (asserted on the CPU): 6, 63 and
    4098 columns are k_add_rms_norm_mul's by their width, 64 k_row_norm4's"""
    a, b = R.rms_sq_row(ncols, with_add)
    w = np.random.default_rng(ncols).standard_normal((1, ncols)).astype(np.float32)
    nodes = [g.node(H.OP_ADD, g.dev(a), g.dev(b))] if with_add else []
    nodes.append(g.node(H.OP_RMS_NORM, nodes[-1] if with_add else g.dev(b)))
    nodes.append(g.node(H.OP_MUL, nodes[-1], g.dev(w)))
    for t in nodes:
        g.forward(t)
    x = R.add(a, b) if with_add else b
    nrm = R.rms_norm(x)
    assert_bits(g.read(nodes[-1], x.shape), R.mul(nrm, w))
    assert_bits(g.read(nodes[-2], x.shape), nrm)
    ran(g, FUSED_NORM, ([H.OP_ADD] if with_add else []) + [H.OP_RMS_NORM, H.OP_MUL])


@pytest.mark.parametrize("n", [1, 255, 256, 257, 11008])
def test_silu_mul(g, tabs, n):
    rng = np.random.default_rng(n)
    a = R.silu_spread(rng, n)
    a[:min(n, 4)] = np.array([0.0, -0.0, 70000.0, -5.9604645e-8], np.float32)[:min(n, 4)]
    b = rng.standard_normal(n).astype(np.float32)
    s = g.node(H.OP_SILU, g.dev(a))
    m = g.node(H.OP_MUL, s, g.dev(b))
    g.forward(s)
    g.forward(m)
    u = R.silu(a, tabs[0])
    assert_bits(g.read(m, (n,)), R.mul(u, b))
    assert_bits(g.read(s, (n,)), u)
    ran(g, FUSED_SILU, [H.OP_SILU, H.OP_MUL])


P, I64 = ctypes.c_void_p, ctypes.c_int64


def attn(L, fused, kc, q, vc, hd, nh, n_ctx, nkv):
    L.ggml_hip_debug_attn_decode.argtypes = [ctypes.c_int, P, I64, I64, P, I64, ctypes.c_int, P, I64, I64, I64, I64, I64,
                                             ctypes.c_int, ctypes.c_float, P, P, P, ctypes.c_int, P]
    n_embd = hd * nh
    kq, sm, kqv = DB(nh * nkv * 4), DB(nh * nkv * 4), DB(nh * hd * 4)
    ggml_hip.check(L.ggml_hip_debug_attn_decode(fused, kc.ptr, n_embd * 2, hd * 2, q.ptr, hd * 4, hd, vc.ptr, n_ctx * 2,
                                                hd * n_ctx * 2, nkv, nh, hd, nkv - 1, float(np.float32(1.0 / np.sqrt(hd))),
                                                kq.ptr, sm.ptr, kqv.ptr, 0, None), "attn")
    return sm.download((nh, nkv), np.float32), kqv.download((nh, hd), np.float32)


@pytest.mark.parametrize("hd,nh", [(64, 8), (80, 4), (128, 4), (256, 2)])
@pytest.mark.parametrize("nkv", [1, 33, 100, 101, 192, 193, 1000])
def test_decode_attention(tabs, hd, nh, nkv):
    """ggml_hip_debug_attn_decode, KQ folded in (fused = 1) and KQ's own launch first (fused = 0), on the reference
    llama.cpp's cache layouts (K rows of n_embd f16 per key, heads hd apart; V transposed: rows of n_ctx f16), in
    exact and in fast mode: the softmax rows and KQV bitwise decode_attention's"""
    L = ggml_hip.load()
    n_ctx, n_embd = 1024, hd * nh
    rng = np.random.default_rng(hd + nh + nkv)
    kc = (rng.standard_normal((n_ctx, n_embd)) * 0.5).astype(np.float16)
    vc = rng.standard_normal((n_embd, n_ctx)).astype(np.float16)
    q = rng.standard_normal(n_embd).astype(np.float32)
    K = kc[:nkv].reshape(nkv, nh, hd).transpose(1, 0, 2)
    V = vc.reshape(nh, hd, n_ctx)[:, :, :nkv]
    sm_ref, kqv_ref = R.decode_attention(K, q.reshape(nh, hd), V, np.float32(1.0 / np.sqrt(hd)), nkv - 1, tabs[1])
    assert np.isfinite(kqv_ref).all()
    dk, dq, dv = DB.from_array(kc), DB.from_array(q), DB.from_array(vc)
    prev = L.ggml_hip_get_exact()
    try:
        for exact in (1, 0):
            ggml_hip.check(L.ggml_hip_set_exact(exact), "set_exact")
            for fused in (0, 1):
                sm, kqv = attn(L, fused, dk, dq, dv, hd, nh, n_ctx, nkv)
                assert_bits(sm, sm_ref)
                assert_bits(kqv, kqv_ref)
    finally:
        L.ggml_hip_set_exact(prev)
