"""Each single-node device op of a LLaMA layer (csrc/ggml_ops.hip: add, mul, scale, silu, diag_mask_inf, rms_norm,
soft_max, rope, cpy) against the numpy restatement of ggml.c's CPU op (tests/ggml_ops_ref.py, itself pinned to
fixtures recorded from the compiled reference by tests/test_ggml_ops_ref.py), bit for bit.  The nodes are hand-built
ggml_tensors run through ggml_hip_compute_forward with fusion off, so each is its own launch; the op counters show
the device took it.  Tables and cos / sin come from the host libm of the machine the test runs on, as the
backend's do.  Shapes: one element, the sizes around a wave and a workgroup, odd sizes, more than one workgroup,
and both kernels of rms_norm (rows of 4 n <= 16384 values, and the rest)."""
import numpy as np
import pytest

import ggml_ops_ref as R
import hook_nodes as H
from ggml_ops_ref import assert_bits
from golden_io import load
from hip_env import ggml_hip, gpu_available

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason="needs a HIP device and libggml_hip.so")]


@pytest.fixture(scope="module")
def tabs():
    return R.tables()


@pytest.fixture()
def g():
    """a node builder with fusion off (every node its own launch) and the counters reset"""
    L = ggml_hip.load()
    H.set_fuse(L, 0)
    H.op_stats(L)
    n = H.Nodes(L)
    try:
        yield n
    finally:
        n.close()
        H.set_fuse(L, H.FUSE_DEFAULT)


def taken(g, op, n=1):
    ops, fused = H.op_stats(g.L)
    assert ops[op] == n and ops.sum() == n, ops.nonzero()
    assert fused.sum() == 0


@pytest.mark.parametrize("n", [1, 255, 256, 257, 70001])
def test_add_and_scale(g, n):
    rng = np.random.default_rng(n)
    a = R.silu_spread(rng, n)
    b = rng.standard_normal(n).astype(np.float32)
    v = np.array([1.0 / np.sqrt(128.0)], np.float32)
    ta, tb = g.dev(a), g.dev(b)
    y = g.node(H.OP_ADD, ta, tb)
    g.forward(y)
    assert_bits(g.read(y, (n,)), R.add(a, b))
    taken(g, H.OP_ADD)
    s = g.node(H.OP_SCALE, ta, g.host(v, H.TYPE_F32))
    g.forward(s)
    assert_bits(g.read(s, (n,)), R.scale(a, v[0]))
    taken(g, H.OP_SCALE)


@pytest.mark.parametrize("ne00", [1, 6, 256])
@pytest.mark.parametrize("ne11", [1, 5])
def test_mul_rows_repeat(g, ne00, ne11):
    rng = np.random.default_rng(ne00 + ne11)
    a = rng.standard_normal((3, 5, ne00)).astype(np.float32)
    b = rng.standard_normal((1, ne11, ne00)).astype(np.float32)
    y = g.node(H.OP_MUL, g.dev(a), g.dev(b))
    g.forward(y)
    assert_bits(g.read(y, a.shape), R.mul(a, b))
    taken(g, H.OP_MUL)


@pytest.mark.parametrize("which", ["fixture", "spread"])
def test_silu(g, tabs, which):
    x = load("ops", "silu_x") if which == "fixture" else R.silu_spread(np.random.default_rng(11008), 11008)
    y = g.node(H.OP_SILU, g.dev(x))
    g.forward(y)
    assert_bits(g.read(y, x.shape), R.silu(x, tabs[0]))
    taken(g, H.OP_SILU)


@pytest.mark.parametrize("ncols", [1, 65])
def test_diag_mask_inf(g, ncols):
    n_past = max(0, ncols - 3)                                # (ggml.c asserts n_past >= 0)
    x = np.random.default_rng(ncols).standard_normal((2, 3, ncols)).astype(np.float32)
    y = g.node(H.OP_DIAG_MASK_INF, g.dev(x), g.host(np.array([n_past, 0], np.int32), H.TYPE_I32))
    g.forward(y)
    ref = R.diag_mask_inf(x, n_past)
    assert ncols == 1 or np.isinf(ref).sum() == 2 * 3
    assert_bits(g.read(y, x.shape), ref)
    taken(g, H.OP_DIAG_MASK_INF)


@pytest.mark.parametrize("ncols,nrows", R.RMS_NODE_CASES)
def test_rms_norm(g, ncols, nrows):
    """k_row_norm4 (ncols % 4 == 0, <= 16384) and k_rms_norm_f32, each with its own order of the double sum: the rows
    satisfy rms_order_free, so the float mean is ggml.c's whatever the order"""
    _, x, _ = R.rms_rows(ncols, nrows, R.rms_seed(ncols, nrows))
    y = g.node(H.OP_RMS_NORM, g.dev(x))
    g.forward(y)
    assert_bits(g.read(y, x.shape), R.rms_norm(x))
    taken(g, H.OP_RMS_NORM)


@pytest.mark.parametrize("ncols,with_add", sorted(R.RMS_SQ_SEEDS))
def test_rms_norm_rounds_each_square_to_float(g, ncols, with_add):
    """rows on which (double)(x * x) and (double)x * x give different output bits (asserted on the CPU)"""
    a, b = R.rms_sq_row(ncols, with_add)
    x = R.add(a, b) if with_add else b
    y = g.node(H.OP_RMS_NORM, g.dev(x))
    g.forward(y)
    assert_bits(g.read(y, x.shape), R.rms_norm(x))
    taken(g, H.OP_RMS_NORM)


@pytest.mark.parametrize("ncols", [1, 63, 64, 65, 700, 2500])
@pytest.mark.parametrize("nrows", [1, 5])
def test_soft_max(g, tabs, ncols, nrows):
    """row 0 has a range beyond 65504, the last row -inf entries, row 1 (of 5) is negative throughout: a maximum
    started at 0 changes its bits (asserted on the CPU)"""
    x = R.soft_max_rows(np.random.default_rng(ncols * 8 + nrows), ncols, nrows)
    assert ncols == 1 or (np.isinf(x[-1]).any() and x[0].max() - x[0].min() > 65504)
    y = g.node(H.OP_SOFT_MAX, g.dev(x))
    g.forward(y)
    ref = R.soft_max(x, tabs[1])
    assert np.isfinite(ref).all()
    assert_bits(g.read(y, x.shape), ref)
    taken(g, H.OP_SOFT_MAX)


@pytest.mark.parametrize("ne0", [64, 128])
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("ntok", [1, 7])
@pytest.mark.parametrize("n_past", [0, 37])
def test_rope(g, ne0, half, ntok, n_past):
    n_dims = ne0 // 2 if half else ne0
    x = (np.random.default_rng(ne0 + ntok + n_past).standard_normal((ntok, 3, ne0)) * 2).astype(np.float32)
    y = g.node(H.OP_ROPE, g.dev(x), g.host(np.array([n_past, n_dims, 0, 0], np.int32), H.TYPE_I32))
    g.forward(y)
    assert_bits(g.read(y, x.shape), R.rope(x, n_past, n_dims))
    taken(g, H.OP_ROPE)


@pytest.mark.parametrize("f16", [True, False])
def test_cpy_into_transposed_view(g, f16):
    x = np.random.default_rng(7).standard_normal((2, 5, 7)).astype(np.float32)
    x[0, 0, :4] = [1.00048828125, 65519.9, 65520.0, -2.98023223876953125e-8]      # fp16 ties, the overflow boundary
    gt, dt, es = (H.TYPE_F16, np.uint16, 2) if f16 else (H.TYPE_F32, np.float32, 4)
    base = g.dev(np.zeros((2, 7, 5), dt), gt)
    target = g.view(base, (7, 5, 2), (5 * es, es, 35 * es), gt)      # ggml_transpose of the base
    y = g.cpy_node(g.dev(x), target)
    g.forward(y)
    got = g.read(base, (70,), dt)
    ref = R.cpy(x, np.zeros(70, dt), (7, 5, 2), (5 * es, es, 35 * es))
    assert np.array_equal(got.view(np.uint16 if f16 else np.uint32), ref.view(np.uint16 if f16 else np.uint32))
    assert np.array_equal(ref.reshape(2, 7, 5).transpose(0, 2, 1), R.fp16_bits(x) if f16 else x)
    taken(g, H.OP_CPY)
