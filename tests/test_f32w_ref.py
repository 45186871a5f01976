"""CPU checks of the F32-weight restatements (tests/f32w_ref.py): mul_mat_f32 (ggml_vec_dot_f32's AVX2 + FMA schedule)
reproduces the fixtures the reference's own ggml_mul_mat wrote (tests/golden/gen_golden_f32w.c: K = 32, 288, 1056 on
1 and 4 threads, with +-0, subnormal weights and magnitudes spread over 2^+-20) bit for bit; the GEMV's and the GEMM's
orders (S = 1, 2, 4) are within the derived bound 1.01 K 2^-24 sum|w x| of the float64 sum on the very inputs of the GPU
tests; and their bits differ from mul_mat_f32's and from each other's there, so a bitwise match on the device tells the
three orders apart."""
import numpy as np
import pytest

import f32w_ref as R
import ggml_ops_ref as G
import golden_io

IDS = ["K%d_M%d_N%d%s" % (c[0], c[1], c[2], "_special" if c[4] else "") for c in R.CASES]


@pytest.mark.parametrize("K", [32, 288, 1056])
def test_mul_mat_f32_reproduces_the_reference(K):
    w, x = golden_io.load("f32w", f"w{K}_f32"), golden_io.load("f32w", f"x{K}_f32")
    assert w.shape == (24, K) and x.shape == (3, K)
    y = R.mul_mat_f32(w, x)
    for threads in ("t1", "t4"):
        gold = golden_io.load("f32w", f"y{K}_{threads}")
        assert gold.shape == (3, 24) and np.isfinite(gold).all()
        assert np.array_equal(G.bits(y), G.bits(gold)), threads
    # the fixtures do hold what they are there for: +-0 and subnormal weights, and a product that only survives if
    # subnormals are kept (row 0: 2^-130 * 2^20)
    wb = G.bits(w)
    assert (wb == 0x80000000).any() and (wb == 0).any() and ((wb & 0x7F800000) == 0)[w != 0].any()
    assert (gold[:, 0] == np.float32(2.0 ** -110)).all()
    assert np.log2(np.abs(w[w != 0]).max() / np.abs(w[3:][w[3:] != 0]).min()) > 30


@pytest.mark.parametrize("i", range(len(R.CASES)), ids=IDS)
def test_schedules_within_the_derived_bound(i):
    K = R.CASES[i][0]
    w, x = R.case(i)
    s64, sab = R.exact_terms(w, x)
    lim = R.bound(K, sab)
    for kind, S in (("gemv", 1), ("exact", 1), ("gemm", 1), ("gemm", 2), ("gemm", 4)):
        y = R.ref(i, kind, S)
        assert y.shape == (x.shape[0], w.shape[0]) and np.isfinite(y).all()
        err = np.abs(y.astype(np.float64) - s64)
        print(R.CASES[i], kind, S, "max err / bound", float((err / (lim + 1e-300)).max()))
        assert (err <= lim).all(), (kind, S)


def test_the_three_orders_differ():
    for i in range(len(R.CASES)):
        exact = G.bits(R.ref(i, "exact"))
        assert (G.bits(R.ref(i, "gemv")) != exact).any(), i
        assert (G.bits(R.ref(i, "gemm", 1)) != exact).any(), i
        assert (G.bits(R.ref(i, "gemm", 1)) != G.bits(R.ref(i, "gemv"))).any(), i
    i = len(R.GEMV_CASES) + 4                                # K = 2048: the splits differ from each other too
    assert (G.bits(R.ref(i, "gemm", 1)) != G.bits(R.ref(i, "gemm", 2))).any()
    assert (G.bits(R.ref(i, "gemm", 2)) != G.bits(R.ref(i, "gemm", 4))).any()


def test_restatement_properties():
    """a column's y does not depend on the columns beside it or on the rows beside its row; a zero row gives +0; a
    lane past K adds nothing; a split that leaves no whole chunks runs as the next smaller one"""
    i = 3                                                    # K = 1504, M = 65, N = 17
    w, x = R.case(i)
    y = R.ref(i, "gemv")
    assert np.array_equal(G.bits(R.gemv_schedule(w, x[3:4])), G.bits(y[3:4]))
    assert np.array_equal(G.bits(R.gemv_schedule(w[10:12], x)), G.bits(y[:, 10:12]))
    z = R.gemv_schedule(np.zeros((2, 64), np.float32), np.full((1, 64), -3.0, np.float32))
    assert np.array_equal(G.bits(z), np.zeros((1, 2), np.uint32))
    w1 = np.arange(1, 33, dtype=np.float32)[None, :]
    one = np.ones((1, 32), np.float32)
    assert R.gemv_schedule(w1, one)[0, 0] == R.gemm_schedule(w1, one, 4)[0, 0] == R.mul_mat_f32(w1, one)[0, 0] == 528
    assert [R.gemm_ksplit(K, 4) for K in (32, 64, 128, 4544, 1504)] == [1, 2, 4, 2, 1]
    assert np.array_equal(G.bits(R.gemm_schedule(w, x[:2], 4)), G.bits(R.gemm_schedule(w, x[:2], 1)))
