"""The inputs of the GEMV prologue tests (tests/gemv_norm_util.py chain_case, used by tests/test_gpu_gemv_prologue.py)
and of the epilogue tests' prologue reference (tests/test_gpu_gemv_epi.py), checked without a device: every rms_norm
row is order-free (tests/ggml_ops_ref.py rms_order_free: the kernel's double sum may take any order), every silu input
has a finite fp16 with the special values in front, and every reference `out` is finite and not all zero."""
import numpy as np
import pytest

import gemv_norm_util as U
import ggml_ops_ref as R


@pytest.fixture(scope="module")
def tabs():
    return R.tables()


KIND1 = sorted(set(U.KS_KIND1) | set(U.HOOK_KS[1]) | set(U.HOOK_KS_WIDE[1]))
KIND2 = sorted(set(U.KS_KIND2) | set(U.HOOK_KS[2]) | set(U.HOOK_KS_WIDE[2]))


@pytest.mark.parametrize("with_add", [True, False], ids=["add", "noadd"])
@pytest.mark.parametrize("K", KIND1)
def test_norm_chain_inputs(tabs, K, with_add):
    c = U.chain_case(1, K, with_add, tabs)
    U.assert_case_inputs(c)
    assert (c["a"] is None) == (not with_add) and c["sum"].shape == c["out"].shape == (K,)
    # and then every correct double summation gives ggml.c's float mean: whole, reversed, per 64-lane wave first
    x = c["sum"]
    sq = (x * x).astype(np.float32).astype(np.float64)
    m = R.rms_norm_mean(x)
    for s in (sq.sum(), sq[::-1].cumsum()[-1], sq.reshape(-1, 64).sum(axis=1).sum()):
        assert R.bits(np.float32(s / K)) == R.bits(m)


@pytest.mark.parametrize("K", KIND2)
def test_silu_chain_inputs(tabs, K):
    c = U.chain_case(2, K, False, tabs)
    U.assert_case_inputs(c)
    assert c["sum"] is None and c["w"] is None
    h = R.fp16_bits(c["a"])
    assert len(set(((h >> 10) & 31).tolist())) >= (20 if K >= 512 else 8)      # spread over the fp16 exponents
    assert R.bits(c["norm"][:4]).tolist()[:2] == [0, 0x80000000]                # silu(+-0) keeps the sign


def test_epilogue_tests_rms_rows_are_order_free():
    """the rows tests/test_gpu_gemv_epi.py draws (its seeds and its order of draws exactly)"""
    for K, hd, nh, _ in U.EPI_ROPE_CASES:
        M = hd * nh
        rng = np.random.default_rng(K + hd + nh)
        for _ in range(3):
            U.rand_q4(M, K, rng)
        b, a = rng.standard_normal(K).astype(np.float32), rng.standard_normal(K).astype(np.float32)
        assert R.rms_order_free(R.add(a, b)), (K, hd, nh)
    for K, M in U.EPI_GLU_CASES:
        rng = np.random.default_rng(K + M)
        for _ in range(2):
            U.rand_q4(M, K, rng)
        assert R.rms_order_free(rng.standard_normal(K).astype(np.float32)), (K, M)
