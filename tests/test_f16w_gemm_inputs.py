"""What the bound of the F16-weight prefill GEMM's tests (tests/test_gpu_f16w_gemm.py: |y - S| <= 1e-5 * sum |W *
fp16(x)|) asks of the inputs in tests/f16w_gemm_cases.py, on the CPU.  The bound is a condition on the inputs as well as
on the kernel: on every listed case the least favourable order a kernel could use (one sequential fp32 chain over K)
and the GEMV's order stay within a quarter of it, so a kernel that adds exact products in fp32 in any order has room;
and it does detect a wrong rounding of x: truncating x to fp16 instead of rounding to nearest even puts at least a
tenth of the outputs of every random-input case past it."""
import numpy as np
import pytest

import f16w_gemm_cases as C
import f16w_ref as R


def chain(w16, x):
    """f32 [N, M]: one fp32 chain per output over e = 0 .. K - 1 from +0"""
    w, xh = R.operands(w16, x)
    acc = np.zeros((xh.shape[0], w.shape[0]), np.float32)
    wt = np.ascontiguousarray(w.T)
    xt = np.ascontiguousarray(xh.T)
    with np.errstate(over="ignore", invalid="ignore"):
        for e in range(w.shape[1]):
            acc += np.multiply.outer(xt[e], wt[e])           # the product is exact in float32
    return acc


def truncated(x):
    """x rounded to fp16 toward zero, as float32"""
    h = x.astype(np.float16)
    over = np.abs(h.astype(np.float32)) > np.abs(x)
    h = np.where(over, np.nextafter(h, np.float16(0)), h)
    return h.astype(np.float32)


@pytest.mark.parametrize("i", range(len(C.CASES)), ids=C.IDS)
def test_chain_and_gemv_order_within_a_quarter_of_the_bound(i):
    w16, x, ref, sab = C.case(i)
    for name, y in (("chain", chain(w16, x)), ("gemv", R.gemv_schedule(w16, x))):
        assert np.isfinite(y).all()
        share = float((np.abs(y.astype(np.float64) - ref) / (sab + 1e-30)).max())
        print(C.IDS[i], name, share)
        assert share <= C.BOUND / 4, (name, share)


@pytest.mark.parametrize("i", [i for i, c in enumerate(C.CASES) if not c[3]],
                         ids=[C.IDS[i] for i, c in enumerate(C.CASES) if not c[3]])
def test_truncated_x_is_past_the_bound(i):
    w16, x, ref, sab = C.case(i)
    w = w16.view(np.float16).astype(np.float64)
    y = truncated(x).astype(np.float64) @ w.T                # exact sums of the wrong products
    past = np.abs(y - ref) > C.BOUND * sab + 1e-30
    print(C.IDS[i], "past the bound:", float(past.mean()))
    assert past.mean() >= 0.10


def test_plan_cases_are_well_formed():
    for K, M, N, plan in C.PLAN_CASES:
        assert K % 32 == 0 and M >= 1 and N >= 1 and 1 <= plan <= 3
    assert C.BIG in C.PLAN_CASES and C.CASES[C.WIDE][:3] == (4160, 70, 130)
