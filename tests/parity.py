"""Shared parity helpers (numpy): block decoding and the fp32-accumulator bound.

The north-star tolerance is "within 1e-3 relative on the fp32 accumulator".
A bare relative error is ill-conditioned where y ~ 0 (cancellation), so every
y comparison uses the per-element bound of SURVEY.md §7.3:

    |y_gpu - y_ref| <= rtol * |y_ref| + atol_blocks * S_abs,
    S_abs[n, m] = sum_b |d_w[m,b] * d_x[n,b] * sumi[n,m,b]|

and also reports max relative error over |y_ref| > 1e-3 * max|y_ref|.  SURVEY §7.3 sets
atol_blocks = 1e-6; a float32 simulation of the GEMM's block-sequential fma chain against the
oracle at 4096x4096x512 needs at most 8.2e-8 (12x margin).  Every check_y call records its
worst relative error and the smallest atol_blocks that would have passed; conftest.py prints the
table at the end of the run (`parity report`).
"""
import os

import numpy as np

REPORT = []          # (test id, n elements, max rel (well conditioned), atol_blocks needed)

QK = 32


def split_q4_0(wq, K):
    """uint8 [M, K/32*18] -> (d_w f32 [M, nb], w int8 [M, nb, 32]) with w = nib - 8."""
    nb = K // QK
    b = np.ascontiguousarray(wq).reshape(-1, nb, 18)
    d = b[:, :, 0:2].copy().view(np.float16)[:, :, 0].astype(np.float32)
    qs = b[:, :, 2:18]
    lo = (qs & 0x0F).astype(np.int8) - 8
    hi = (qs >> 4).astype(np.int8) - 8
    return d, np.concatenate([lo, hi], axis=2)


def split_q8_0(xq, K):
    """uint8 [N, K/32*34] -> (d_x f32 [N, nb], q int8 [N, nb, 32])."""
    nb = K // QK
    b = np.ascontiguousarray(xq).reshape(-1, nb, 34)
    d = b[:, :, 0:2].copy().view(np.float16)[:, :, 0].astype(np.float32)
    q = b[:, :, 2:34].copy().view(np.int8)
    return d, q


def block_terms(wq, xq, K):
    """(y_exact f64 [N, M], S_abs f64 [N, M]) from the integer block sums."""
    dw, w = split_q4_0(wq, K)
    dx, q = split_q8_0(xq, K)
    sumi = np.einsum("mbj,nbj->nmb", w.astype(np.int32), q.astype(np.int32))
    d = dx.astype(np.float64)[:, None, :] * dw.astype(np.float64)[None, :, :]
    t = d * sumi
    return t.sum(axis=2), np.abs(t).sum(axis=2)


def s_abs_exact(wq, xq, K, n_chunk=None):
    """S_abs[n, m] = sum_b |d_w d_x sumi| exactly (integer block sums through float32 BLAS: every
    partial sum is an integer below 2^24, so the products are exact), chunked over blocks so that
    full LLaMA shapes (512 x 11008 x 128 blocks) fit in memory.  Replaces the elementwise
    |W_deq| @ |X_deq|^T upper bound, which is ~sqrt(32)x looser."""
    dw, w = split_q4_0(wq, K)
    dx, q = split_q8_0(xq, K)
    N, M, nb = q.shape[0], w.shape[0], K // QK
    out = np.zeros((N, M), np.float32)
    wf = w.astype(np.float32)
    qf = q.astype(np.float32)
    for b in range(nb):
        s = qf[:, b, :] @ wf[:, b, :].T
        np.abs(s, out=s)
        s *= np.abs(dx[:, b])[:, None]
        s *= np.abs(dw[:, b])[None, :]
        out += s
    return out.astype(np.float64)


def check_y(y_got, y_ref, s_abs, rtol=1e-3, atol_blocks=1e-6):
    """Assert the per-element bound; return (max_rel_well_conditioned, max_abs_err)."""
    y_got = np.asarray(y_got, dtype=np.float64)
    y_ref = np.asarray(y_ref, dtype=np.float64)
    err = np.abs(y_got - y_ref)
    bound = rtol * np.abs(y_ref) + atol_blocks * s_abs
    with np.errstate(divide="ignore", invalid="ignore"):
        need = np.where(s_abs > 0, (err - rtol * np.abs(y_ref)) / s_abs, np.where(err > rtol * np.abs(y_ref), np.inf, 0))
    need_max = float(max(need.max(), 0.0)) if need.size else 0.0
    bad = err > bound
    if bad.any():
        i = np.argwhere(bad)[0]
        raise AssertionError(f"{bad.sum()} elements out of bound; first {tuple(i)}: got {y_got[tuple(i)]} "
                             f"ref {y_ref[tuple(i)]} bound {bound[tuple(i)]}")
    big = np.abs(y_ref) > 1e-3 * np.abs(y_ref).max()
    rel = (err[big] / np.abs(y_ref[big])).max() if big.any() else 0.0
    REPORT.append((os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0], int(err.size), float(rel), need_max))
    return float(rel), float(err.max())


def check_y_terms(y_got, y64, s_abs, nb, roundings=2):
    """Assert |y - y64| <= 1.01 * (nb + roundings) * 2^-24 * S_abs, the bound with no relative term; return the
    multiple of 2^-24 * S_abs the worst element needed (a record of what was measured, not a threshold).

    y64, S_abs: block_terms on the oracle's q8_0 bytes of x (the exact sum of the exact block terms).  Derivation: the
    integer block sums are exact and d_w * d_x is exact in fp32 (two 11-bit significands), so term b reaches the
    accumulator as fl(p * sumi) or inside an fma: at most `roundings` roundings before the accumulation (2 covers
    (d_x * sumi) * d_w), each of relative size 2^-24 of |term|.  Whatever the tree, a term then passes through at most
    nb - 1 additions, each rounding a partial sum that is at most S_abs in magnitude (to first order): in all
    (nb - 1 + roundings) * 2^-24 * S_abs, rounded up to nb + roundings; the factor 1.01 covers the second-order terms
    ((1 + 2^-24)^nb - 1 - nb 2^-24 < 1e-3 nb 2^-24 for nb <= 2^13) and the final rounding of the comparison itself.
    A caller whose kernel rounds more often, or keeps the nibble dot and the -8 sum(q) correction as separate floats,
    passes the count (or the larger magnitude sum as s_abs) read from the kernel's code."""
    y_got = np.asarray(y_got, dtype=np.float64)
    y64 = np.asarray(y64, dtype=np.float64)
    s_abs = np.asarray(s_abs, dtype=np.float64)
    assert y_got.shape == y64.shape == s_abs.shape
    err = np.abs(y_got - y64)
    u = 2.0 ** -24
    with np.errstate(divide="ignore", invalid="ignore"):
        need = np.where(s_abs > 0, err / (u * s_abs), np.where(err > 0, np.inf, 0.0))
    need_max = float(need.max()) if need.size else 0.0
    bad = ~(err <= 1.01 * (nb + roundings) * u * s_abs)           # a NaN in y is out of bound
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{bad.sum()} elements outside (nb + {roundings}) * 2^-24 * S_abs (nb = {nb}); first {i}: "
                             f"got {y_got[i]!r} exact {y64[i]!r} needs {need[i]:.3g} * 2^-24 * S_abs")
    return need_max


def assert_equal_values(y_got, y64):
    """y == float32(y64) as values (-0.0 == +0.0 is accepted, nothing else differs): the order-free comparison."""
    y_got = np.asarray(y_got)
    assert y_got.dtype == np.float32 and y_got.shape == y64.shape
    want = np.asarray(y64, dtype=np.float64).astype(np.float32)
    assert np.array_equal(want.astype(np.float64), y64), "y64 is not representable in fp32: not an order-free case"
    bad = ~(y_got == want)
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{bad.sum()} of {bad.size} elements differ from float32(y64); first (n, m) = {i}: "
                             f"got {y_got[i]!r} exact {want[i]!r}")
