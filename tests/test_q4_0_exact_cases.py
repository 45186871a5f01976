"""The order-free exact cases and the term bound (tests/q4_0_exact_cases.py, parity.check_y_terms) on the CPU:
the construction holds (both reference quantizers return the stated bytes, the oracle's mul_mat and random fp32
summation orders give float32(y64) exactly), the oracle's own fp32 order is inside the term bound on every gaussian
case the GPU module uses, and three corrupted references that the old bound (check_y at 1e-3 / 1e-6) accepts are
rejected by the term bound and by the order-free equality.
"""
import numpy as np
import pytest

import oracle as O
import q4_0_exact_cases as C
from parity import QK, assert_equal_values, block_terms, check_y, check_y_terms, split_q4_0, split_q8_0

# the windows of the construction, one row per K (the K between rows take the next row's)
TABLE = [(64, 4, 3, 127), (256, 3, 2, 127), (1024, 2, 1, 127), (4096, 1, 0, 127), (4544, 1, 0, 127),
         (11008, 0, 0, 15), (13824, 0, 0, 15)]


def test_windows_are_the_stated_ones():
    assert C.WINDOWS == TABLE
    assert C.windows_for(128) == (3, 2, 127) and C.windows_for(12352) == (0, 0, 15) and C.windows_for(320) == (2, 1, 127)


@pytest.mark.parametrize("K,span_w,span_x,qmax", TABLE)
def test_construction_holds(K, span_w, span_x, qmax):
    """Both quantizers return exactly the expected q8_0 bytes; the oracle's mul_mat (AVX2 order, 1 and 8 threads,
    with and without the pool) is float32(y64) as values; the nibbles use all 16 codes and d_w both signs."""
    M, N = 24, 3
    c = C.order_free_case(K, M, N, seed=K, span_w=span_w, span_x=span_x, qmax=qmax)
    assert c["mag_log2"] < 23.0
    for mode in ("avx2", "ref"):
        assert np.array_equal(O.quantize_q8_0(c["x"], mode), c["xq"]), mode
    for nthreads in (1, 8):
        for pool in (False, True):
            assert_equal_values(O.mul_mat(c["wq"], K, c["x"], nthreads=nthreads, mode="avx2", pool=pool), c["y64"])
    dw, w = split_q4_0(c["wq"], K)
    assert set(np.unique(w)) == set(range(-8, 8)) and (dw > 0).any() and (dw < 0).any()
    assert len(np.unique(np.abs(dw))) == span_w + 1
    dx, q = split_q8_0(c["xq"], K)
    assert np.all(np.abs(q.astype(np.int32)).max(axis=2) == 127)
    others = np.sort(np.abs(q.astype(np.int32)), axis=2)[:, :, :-1]
    assert others.max() <= qmax


@pytest.mark.parametrize("K,span_w,span_x,qmax", TABLE)
def test_random_fp32_orders_are_exact(K, span_w, span_x, qmax):
    """Sequential fp32 sums of the block terms in random orders, and of the 2 nb terms of a kernel that keeps the
    unsigned-nibble dot and the -8 sum(q) correction apart, equal float32(y64) bit for bit."""
    M, N = 16, 2
    c = C.order_free_case(K, M, N, seed=K + 1, span_w=span_w, span_x=span_x, qmax=qmax)
    dw, w = split_q4_0(c["wq"], K)
    dx, q = split_q8_0(c["xq"], K)
    d = dx[:, None, :] * dw[None, :, :]                                       # fp32 product, exact
    assert d.dtype == np.float32
    sumi = np.einsum("mbj,nbj->nmb", w.astype(np.int32), q.astype(np.int32))
    udot = np.einsum("mbj,nbj->nmb", w.astype(np.int32) + 8, q.astype(np.int32))
    corr = -8 * q.astype(np.int32).sum(axis=2)[:, None, :] + 0 * sumi
    want = c["y64"].astype(np.float32)
    rng = np.random.default_rng(K)
    for terms in (d * sumi.astype(np.float32),
                  np.concatenate([d * udot.astype(np.float32), d * corr.astype(np.float32)], axis=2)):
        assert terms.dtype == np.float32
        for _ in range(3):
            p = rng.permutation(terms.shape[2])
            got = np.cumsum(terms[:, :, p], axis=2, dtype=np.float32)[:, :, -1]
            assert np.array_equal(got, want)


def test_exact_terms_is_block_terms():
    """The block-at-a-time form the cases use is parity.block_terms: equal exactly on an order-free case, and to a
    few float64 roundings of S_abs (the two add the same exact terms in different orders) on a gaussian one."""
    c = C.order_free(1024, 65, 9)
    y, s = block_terms(c["wq"], c["xq"], 1024)
    assert np.array_equal(y, c["y64"]) and np.array_equal(s, c["s_abs"])
    g = C.gaussian(O, 4544, 73, 33, spread=True)
    y, s = block_terms(g["wq"], g["xq"], 4544)
    assert np.all(np.abs(y - g["y64"]) <= 2.0 ** -45 * s) and np.all(np.abs(s - g["s_abs"]) <= 2.0 ** -45 * s)


def test_headroom_holds_for_every_gpu_case():
    """Every order-free case of the GPU module satisfies the asserted condition (build() raises otherwise)."""
    for K, M, N in C.all_shapes():
        assert C.order_free(K, M, N)["mag_log2"] < 23.0, (K, M, N)
    assert C.extreme_order_free(*C.EXTREME_SHAPE)["mag_log2"] < 23.0


def test_extreme_twin_has_the_extreme_blocks():
    c = C.extreme_order_free(*C.EXTREME_SHAPE)
    K = C.EXTREME_SHAPE[0]
    _, w = split_q4_0(c["wq"], K)
    _, q = split_q8_0(c["xq"], K)
    assert np.all(w[:8] == -8) and np.all(w[8:16] == 7)
    assert np.all(q[:8] == 127) and np.all(q[8:16] == -127)
    assert np.all((q[16:24] != 0).sum(axis=2) == 1)
    sumi = np.einsum("mbj,nbj->nmb", w.astype(np.int32), q.astype(np.int32))
    assert np.abs(sumi).max() == 32 * 8 * 127
    assert np.array_equal(O.quantize_q8_0(c["x"], "avx2"), c["xq"])
    assert_equal_values(O.mul_mat(c["wq"], K, c["x"], nthreads=4), c["y64"])


def _s_abs_lanes(wq, xq, K):
    """The magnitude sum of the oracle's AVX2 order (oracle/q4_0_oracle.c oracle_vec_dot_q4_0_q8_0_avx2): lane l
    of 8 accumulates fma(d_x d_w, float(sum of the products of elements 4l .. 4l + 3), acc_l), so its terms are the 8
    quarter-block sums of a block, kept as separate floats: sum_b |d| sum_l |sum_{4l..4l+3} w q| >= S_abs."""
    dw, w = split_q4_0(wq, K)
    dx, q = split_q8_0(xq, K)
    wf, qf = w.astype(np.float32), q.astype(np.float32)
    s = np.zeros((q.shape[0], w.shape[0]))
    for b in range(K // QK):
        part = sum(np.abs(qf[:, b, 4 * l:4 * l + 4] @ wf[:, b, 4 * l:4 * l + 4].T) for l in range(8))
        s += part.astype(np.float64) * np.abs(dx.astype(np.float64)[:, b, None] * dw.astype(np.float64)[None, :, b])
    return s


@pytest.mark.parametrize("spread", [False, True], ids=["gauss", "spread"])
def test_oracle_is_inside_the_term_bound(spread):
    """One legitimate fp32 order alone meets the bound on every gaussian case of the GPU module: the oracle's scalar
    order (ggml.c:2588-2606, sumf += ((float)sumi * d_w) * d_x over the blocks in order: two roundings per term, then
    the chain) against S_abs as it stands.  The oracle's AVX2 order does not add block sums: it keeps 8 quarter-block
    sums per block in 8 lane chains of nb fmas each and adds the lanes in 3 steps (hsum_float_8), so a term passes
    through at most nb - 1 + 3 additions, and its magnitude sum is the quarter-block one (_s_abs_lanes, read from
    oracle_vec_dot_q4_0_q8_0_avx2), which is passed in: at K = 64 two quarter sums that cancel inside a block make
    it 1.3 times S_abs."""
    worst = {"scalar": 0.0, "avx2": 0.0}
    for K, M, N in C.all_shapes():
        c = C.gaussian(O, K, M, N, spread=spread)
        nb = K // QK
        rows = min(M, 30000 // N)                      # one call per output: the first rows of the 4100-row case
        y = np.array([[O.vec_dot(K, wr, xr, "scalar") for wr in c["wq"][:rows]] for xr in c["xq"]], np.float32)
        worst["scalar"] = max(worst["scalar"], check_y_terms(y, c["y64"][:, :rows], c["s_abs"][:, :rows], nb))
        y = O.mul_mat(c["wq"], K, c["x"], nthreads=4, mode="avx2")
        worst["avx2"] = max(worst["avx2"], check_y_terms(y, c["y64"], _s_abs_lanes(c["wq"], c["xq"], K), nb))
    print(f"oracle worst need, in 2^-24 * (its magnitude sum): {worst}")


# ------------------------------------------------------------------------------------------- sensitivity
def _corrupt(kind, wq, xq, K, pos):
    """A copy of (wq, xq) with element pos = (block, j) of row 0 / token 0 corrupted."""
    wq, xq = wq.copy(), xq.copy()
    b, j = pos
    if kind == "q8_lsb":                                  # one q8_0 value moved by one LSB
        v = int(xq[0, b * 34 + 2 + j].astype(np.int8))
        xq[0, b * 34 + 2 + j] = np.array(v + 1 if v < 127 else v - 1, np.int8).view(np.uint8)
    elif kind == "nibble":                                # one nibble of weight row 0 changed by one code
        byte = wq[0, b * 18 + 2 + (j & 15)]
        lo, hi = byte & 15, byte >> 4
        if j < 16:
            lo = lo + 1 if lo < 15 else lo - 1
        else:
            hi = hi + 1 if hi < 15 else hi - 1
        wq[0, b * 18 + 2 + (j & 15)] = np.uint8(lo | (hi << 4))
    else:                                                 # one q8_0 element's sign flipped
        v = int(xq[0, b * 34 + 2 + j].astype(np.int8))
        xq[0, b * 34 + 2 + j] = np.array(-v if v != -128 else 127, np.int8).view(np.uint8)
    return wq, xq


@pytest.mark.parametrize("kind,K", [("q8_lsb", 1024), ("nibble", 4544), ("sign", 4096)])
def test_old_bound_accepts_what_the_new_checks_reject(kind, K):
    """A correct y (the oracle's) against a corrupted reference: check_y at (1e-3, 1e-6) accepts the corrupted
    reference, check_y_terms rejects it; and on the order-free case of the same K the same corruption changes
    float32(y64), so the equality rejects it.  No kernel is mutated: the gap is in the bound.

    The corrupted element is not arbitrary: the old bound is loose by 1e-3 |y|, so it hides a corruption only where
    |delta y| <= 1e-3 |y| on every row the element touches (an element with a small |q| * |w| on rows that do not
    cancel).  The test walks the elements of token 0 / row 0 in order (fixed seed, M = 4) and takes the first that the
    old bound accepts and that changes y at all; it asserts that one exists."""
    M, N = 4, 1
    g = C.gaussian_case(O, K, M, N, seed=K)
    y = O.mul_mat(g["wq"], K, g["x"], nthreads=1)
    nb = K // QK
    check_y(y, g["y64"], g["s_abs"], 1e-3, 1e-6)
    check_y_terms(y, g["y64"], g["s_abs"], nb)
    found = None
    for b in range(nb):
        for j in range(QK):
            wq2, xq2 = _corrupt(kind, g["wq"], g["xq"], K, (b, j))
            y2, s2 = block_terms(wq2, xq2, K)
            if np.array_equal(y2, g["y64"]):
                continue                                   # w = 0 or q = 0 there: y unchanged
            try:
                check_y(y, y2, s2, 1e-3, 1e-6)
            except AssertionError:
                continue
            found = (b, j, y2, s2)
            break
        if found:
            break
    assert found, "no element whose corruption the old bound accepts"
    b, j, y2, s2 = found
    with pytest.raises(AssertionError):
        check_y_terms(y, y2, s2, nb)
    # the same corruption, same element, on the order-free case: an exact y no longer equals the reference
    c = C.order_free(K, M, N, seed=7)
    wq3, xq3 = _corrupt(kind, c["wq"], c["xq"], K, (b, j))
    y3, _ = block_terms(wq3, xq3, K)
    exact = c["y64"].astype(np.float32)
    assert_equal_values(exact, c["y64"])
    if np.array_equal(y3, c["y64"]):                       # this element is w = 0 / q = 0 on the order-free case
        pytest.fail("the corrupted element does not change the order-free y64; choose another seed")
    with pytest.raises(AssertionError):
        assert_equal_values(exact, y3)


def test_check_y_terms_edges():
    """S_abs = 0 admits only err = 0; a NaN is out of bound; the need is returned in units of 2^-24 * S_abs."""
    y64 = np.array([[0.0, 1.0]])
    s = np.array([[0.0, 2.0]])
    assert check_y_terms(np.array([[0.0, 1.0]], np.float32), y64, s, 4) == 0.0
    assert check_y_terms(np.array([[-0.0, 1.0 + 2.0 ** -22]], np.float32), y64, s, 4) == pytest.approx(2.0)
    for bad in ([[1e-30, 1.0]], [[0.0, np.nan]], [[0.0, 1.0 + 2.0 ** -20]]):
        with pytest.raises(AssertionError):
            check_y_terms(np.array(bad, np.float32), y64, s, 4)
    assert_equal_values(np.array([[-0.0, 1.0]], np.float32), y64)
    with pytest.raises(AssertionError):
        assert_equal_values(np.array([[0.0, 1.0 + 2.0 ** -23]], np.float32), y64)
