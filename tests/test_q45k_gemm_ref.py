"""CPU-side checks of the Q5_K / Q4_K prefill GEMM's integer arithmetic (tests/q45k_gemm_ref.py) and of the auto rule
of ggml_hip_mul_mat_q5_K / _q4_K (ggml_hip_debug_q45k_auto_algo, no device needed)."""
import os

import numpy as np
import pytest

import q45k_gemm_ref as G
import q45k_ref as R
from hip_env import LIB_PATH, ggml_hip

needs_lib = pytest.mark.skipif(not os.path.exists(LIB_PATH), reason="libggml_hip.so not built")
BOTH = pytest.mark.parametrize("qh", [True, False], ids=["q5k", "q4k"])
GTYPE = {True: ggml_hip.GGML_TYPE_Q5_K, False: ggml_hip.GGML_TYPE_Q4_K}
ENV = "GGML_HIP_Q45K_GEMM_MIN_N"


def check_digits(wq, K, qh):
    w = G.scaled_weights(wq, K, qh)
    hi, lo = G.digits(wq, K, qh)
    assert np.array_equal(128 * hi + lo, w)
    assert lo.min() >= 0 and lo.max() <= 127
    assert hi.min() >= 0 and hi.max() <= 15
    assert w.min() >= 0 and w.max() <= 63 * G.Q_MAX[qh]
    return w, hi, lo


@BOTH
@pytest.mark.parametrize("K,M", [(256, 64), (2304, 9)])
def test_digit_split_random(qh, K, M):
    check_digits(R.random_q45_K(np.random.default_rng([0x47, qh, K, M]), M, K, qh, special=True), K, qh)


@BOTH
def test_digit_split_corners(qh):
    """sc in {0, 63} x q in {0, max}: the four corners of w'."""
    qmax = G.Q_MAX[qh]
    corners = [(0, 0), (0, qmax), (63, 0), (63, qmax)]
    q = np.zeros((4, 1, 8, 32), np.int64)
    sc = np.zeros((4, 1, 8), np.int64)
    for r, (s, v) in enumerate(corners):
        q[r], sc[r] = v, s
    wq = G.pack_q45_K(q, sc, sc, np.full((4, 1), 0.01, np.float16), np.full((4, 1), 0.02, np.float16), qh)
    _, _, s2, m2, q2 = R.split_q45_K(wq, 256, qh)              # pack_q45_K is split_q45_K's inverse
    assert np.array_equal(s2, sc) and np.array_equal(m2, sc) and np.array_equal(q2, q)
    w, hi, lo = check_digits(wq, 256, qh)
    top = 63 * qmax
    assert [int(w[r, 0, 0, 0]) for r in range(4)] == [0, 0, 0, top]
    assert int(hi[3, 0, 0, 0]) == top >> 7 and int(lo[3, 0, 0, 0]) == top & 127
    assert int(hi.max()) == (15 if qh else 7)


@BOTH
def test_pack_q45_K_round_trip(qh):
    rng = np.random.default_rng([0x47, 3, qh])
    q = rng.integers(0, G.Q_MAX[qh] + 1, size=(5, 3, 8, 32))
    sc, m = rng.integers(0, 64, size=(5, 3, 8)), rng.integers(0, 64, size=(5, 3, 8))
    d, dmin = (rng.standard_normal((2, 5, 3)) * 0.01).astype(np.float16)
    dw, dm, s2, m2, q2 = R.split_q45_K(G.pack_q45_K(q, sc, m, d, dmin, qh), 768, qh)
    assert np.array_equal(s2, sc) and np.array_equal(m2, m) and np.array_equal(q2, q)
    assert np.array_equal(dw, d.astype(np.float32)) and np.array_equal(dm, dmin.astype(np.float32))


def check_bsum_digits(x, K, lo=-4096, hi=4064):
    xq = R.quantize_q8_K(np.asarray(x, np.float32))
    s = G.bsum32(xq, K)
    bh, bl = G.bsum_digits(xq, K)
    assert np.array_equal(128 * bh + bl, s)
    assert bl.min() >= 0 and bl.max() <= 127
    assert bh.min() >= -32 and bh.max() <= 31
    assert s.min() >= lo and s.max() <= hi
    return s, bh, bl


def test_bsum_digits_range_ends():
    """q8_K gives the block's extreme element -128 whatever its sign (iscale = -128 / max), so an all-equal block,
    positive or negative, is all -128: bsum32 = -4096.  The other end, 32 * 127 = 4064, needs a sub-block of +128s
    clamped to 127: elements of the extreme's magnitude and the opposite sign, the extreme itself elsewhere."""
    for v in (1.0, -1.0):
        s, bh, bl = check_bsum_digits(np.full((1, 256), v), 256)
        assert np.all(s == -4096) and np.all(bh == -32) and np.all(bl == 0)
    for v in (1.0, -1.0):
        x = np.full((1, 256), v)
        x[0, 0] = -v                                           # the first element of largest |x| is the extreme
        s, bh, bl = check_bsum_digits(x, 256)
        assert s[0, 0, 0] == -128 + 31 * 127
        assert np.all(s[0, 0, 1:] == 4064) and np.all(bh[0, 0, 1:] == 31) and np.all(bl[0, 0, 1:] == 96)


@pytest.mark.parametrize("K", [256, 2304])
def test_bsum_digits_random(K):
    rng = np.random.default_rng([0x47, 5, K])
    check_bsum_digits(rng.standard_normal((7, K)) * 3, K)


@BOTH
@pytest.mark.parametrize("K", [256, 768])
def test_sums_from_digits_equal_int_terms(qh, K):
    rng = np.random.default_rng([0x47, 6, qh, K])
    wq = R.random_q45_K(rng, 19, K, qh)
    x = rng.standard_normal((5, K)).astype(np.float32)
    x[1, :256], x[2, :256], x[3, :256] = 1.0, -1.0, 1.0
    x[3, 0] = -1.0                                             # bsum32 = 4064 in seven sub-blocks
    xq = R.quantize_q8_K(x)
    _, _, _, lanes, prod = R._int_terms(wq, xq, K, qh)
    isum, msum = G.sums_from_digits(wq, xq, K, qh)
    assert np.array_equal(isum, lanes.sum(axis=3)) and np.array_equal(msum, prod.sum(axis=3))


@pytest.fixture
def lib():
    L = ggml_hip.load()
    exact, min_n = L.ggml_hip_get_exact(), L.ggml_hip_debug_set_q45k_gemm_min_n(-1)
    env = os.environ.pop(ENV, None)
    L.ggml_hip_set_exact(0)
    yield L
    os.environ.pop(ENV, None)
    if env is not None:
        os.environ[ENV] = env
    L.ggml_hip_debug_set_q45k_gemm_min_n(min_n)
    L.ggml_hip_set_exact(exact)


@needs_lib
@BOTH
def test_auto_algo_rule(lib, qh):
    t = GTYPE[qh]
    auto = lib.ggml_hip_debug_q45k_auto_algo
    lib.ggml_hip_debug_set_q45k_gemm_min_n(-1)
    min_n = lib.ggml_hip_debug_set_q45k_gemm_min_n(-1)      # the default (no environment value)
    assert min_n >= 9
    for N in (1, 8):
        assert auto(t, 4096, 11008, N) == 1
    assert auto(t, 4096, 11008, min_n - 1) == 1
    for N in (min_n, min_n + 1):
        assert auto(t, 4096, 11008, N) == 6
    assert auto(t, 16384, 5, 1) == 1
    for N in (1, min_n, 512):
        assert auto(t, 16640, 5, N) == 4                    # the GEMV stops at K = 16384: the exact kernel, as before
    lib.ggml_hip_set_exact(1)
    for K, N in ((4096, 1), (4096, 512), (16640, 1), (16640, 512)):
        assert auto(t, K, 100, N) == 4
    lib.ggml_hip_set_exact(0)
    assert auto(t, 384, 4, 1) == ggml_hip.ERR_INVALID
    assert auto(ggml_hip.GGML_TYPE_Q4_0, 4096, 4, 1) == ggml_hip.ERR_INVALID


@needs_lib
def test_min_n_setter_and_environment(lib):
    auto, setter = lib.ggml_hip_debug_q45k_auto_algo, lib.ggml_hip_debug_set_q45k_gemm_min_n
    default = setter(100)
    assert setter(100) == 100                               # returns the previous value
    for t in GTYPE.values():                                # one threshold for both types
        assert auto(t, 4096, 64, 99) == 1 and auto(t, 4096, 64, 100) == 6
    assert setter(3) == 100 and setter(-1) == 9             # never below 9
    assert setter(-1) == default
    os.environ[ENV] = "77"
    setter(-1)                                              # re-reads the environment
    assert setter(-1) == 77
    t = GTYPE[True]
    assert auto(t, 4096, 64, 76) == 1 and auto(t, 4096, 64, 77) == 6
    del os.environ[ENV]
    setter(-1)
    assert setter(-1) == default
