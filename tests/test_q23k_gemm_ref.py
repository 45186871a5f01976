"""CPU-side checks of the Q3_K / Q2_K prefill GEMM's integer arithmetic (tests/q23k_gemm_ref.py), of the new entry
point's declaration, export and binding, and of the auto rule of ggml_hip_mul_mat_q3_K / _q2_K with the GEMM
threshold (ggml_hip_debug_q23k_auto_algo, ggml_hip_debug_set_q23k_gemm_min_n; no device needed)."""
import os
import re

import numpy as np
import pytest

import q23k_gemm_ref as G
import q23k_ref as R
from hip_env import LIB_PATH, PKG, ggml_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_lib = pytest.mark.skipif(not os.path.exists(LIB_PATH), reason="libggml_hip.so not built")
BOTH = pytest.mark.parametrize("q3", [True, False], ids=["q3k", "q2k"])
GTYPE = {True: ggml_hip.GGML_TYPE_Q3_K, False: ggml_hip.GGML_TYPE_Q2_K}
ENV = "GGML_HIP_Q23K_GEMM_MIN_N"
SETTER = "ggml_hip_debug_set_q23k_gemm_min_n"
GEMV, EXACT, GEMM = 1, 4, 8


@BOTH
def test_pack_q23_K_round_trip(q3):
    rng = np.random.default_rng([0x48, 1, q3])
    q = rng.integers(-4, 4, size=(5, 3, 16, 16)) if q3 else rng.integers(0, 4, size=(5, 3, 16, 16))
    sc = rng.integers(-32, 32, size=(5, 3, 16)) if q3 else rng.integers(0, 16, size=(5, 3, 16))
    m = np.zeros((5, 3, 16), np.int64) if q3 else rng.integers(0, 16, size=(5, 3, 16))
    d, dmin = (rng.standard_normal((2, 5, 3)) * 0.01).astype(np.float16)
    wq = G.pack_q23_K(q, sc, m, d, dmin, q3)
    assert wq.shape == (5, 3 * R.block_bytes(q3)) and wq.dtype == np.uint8
    dw, dm, s2, m2, q2 = R._split(wq, 768, q3)
    assert np.array_equal(s2, sc) and np.array_equal(m2, m) and np.array_equal(q2, q)
    assert np.array_equal(dw, d.astype(np.float32))
    assert np.array_equal(dm, np.zeros_like(dw) if q3 else dmin.astype(np.float32))


@BOTH
def test_split_pack_round_trip_on_random_bytes(q3):
    """any bytes form a valid block: split then pack gives the bytes back"""
    wq = R.random_q23_K(np.random.default_rng([0x48, 2, q3]), 7, 768, q3)
    d, dmin, sc, m, q = R._split(wq, 768, q3)
    nb = 3
    raw = wq.reshape(7, nb, -1)
    off = 108 if q3 else 80
    d16 = raw[:, :, off:off + 2].copy().view(np.float16)[:, :, 0]
    dm16 = d16 if q3 else raw[:, :, 82:84].copy().view(np.float16)[:, :, 0]
    assert np.array_equal(G.pack_q23_K(q, sc, m, d16, dm16, q3), wq)


@BOTH
@pytest.mark.parametrize("K,M", [(256, 64), (2304, 9)])
def test_scaled_weights_are_int8_random(q3, K, M):
    w = G.scaled_weights(R.random_q23_K(np.random.default_rng([0x48, 3, q3, K, M]), M, K, q3), K, q3)
    lo, hi = (-128, 124) if q3 else (0, 45)
    assert w.min() >= lo and w.max() <= hi


def test_scaled_weights_corners_q3k():
    """(sc, q) in {-32, 31} x {-4, 3}: sc q reaches +128, the negated product stays an int8 and reaches -128"""
    corners = [(-32, -4), (-32, 3), (31, -4), (31, 3)]
    q = np.zeros((4, 1, 16, 16), np.int64)
    sc = np.zeros((4, 1, 16), np.int64)
    for r, (s, v) in enumerate(corners):
        q[r], sc[r] = v, s
    wq = G.pack_q23_K(q, sc, None, np.full((4, 1), 0.01, np.float16), None, True)
    _, _, s2, _, q2 = R._split(wq, 256, True)
    assert np.array_equal(s2, sc) and np.array_equal(q2, q)
    assert int((s2[0, 0, 0] * q2[0, 0, 0, 0])) == 128                     # not an int8
    w = G.scaled_weights(wq, 256, True)
    assert [int(w[r, 0, 0, 0]) for r in range(4)] == [-128, 96, 124, -93]
    assert w.min() == -128 and w.max() == 124


def test_scaled_weights_corner_q2k():
    q = np.full((1, 1, 16, 16), 3)
    s = np.full((1, 1, 16), 15)
    wq = G.pack_q23_K(q, s, s, np.full((1, 1), 0.01, np.float16), np.full((1, 1), 0.02, np.float16), False)
    _, _, s2, m2, q2 = R._split(wq, 256, False)
    assert np.array_equal(s2, s) and np.array_equal(m2, s) and np.array_equal(q2, q)
    w = G.scaled_weights(wq, 256, False)
    assert np.all(w == 45)


def check_bsum_digits(x, K):
    xq = R.quantize_q8_K(np.asarray(x, np.float32))
    s = G.bsum16(xq, K)
    bh, bl = G.bsum_digits(xq, K)
    assert np.array_equal(128 * bh + bl, s)
    assert bl.min() >= 0 and bl.max() <= 127
    assert bh.min() >= -16 and bh.max() <= 15
    assert s.min() >= -2048 and s.max() <= 2032
    return s, bh, bl


def test_bsum_digits_range_ends():
    """q8_K gives the block's extreme element -128 whatever its sign (iscale = -128 / max), so an all-equal block,
    positive or negative, is all -128: bsum16 = -2048.  The other end, 16 * 127 = 2032, needs a sub-block of +128s
    clamped to 127: elements of the extreme's magnitude and the opposite sign, the extreme itself elsewhere."""
    for v in (1.0, -1.0):
        s, bh, bl = check_bsum_digits(np.full((1, 256), v), 256)
        assert np.all(s == -2048) and np.all(bh == -16) and np.all(bl == 0)
    for v in (1.0, -1.0):
        x = np.full((1, 256), v)
        x[0, 0] = -v                                           # the first element of largest |x| is the extreme
        s, bh, bl = check_bsum_digits(x, 256)
        assert s[0, 0, 0] == -128 + 15 * 127
        assert np.all(s[0, 0, 1:] == 2032) and np.all(bh[0, 0, 1:] == 15) and np.all(bl[0, 0, 1:] == 112)


@pytest.mark.parametrize("K", [256, 2304])
def test_bsum_digits_random(K):
    check_bsum_digits(np.random.default_rng([0x48, 5, K]).standard_normal((7, K)) * 3, K)


@BOTH
@pytest.mark.parametrize("K", [256, 768, 2304])
def test_sums_from_planes_equal_int_terms(q3, K):
    rng = np.random.default_rng([0x48, 6, q3, K])
    wq = R.random_q23_K(rng, 19, K, q3)
    x = rng.standard_normal((5, K)).astype(np.float32)
    x[1, :256], x[2, :256], x[3, :256] = 1.0, -1.0, 1.0
    x[3, 0] = -1.0                                             # bsum16 = 2032 in fifteen sub-blocks
    xq = R.quantize_q8_K(x)
    _, _, _, lanes, prod = R._int_terms(wq, xq, K, q3)
    isum, msum = G.sums_from_planes(wq, xq, K, q3)
    assert np.array_equal(isum, lanes.sum(axis=3)) and np.array_equal(msum, prod.sum(axis=3))
    if q3:
        assert not msum.any()


@pytest.fixture
def lib():
    L = ggml_hip.load()
    exact, min_n = L.ggml_hip_get_exact(), getattr(L, SETTER)(-1)
    env = os.environ.pop(ENV, None)
    L.ggml_hip_set_exact(0)
    yield L
    os.environ.pop(ENV, None)
    if env is not None:
        os.environ[ENV] = env
    getattr(L, SETTER)(min_n)
    L.ggml_hip_set_exact(exact)


@needs_lib
def test_new_symbol_in_header_exports_binding_and_makefile(lib):
    header = open(os.path.join(ROOT, "include", "ggml-hip.h")).read()
    assert re.search(r"\bint %s\(int n\);" % SETTER, header)
    assert re.search(r"global:\s*ggml_\*;", open(os.path.join(PKG, "exports.map")).read())
    assert getattr(lib, SETTER).argtypes is not None           # bound with a signature (and exported)
    assert callable(ggml_hip.debug_set_q23k_gemm_min_n)
    assert re.search(r"^KERNELS\s*=.*\bq23_k_gemm\b", open(os.path.join(PKG, "Makefile")).read(), re.M)
    assert os.path.exists(os.path.join(PKG, "csrc", "q23_k_gemm.hip"))


@needs_lib
@BOTH
def test_auto_algo_rule(lib, q3):
    t = GTYPE[q3]
    auto, setter = lib.ggml_hip_debug_q23k_auto_algo, getattr(lib, SETTER)
    setter(-1)
    assert setter(-1) == 2 ** 31 - 1                        # the default with no environment value: never
    for N in (1, 8, 9, 512, 1 << 20):
        assert auto(t, 4096, 4096, N) == GEMV
    setter(9)
    assert auto(t, 4096, 11008, 9) == GEMM and auto(t, 4096, 11008, 512) == GEMM
    assert auto(t, 4096, 11008, 8) == GEMV and auto(t, 4096, 11008, 1) == GEMV
    assert auto(t, 16384, 5, 9) == GEMM
    for N in (1, 9, 512):
        assert auto(t, 17920, 5, N) == EXACT                # the GEMV stops at K = 16384: the exact kernel, as before
    lib.ggml_hip_set_exact(1)
    for K, N in ((4096, 1), (4096, 512), (17920, 1), (17920, 512)):
        assert auto(t, K, 100, N) == EXACT
    lib.ggml_hip_set_exact(0)
    assert auto(t, 384, 4, 9) == ggml_hip.ERR_INVALID
    setter(-1)
    assert auto(t, 4096, 4096, 512) == GEMV


@needs_lib
def test_min_n_setter_and_environment(lib):
    auto, setter = lib.ggml_hip_debug_q23k_auto_algo, getattr(lib, SETTER)
    default = setter(100)
    assert default == 2 ** 31 - 1
    assert setter(100) == 100                               # returns the previous value
    for t in GTYPE.values():                                # one threshold for both types
        assert auto(t, 4096, 64, 99) == GEMV and auto(t, 4096, 64, 100) == GEMM
    assert setter(3) == 100 and setter(-1) == 9             # never below 9
    assert setter(-1) == default
    os.environ[ENV] = "77"
    setter(-1)                                              # re-reads the environment
    assert setter(-1) == 77
    assert ggml_hip.debug_set_q23k_gemm_min_n(-1) == 77
    t = GTYPE[True]
    assert auto(t, 4096, 64, 76) == GEMV and auto(t, 4096, 64, 77) == GEMM
    del os.environ[ENV]
    setter(-1)
    assert setter(-1) == default
    assert auto(t, 4096, 4096, 512) == GEMV
