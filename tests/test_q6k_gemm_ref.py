"""CPU-side checks of the Q6_K prefill GEMM's arithmetic (tests/q6k_gemm_ref.py) and of the auto rule of
ggml_hip_mul_mat_q6_K (ggml_hip_debug_q6k_auto_algo, no device needed)."""
import os

import numpy as np
import pytest

import q6k_gemm_ref as G
import q6k_ref as R
from hip_env import LIB_PATH, ggml_hip
from parity import check_y

needs_lib = pytest.mark.skipif(not os.path.exists(LIB_PATH), reason="libggml_hip.so not built")


def check_digits(wq, K):
    w = G.scaled_weights(wq, K)
    hi, lo = G.digits(wq, K)
    assert np.array_equal(128 * hi + lo, w)
    assert lo.min() >= -64 and lo.max() <= 63
    assert hi.min() >= -32 and hi.max() <= 32
    assert w.min() >= -4064 and w.max() <= 4096
    return w, hi, lo


@pytest.mark.parametrize("K,M", [(256, 64), (2304, 9)])
def test_digit_split_random(K, M):
    check_digits(R.random_q6_K(np.random.default_rng([0x6C, K, M]), M, K), K)


def test_digit_split_extremes():
    """scale bytes 0x80 and 0x7F against the 6-bit values 0 and 63: all four corners of w'."""
    q6 = np.zeros((4, 1, 256), np.uint8)
    sc = np.zeros((4, 1, 16), np.int8)
    for r, (s, v) in enumerate([(-128, 0), (-128, 63), (127, 0), (127, 63)]):
        q6[r], sc[r] = v, s
    wq = G.pack_q6_K(q6, sc, np.full((4, 1), 0.01, np.float16))
    _, s2, q2 = R.split_q6_K(wq, 256)                       # pack_q6_K is split_q6_K's inverse
    assert np.array_equal(s2, sc) and np.array_equal(q2, q6.astype(np.int16) - 32)
    w, hi, lo = check_digits(wq, 256)
    assert [int(w[r, 0, 0]) for r in range(4)] == [4096, -3968, -4064, 3937]
    assert int(hi[0, 0, 0]) == 32 and int(lo[0, 0, 0]) == 0
    assert int(hi[2, 0, 0]) == -32 and int(lo[2, 0, 0]) == 32


def test_pack_q6_K_round_trip():
    rng = np.random.default_rng([0x6C, 3])
    q6 = rng.integers(0, 64, size=(5, 3, 256), dtype=np.uint8)
    sc = rng.integers(-128, 128, size=(5, 3, 16)).astype(np.int8)
    d = (rng.standard_normal((5, 3)) * 0.01).astype(np.float16)
    dw, s2, q2 = R.split_q6_K(G.pack_q6_K(q6, sc, d), 768)
    assert np.array_equal(s2, sc) and np.array_equal(q2, q6.astype(np.int16) - 32)
    assert np.array_equal(dw, d.astype(np.float32))


@pytest.mark.parametrize("K", [256, 2304])
def test_gemv_order_within_parity_bound(K):
    rng = np.random.default_rng([0x6C, 4, K])
    wq = R.random_q6_K(rng, 19, K)
    xq = R.quantize_q8_K(rng.standard_normal((3, K)).astype(np.float32))
    y_ref, s_abs = R.block_terms(wq, xq, K)
    check_y(G.gemv_order(wq, xq, K), y_ref, s_abs)


@pytest.fixture
def lib():
    L = ggml_hip.load()
    exact, min_n = L.ggml_hip_get_exact(), L.ggml_hip_debug_set_q6k_gemm_min_n(-1)
    env = os.environ.pop("GGML_HIP_Q6K_GEMM_MIN_N", None)
    L.ggml_hip_set_exact(0)
    yield L
    os.environ.pop("GGML_HIP_Q6K_GEMM_MIN_N", None)
    if env is not None:
        os.environ["GGML_HIP_Q6K_GEMM_MIN_N"] = env
    L.ggml_hip_debug_set_q6k_gemm_min_n(min_n)
    L.ggml_hip_set_exact(exact)


@needs_lib
def test_auto_algo_rule(lib):
    auto = lib.ggml_hip_debug_q6k_auto_algo
    lib.ggml_hip_debug_set_q6k_gemm_min_n(-1)
    min_n = lib.ggml_hip_debug_set_q6k_gemm_min_n(-1)       # the default (no environment value)
    assert min_n >= 9
    for N in (1, 8):
        assert auto(4096, 32000, N) == 1
    assert auto(4096, 32000, min_n - 1) == 1
    for N in (min_n, min_n + 1, 512):
        assert auto(4096, 32000, N) == 5
    assert auto(16384, 5, 1) == 1
    assert auto(16640, 5, 1) == 5                           # the GEMV stops at K = 16384
    lib.ggml_hip_set_exact(1)
    for K, N in ((4096, 1), (4096, 512), (16640, 1)):
        assert auto(K, 100, N) == 4
    lib.ggml_hip_set_exact(0)
    assert auto(384, 4, 1) == ggml_hip.ERR_INVALID


@needs_lib
def test_min_n_setter_and_environment(lib):
    auto, setter = lib.ggml_hip_debug_q6k_auto_algo, lib.ggml_hip_debug_set_q6k_gemm_min_n
    default = setter(100)
    assert setter(100) == 100                               # returns the previous value
    assert auto(4096, 64, 99) == 1 and auto(4096, 64, 100) == 5
    assert setter(3) == 100 and setter(-1) == 9             # never below 9
    assert setter(-1) == default
    os.environ["GGML_HIP_Q6K_GEMM_MIN_N"] = "77"
    setter(-1)                                              # re-reads the environment
    assert setter(-1) == 77
    assert auto(4096, 64, 76) == 1 and auto(4096, 64, 77) == 5
    del os.environ["GGML_HIP_Q6K_GEMM_MIN_N"]
    setter(-1)
    assert setter(-1) == default
