"""CPU checks of the Q4_1 / Q5_1 prefill GEMM (algo 7): its numpy restatement (tests/q5x_gemm_ref.chain) stays within
the project's parity bound of the fixtures the compiled reference wrote, of the exact value on mean-shifted
activations and on full-range blocks; the rule behind algo 0 with the types' own threshold (no device needed); the new
entry point is in the header and in the binding."""
import os
import re
import subprocess

import numpy as np
import pytest

import q5x_gemm_ref as G
import q5x_ref as R
from golden_io import load
from hip_env import LIB_PATH, PKG, ROOT, ggml_hip
from parity import check_y

TYPES = ("q41", "q51")
NAME = {"q41": "q4_1", "q51": "q5_1"}
ENV = "GGML_HIP_Q41_Q51_GEMM_MIN_N"
GEMV, EXACT, GEMM = 1, 4, 7


# ---- the restatement against the bound ----------------------------------------------------------------------

@pytest.mark.parametrize("K", [64, 2304, 4160])
@pytest.mark.parametrize("t", TYPES)
def test_chain_within_bound_of_fixture(t, K):
    wq, xq, y = load(t, f"w{K}_q"), load(t, f"x{K}_q"), load(t, f"y{K}_vec_dot")
    _, s_abs = R.block_terms(t, wq, xq, K)
    check_y(G.chain(t, wq, xq, K), y, s_abs, rtol=1e-3, atol_blocks=1e-6)


@pytest.mark.parametrize("t", TYPES)
def test_chain_mean_shifted_activations_against_exact_value(t):
    """x ~ N(1, 1): the d * isum and m * s sums are large and opposite; the chain keeps a block's two terms adjacent."""
    K, M, N = 4096, 33, 8
    rng = np.random.default_rng([0x57, 1, R.TYPES[t][0]])
    wq = R.quantize_w(t, (rng.standard_normal((M, K)) * 0.02).astype(np.float32))
    xq = R.quantize_x(t, (rng.standard_normal((N, K)) + 1.0).astype(np.float32))
    y_exact, s_abs = R.block_terms(t, wq, xq, K)
    check_y(G.chain(t, wq, xq, K), y_exact, s_abs, rtol=1e-3, atol_blocks=1e-6)


@pytest.mark.parametrize("t", TYPES)
def test_chain_full_range_blocks(t):
    """random_blocks (every nibble and qh pattern, d and m of both signs over a wide exponent range, the specials) and
    x rows at +-amax (every q8 = +-127): against the reference's AVX2 order and against the exact value."""
    K, M, N = 4160, 33, 5
    rng = np.random.default_rng([0x57, 2, R.TYPES[t][0]])
    wq = R.random_blocks(rng, M, K, R.has_qh(t), True)
    x = rng.standard_normal((N, K)).astype(np.float32)
    x[0], x[1, ::2], x[1, 1::2] = 2.0, 2.0, -2.0
    xq = R.quantize_x(t, x)
    y_exact, s_abs = R.block_terms(t, wq, xq, K)
    y = G.chain(t, wq, xq, K)
    check_y(y, R.vec_dot_avx2(t, wq, xq, K), s_abs, rtol=1e-3, atol_blocks=1e-6)
    check_y(y, y_exact, s_abs, rtol=1e-3, atol_blocks=1e-6)


def test_chain_is_the_stated_recurrence():
    """one block pair by hand, in Python floats rounded at every step the schedule rounds"""
    t, K = "q51", 64
    wq, xq = load(t, "craft_q"), load(t, "craft_x_q")
    dw, mw, dx, sx, lanes = R._lane_sums(t, wq, xq, K)
    y = G.chain(t, wq, xq, K)
    f = np.float32
    for n in range(dx.shape[0]):
        for m in range(dw.shape[0]):
            acc = f(0)
            for b in range(2):
                d = f(dw[m, b] * dx[n, b])
                acc = G.fmaf32(np.array([f(lanes[n, m, b].sum())]), np.array([d]), np.array([acc]))[0]
                acc = G.fmaf32(np.array([mw[m, b]]), np.array([sx[n, b]]), np.array([acc]))[0]
            assert acc.view(np.uint32) == y[n, m].view(np.uint32)


# ---- the auto rule ------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def built():
    if not os.path.exists(LIB_PATH):
        subprocess.check_call(["make", "-s", "-C", PKG, "-j4"])
    return ggml_hip.load()


@pytest.fixture
def lib(built):
    L = built
    exact, min_n = L.ggml_hip_get_exact(), L.ggml_hip_debug_set_q41_q51_gemm_min_n(-1)
    env = os.environ.pop(ENV, None)
    L.ggml_hip_set_exact(0)
    yield L
    os.environ.pop(ENV, None)
    if env is not None:
        os.environ[ENV] = env
    L.ggml_hip_debug_set_q41_q51_gemm_min_n(min_n)
    L.ggml_hip_set_exact(exact)


@pytest.mark.parametrize("t", TYPES)
def test_auto_algo_rule(lib, t):
    auto, setter = getattr(lib, f"ggml_hip_debug_{NAME[t]}_auto_algo"), lib.ggml_hip_debug_set_q41_q51_gemm_min_n
    setter(-1)
    assert setter(-1) == 2 ** 31 - 1                         # the default (no environment value): never
    for N in (1, 8, 32, 512):
        assert auto(4096, 4096, N) == GEMV
    setter(9)
    assert auto(4096, 4096, 8) == GEMV
    for N in (9, 512):
        assert auto(4096, 4096, N) == GEMM
    assert auto(52480, 4, 512) == EXACT                      # past the GEMV's K: the exact kernel still
    lib.ggml_hip_set_exact(1)
    for N in (1, 9, 512):
        assert auto(4096, 4096, N) == EXACT
    lib.ggml_hip_set_exact(0)
    assert auto(4096, 4096, 512) == GEMM
    for N in (1, 9, 512, 100000):                            # Q5_0's auto never returns 7
        assert lib.ggml_hip_debug_q5_0_auto_algo(4096, 4096, N) in (1, 2)


def test_min_n_setter_and_environment(lib):
    setter = lib.ggml_hip_debug_set_q41_q51_gemm_min_n
    auto41, auto51 = lib.ggml_hip_debug_q4_1_auto_algo, lib.ggml_hip_debug_q5_1_auto_algo
    default = setter(100)
    assert default == 2 ** 31 - 1
    assert setter(100) == 100                                # returns the previous value
    for auto in (auto41, auto51):                            # one threshold for both types
        assert auto(4096, 64, 99) == GEMV and auto(4096, 64, 100) == GEMM
    assert setter(3) == 100 and setter(-1) == 9              # 3 counts as 9
    assert setter(-1) == default
    os.environ[ENV] = "77"
    setter(-1)                                               # the environment variable is read after set(-1)
    assert setter(-1) == 77
    assert auto51(4096, 64, 76) == GEMV and auto51(4096, 64, 77) == GEMM
    del os.environ[ENV]
    setter(-1)
    assert setter(-1) == default


def test_thresholds_do_not_move_each_other(lib):
    setter = lib.ggml_hip_debug_set_q41_q51_gemm_min_n
    q50, q8 = lib.ggml_hip_debug_set_q5_0_gemm_min_n, lib.ggml_hip_debug_set_q8_0_gemm_min_n
    q50_was, q8_was = q50(-1), q8(-1)
    q50_dflt, q8_dflt = q50(-1), q8(-1)
    try:
        setter(50)
        assert q50(-1) == q50_dflt and q8(-1) == q8_dflt
        assert lib.ggml_hip_debug_q5_0_auto_algo(4096, 64, 50) == (2 if q50_dflt <= 50 else 1)
        q50(200)
        q8(300)
        assert setter(50) == 50
        assert lib.ggml_hip_debug_q5_1_auto_algo(4096, 64, 50) == GEMM
        assert lib.ggml_hip_debug_q5_0_auto_algo(4096, 64, 199) == 1
    finally:
        q50(q50_was)
        q8(q8_was)


# ---- symbols ------------------------------------------------------------------------------------------------

def test_new_symbol_in_header_and_binding(built):
    header = open(os.path.join(ROOT, "include", "ggml-hip.h")).read()
    name = "ggml_hip_debug_set_q41_q51_gemm_min_n"
    assert re.search(r"\bint %s\(int n\);" % name, header)
    fn = getattr(built, name)
    assert fn.argtypes is not None and len(fn.argtypes) == 1         # bound with a signature (and exported)
    assert ENV in header
