"""CPU checks of the F16-weight path (csrc/f16_w.hip, the ROW_F16 row of ggml-hip-core.cpp): the numpy restatement of
the GEMV's order (tests/f16w_ref.py) is within the fp32-accumulation bound of the float64 sum of the fp16 products,
it differs from ggml_vec_dot_f16's AVX order on the very inputs of tests/test_gpu_f16w.py (so a bitwise match on the
device cannot come from the old kernel), and the auto rule (exact mode, a K past the GEMV, the threshold and its
setter), none of which needs a device."""
import os
import re
import subprocess

import numpy as np
import pytest

import f16w_ref as R
import ggml_ops_ref as G
from hip_env import LIB_PATH, PKG, ROOT, ggml_hip

IDS = ["K%d_M%d_N%d%s" % (c[0], c[1], c[2], "_special" if c[4] else "") for c in R.CASES]


@pytest.mark.parametrize("i", range(len(R.CASES)), ids=IDS)
def test_restatement_within_fp32_bound_of_float64(i):
    """|y - ref| <= 1e-5 * sum|w * fp16(x)| + 1e-30, the bound tests/test_gpu_f16_mul_mat.py uses for F16 x F32"""
    w16, x, y = R.case(i)
    ref, sab = R.exact_terms(w16, x)
    assert np.isfinite(y).all()
    err = np.abs(y.astype(np.float64) - ref)
    print(R.CASES[i], "max err / S_abs", float((err / (sab + 1e-30)).max()))
    assert (err <= 1e-5 * sab + 1e-30).all()


@pytest.mark.parametrize("i", range(1, len(R.CASES)), ids=IDS[1:])
def test_restatement_differs_from_vec_dot_f16(i):
    """(case 0, one output of 32 elements, is the one where the two orders happen to coincide)"""
    w16, x, y = R.case(i)
    old = G.mul_mat_f16_f32(w16, x)
    assert old.shape == y.shape
    assert (G.bits(old) != G.bits(y)).any()


def test_restatement_properties():
    """a column's y does not depend on the columns beside it or on the rows beside its row; a zero row gives +0; a
    lane past K (K = 32: lanes 4 .. 63) adds nothing, whatever x holds there"""
    w16, x, y = R.case(6)                                    # K = 1504, M = 65, N = 17
    assert np.array_equal(G.bits(R.gemv_schedule(w16, x[3:4])), G.bits(y[3:4]))
    assert np.array_equal(G.bits(R.gemv_schedule(w16[10:12], x)), G.bits(y[:, 10:12]))
    z = R.gemv_schedule(np.zeros((2, 64), np.uint16), np.full((1, 64), -3.0, np.float32))
    assert np.array_equal(G.bits(z), np.zeros((1, 2), np.uint32))
    w = np.arange(1, 33, dtype=np.float16)[None, :]
    assert R.gemv_schedule(w, np.ones((1, 32), np.float32))[0, 0] == 32 * 33 / 2


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(LIB_PATH):
        subprocess.check_call(["make", "-s", "-C", PKG, "-j4"])
    return ggml_hip.load()


@pytest.fixture
def lib(built):
    L = built
    exact, min_n = L.ggml_hip_get_exact(), L.ggml_hip_debug_set_f16w_gemm_min_n(-1)
    env = os.environ.pop("GGML_HIP_F16W_GEMM_MIN_N", None)
    L.ggml_hip_set_exact(0)
    yield L
    os.environ.pop("GGML_HIP_F16W_GEMM_MIN_N", None)
    if env is not None:
        os.environ["GGML_HIP_F16W_GEMM_MIN_N"] = env
    L.ggml_hip_debug_set_f16w_gemm_min_n(min_n)
    L.ggml_hip_set_exact(exact)


def test_auto_algo_rule(lib):
    auto = lib.ggml_hip_debug_f16w_auto_algo
    lib.ggml_hip_debug_set_f16w_gemm_min_n(-1)
    min_n = lib.ggml_hip_debug_set_f16w_gemm_min_n(-1)      # the default (no environment value)
    assert min_n == 32
    for K in (32, 4096, 11008, 65536):
        for N in (1, 8, 9, min_n - 1):
            assert auto(K, 4096, N) == 1
        for N in (min_n, min_n + 1, 512):
            assert auto(K, 4096, N) == 9
    for N in (1, 31, 32, 512):                              # one column's fp16 image past the LDS: the exact kernels
        assert auto(65568, 64, N) == 4
    lib.ggml_hip_set_exact(1)
    for K, N in ((4096, 1), (4096, 512), (32, 9), (65568, 40)):
        assert auto(K, 100, N) == 4
    lib.ggml_hip_set_exact(0)
    assert auto(48, 4, 1) == ggml_hip.ERR_INVALID            # K % 32
    assert auto(4096, 0, 1) == ggml_hip.ERR_INVALID


def test_min_n_setter_and_environment(lib):
    auto, setter = lib.ggml_hip_debug_f16w_auto_algo, lib.ggml_hip_debug_set_f16w_gemm_min_n
    default = setter(100)
    assert setter(100) == 100                               # returns the previous value
    assert auto(4096, 64, 99) == 1 and auto(4096, 64, 100) == 9
    assert setter(3) == 100 and setter(-1) == 9             # never below 9
    assert setter(-1) == default
    os.environ["GGML_HIP_F16W_GEMM_MIN_N"] = "77"
    setter(-1)                                              # re-reads the environment
    assert setter(-1) == 77
    assert auto(4096, 64, 76) == 1 and auto(4096, 64, 77) == 9
    del os.environ["GGML_HIP_F16W_GEMM_MIN_N"]
    setter(-1)
    assert setter(-1) == default


def test_rejected_algo_is_refused_first(built):
    """an algo the type does not have is INVALID before any other argument is looked at, an empty call included"""
    for algo in (2, 3, 5, 6, 7, 8, 10, -1):
        assert built.ggml_hip_mul_mat_f16(None, 0, 0, None, 0, None, 0, algo, None) == ggml_hip.ERR_INVALID
        assert b"algo" in built.ggml_hip_last_error()


NEW_SYMBOLS = ("ggml_hip_mul_mat_f16", "ggml_hip_debug_f16w_auto_algo", "ggml_hip_debug_set_f16w_gemm_min_n")


def test_new_symbols_in_header_exports_and_binding(built):
    header = open(os.path.join(ROOT, "include", "ggml-hip.h")).read()
    exports = open(os.path.join(PKG, "exports.map")).read()
    assert re.search(r"global:\s*ggml_\*;", exports)        # every ggml_* name is exported, nothing else
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert getattr(built, name).argtypes is not None, name     # bound with a signature (and exported)
    assert ggml_hip.GGML_TYPE_F16 == 1 and callable(ggml_hip.mul_mat_f16)
    t = ggml_hip.make_tensor(ggml_hip.GGML_TYPE_F16, (64, 3))
    assert (t.nb[0], t.nb[1], t.nb[2]) == (2, 128, 384)
