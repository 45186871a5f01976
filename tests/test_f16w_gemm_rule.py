"""The auto rule of ggml_hip_mul_mat_f16 with the weight-shaped prefill GEMM (algo 11, csrc/f16_w_gemm.hip) in it,
through ggml_hip_debug_f16w_auto_algo: no device needed.  Exact mode -> 4; N from GGML_HIP_F16W_WGEMM_MIN_N (default
never) -> 11 at any K; else the rule as it was (1 / 9 / 4).  The threshold's setter has the semantics of the other
types'; the plan rule is a pure function of the shape (256 CUs where no device is initialised)."""
import os
import re
import subprocess

import pytest

import f16w_gemm_cases as C
from hip_env import LIB_PATH, PKG, ROOT, ggml_hip

ENV = "GGML_HIP_F16W_WGEMM_MIN_N"
NEVER = 2 ** 31 - 1


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(LIB_PATH):
        subprocess.check_call(["make", "-s", "-C", PKG, "-j4"])
    return ggml_hip.load()


@pytest.fixture
def lib(built):
    """exact mode off, both F16 thresholds at their defaults, no environment value; what was found is put back"""
    L = built
    exact = L.ggml_hip_get_exact()
    wmin, gmin = L.ggml_hip_debug_set_f16w_wgemm_min_n(-1), L.ggml_hip_debug_set_f16w_gemm_min_n(-1)
    plan = L.ggml_hip_debug_set_f16w_wgemm_plan(0)
    env = {k: os.environ.pop(k, None) for k in (ENV, "GGML_HIP_F16W_GEMM_MIN_N")}
    L.ggml_hip_debug_set_f16w_wgemm_min_n(-1)
    L.ggml_hip_debug_set_f16w_gemm_min_n(-1)
    L.ggml_hip_set_exact(0)
    yield L
    for k, v in env.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v
    L.ggml_hip_debug_set_f16w_wgemm_min_n(wmin)
    L.ggml_hip_debug_set_f16w_gemm_min_n(gmin)
    L.ggml_hip_debug_set_f16w_wgemm_plan(plan)
    L.ggml_hip_set_exact(exact)


def test_default_is_never_and_the_answers_are_unchanged(lib):
    auto, setter = lib.ggml_hip_debug_f16w_auto_algo, lib.ggml_hip_debug_set_f16w_wgemm_min_n
    assert setter(-1) == NEVER
    assert auto(1504, 65, 17) == 1 and auto(32, 130, 40) == 9 and auto(65568, 1, 1) == 4
    for K in (32, 4096, 11008, 65536):
        for N in (1, 8, 9, 31):
            assert auto(K, 4096, N) == 1
        for N in (32, 512, 100000):
            assert auto(K, 4096, N) == 9
    for N in (1, 32, 512):
        assert auto(65568, 64, N) == 4
    assert auto(48, 4, 1) == ggml_hip.ERR_INVALID and auto(4096, 0, 1) == ggml_hip.ERR_INVALID


def test_threshold_takes_the_gemm_at_any_k(lib):
    auto, setter = lib.ggml_hip_debug_f16w_auto_algo, lib.ggml_hip_debug_set_f16w_wgemm_min_n
    assert setter(12) == NEVER
    assert auto(4096, 4096, 11) == 1 and auto(4096, 4096, 12) == 11 and auto(4096, 4096, 40) == 11
    assert auto(32, 130, 40) == 11 and auto(32, 1, 512) == 11
    assert auto(65568, 64, 12) == 11 and auto(65568, 64, 8) == 4       # no LDS-bound K limit; below it the rule as it was
    lib.ggml_hip_set_exact(1)
    for K, N in ((4096, 1), (4096, 12), (4096, 512), (65568, 40)):
        assert auto(K, 100, N) == 4
    lib.ggml_hip_set_exact(0)
    # a shape whose narrowest tiles exceed one grid: auto keeps the rule as it was
    assert auto(32, 2 ** 31 - 64, 2 ** 20) == 9
    assert setter(-1) == 12
    assert setter(-1) == NEVER
    assert auto(4096, 4096, 40) == 9 and auto(4096, 4096, 12) == 1


def test_setter_semantics_and_environment(lib):
    auto, setter = lib.ggml_hip_debug_f16w_auto_algo, lib.ggml_hip_debug_set_f16w_wgemm_min_n
    default = setter(100)
    assert default == NEVER and setter(100) == 100                     # returns the previous value
    assert auto(4096, 64, 99) == 9 and auto(4096, 64, 100) == 11
    assert setter(3) == 100 and setter(-1) == 9                        # never below 9
    assert setter(0) == default and setter(-1) == 9
    assert setter(-1) == default
    os.environ[ENV] = "77"
    setter(-1)                                                         # re-reads the environment
    assert setter(-1) == 77
    assert auto(4096, 64, 76) == 9 and auto(4096, 64, 77) == 11
    del os.environ[ENV]
    setter(-1)
    assert setter(-1) == default
    # the other F16 threshold is untouched by this one and still rules below it
    assert lib.ggml_hip_debug_set_f16w_gemm_min_n(-1) == 32
    setter(64)
    assert auto(4096, 64, 31) == 1 and auto(4096, 64, 32) == 9 and auto(4096, 64, 64) == 11


def test_plan_rule_and_pin(lib):
    """without a device the rule assumes 256 CUs; the pin is returned by its setter and does not change what the rule
    reports"""
    plan, pin = lib.ggml_hip_debug_f16w_wgemm_plan, lib.ggml_hip_debug_set_f16w_wgemm_plan
    if ggml_hip.device_count() == 0:
        for K, M, N, p in C.PLAN_CASES:
            assert plan(K, M, N) == p, (K, M, N)
        assert plan(4096, 4096, 9) == 1 and plan(4096, 4096, 64) == 1 and plan(4096, 4096, 128) == 1
        assert plan(4096, 4096, 256) == 2 and plan(4096, 4096, 512) == 2
        assert plan(4096, 11008, 64) == 1 and plan(4096, 11008, 128) == 2 and plan(4096, 11008, 512) == 3
        assert plan(4096, 32000, 9) == 3 and plan(4096, 32000, 128) == 3 and plan(4096, 32000, 512) == 3
    for K, M, N in ((32, 1, 1), (4096, 4096, 512), (11008, 4096, 64)):
        assert 1 <= plan(K, M, N) <= 3
        assert plan(K, M, N) == plan(K + 32, M, N)                      # no function of K
    assert pin(2) == 0 and pin(3) == 2
    assert plan(4096, 4096, 9) == 1                                    # what auto would take, whatever is pinned
    assert pin(0) == 3
    assert pin(4) == ggml_hip.ERR_INVALID and pin(-1) == ggml_hip.ERR_INVALID and pin(0) == 0
    assert plan(48, 4, 1) == ggml_hip.ERR_INVALID and plan(64, 0, 1) == ggml_hip.ERR_INVALID


def test_algo_10_is_still_refused_first(built):
    assert built.ggml_hip_mul_mat_f16(None, 0, 0, None, 0, None, 0, 10, None) == ggml_hip.ERR_INVALID
    assert b"algo" in built.ggml_hip_last_error()
    assert built.ggml_hip_mul_mat_f16(None, 0, 0, None, 0, None, 0, 11, None) == ggml_hip.ERR_INVALID
    assert b"algo" not in built.ggml_hip_last_error()                   # 11 is an algo: the null pointer is what is wrong


NEW_SYMBOLS = ("ggml_hip_debug_set_f16w_wgemm_min_n", "ggml_hip_debug_set_f16w_wgemm_plan",
               "ggml_hip_debug_f16w_wgemm_plan")


def test_new_symbols_in_header_and_binding(built):
    header = open(os.path.join(ROOT, "include", "ggml-hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert getattr(built, name).argtypes is not None, name
