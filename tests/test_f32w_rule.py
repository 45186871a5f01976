"""The F32 row's rules, none of which needs a device (csrc/ggml-hip-core.cpp ROW_F32, csrc/f32_w_gemm.hip): what algo 0
of ggml_hip_mul_mat_f32 runs (exact mode, a K past the GEMV, the threshold, its setter and its environment name), the
K split auto takes over a grid of shapes (a pure function of K, M, N and 256 CUs where no device is initialised), the
pin's argument check, the hook switch's setter, and the new names in the header, the exports and the binding."""
import os
import re
import subprocess

import pytest

import f32w_ref as R
from hip_env import LIB_PATH, PKG, ROOT, ggml_hip

GEMV, EXACT, GEMM = 1, 4, 12


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(LIB_PATH):
        subprocess.check_call(["make", "-s", "-C", PKG, "-j4"])
    return ggml_hip.load()


@pytest.fixture
def lib(built):
    L = built
    exact, min_n = L.ggml_hip_get_exact(), L.ggml_hip_debug_set_f32w_gemm_min_n(-1)
    split, sw = L.ggml_hip_debug_set_f32w_gemm_ksplit(0), L.ggml_hip_debug_set_f32_w(0)
    env = os.environ.pop("GGML_HIP_F32W_GEMM_MIN_N", None)
    L.ggml_hip_set_exact(0)
    yield L
    os.environ.pop("GGML_HIP_F32W_GEMM_MIN_N", None)
    if env is not None:
        os.environ["GGML_HIP_F32W_GEMM_MIN_N"] = env
    L.ggml_hip_debug_set_f32w_gemm_min_n(min_n)
    L.ggml_hip_debug_set_f32w_gemm_ksplit(split)
    L.ggml_hip_debug_set_f32_w(sw)
    L.ggml_hip_set_exact(exact)


def test_auto_algo_rule(lib):
    auto = lib.ggml_hip_debug_f32w_auto_algo
    lib.ggml_hip_debug_set_f32w_gemm_min_n(-1)
    min_n = lib.ggml_hip_debug_set_f32w_gemm_min_n(-1)      # the default (no environment value)
    assert min_n >= 9
    for K in (32, 4096, 11008, 32768):
        for N in (1, 8, min_n - 1):
            assert auto(K, 4096, N) == GEMV
        for N in (min_n, min_n + 1, 512):
            assert auto(K, 4096, N) == GEMM
    for N in (1, 31, 32, 512):                              # one column's floats past the LDS: the exact kernel
        assert auto(32800, 64, N) == EXACT
    lib.ggml_hip_set_exact(1)
    for K, N in ((4096, 1), (4096, 512), (32, 9), (32800, 40)):
        assert auto(K, 100, N) == EXACT
    lib.ggml_hip_set_exact(0)
    assert auto(48, 4, 1) == ggml_hip.ERR_INVALID            # K % 32
    assert auto(4096, 0, 1) == ggml_hip.ERR_INVALID


def test_min_n_setter_and_environment(lib):
    auto, setter = lib.ggml_hip_debug_f32w_auto_algo, lib.ggml_hip_debug_set_f32w_gemm_min_n
    default = setter(100)
    assert setter(100) == 100                               # returns the previous value
    assert auto(4096, 64, 99) == GEMV and auto(4096, 64, 100) == GEMM
    assert setter(3) == 100 and setter(-1) == 9             # never below 9
    assert setter(-1) == default
    os.environ["GGML_HIP_F32W_GEMM_MIN_N"] = "77"
    setter(-1)                                              # re-reads the environment
    assert setter(-1) == 77
    assert auto(4096, 64, 76) == GEMV and auto(4096, 64, 77) == GEMM
    del os.environ["GGML_HIP_F32W_GEMM_MIN_N"]
    setter(-1)
    assert setter(-1) == default


def expected_split(K, M, N, cus=256):
    """the rule of csrc/f32_w_gemm.hip restated: the token tile; the S with the fewest rounds of workgroups per slice
    length, ceil(tiles S / CUs) / S, among equals the largest whose grid is resident at once (tiles S <= 2 CUs), else the
    smallest; slices of at least 8 chunks; then whole chunks per slice"""
    tm = (M + 127) // 128
    bn = 32 if N <= 32 else 64 if N <= 64 else (128 if tm * ((N + 127) // 128) >= cus else 64)
    tiles = tm * ((N + bn - 1) // bn)
    best, best_cost = 1, None
    for S in (1, 2, 4):
        if S > 1 and K // S < 256:
            break
        cost = -(-tiles * S // cus) * (4 // S)
        if best_cost is None or cost < best_cost or (cost == best_cost and tiles * S <= 2 * cus):
            best, best_cost = S, cost
    return R.gemm_ksplit(K, best)


def test_ksplit_over_a_grid_of_shapes(lib):
    split = lib.ggml_hip_debug_f32w_gemm_ksplit
    seen = set()
    for K in (32, 256, 512, 1024, 1504, 4096, 4544, 11008):
        for M in (1, 130, 4096, 11008, 32000):
            for N in (1, 9, 32, 33, 64, 65, 128, 512):
                s = split(K, M, N)
                assert s == expected_split(K, M, N), (K, M, N)
                assert s in (1, 2, 4) and K % (32 * s) == 0
                seen.add(s)
    assert seen == {1, 2, 4}
    # the LLaMA-7B layer shapes at N = 32: tiles alone do not fill 256 CUs
    assert (split(4096, 4096, 32), split(4096, 11008, 32), split(11008, 4096, 32)) == (4, 4, 4)
    assert split(4096, 4096, 4096) == 1                      # 1024 tiles of 128 x 128
    # the answer is auto's whatever is pinned
    assert lib.ggml_hip_debug_set_f32w_gemm_ksplit(1) == 0
    assert split(4096, 4096, 32) == 4
    assert split(48, 4, 1) == ggml_hip.ERR_INVALID and split(64, 0, 1) == ggml_hip.ERR_INVALID


def test_pin_and_switch_setters(lib):
    pin, sw = lib.ggml_hip_debug_set_f32w_gemm_ksplit, lib.ggml_hip_debug_set_f32_w
    assert pin(2) == 0 and pin(4) == 2 and pin(1) == 4 and pin(0) == 1
    for bad in (3, 5, 8, -1):
        assert pin(bad) == ggml_hip.ERR_INVALID
    assert pin(0) == 0                                       # a refused value changed nothing
    assert sw(1) == 0 and sw(1) == 1 and sw(0) == 1 and sw(0) == 0
    src = open(os.path.join(PKG, "csrc", "ggml-hip-core.cpp")).read()
    assert '"GGML_HIP_F32_W"' in src and '"GGML_HIP_F32W_GEMM_MIN_N"' in src
    assert '"GGML_HIP_F32W_NT"' in open(os.path.join(PKG, "csrc", "f32_w.hip")).read()


def test_rejected_algo_is_refused_first(built):
    """an algo the type does not have is INVALID before any other argument is looked at, an empty call included"""
    for algo in (2, 3, 5, 6, 7, 8, 9, 10, 11, 13, -1):
        assert built.ggml_hip_mul_mat_f32(None, 0, 0, None, 0, None, 0, algo, None) == ggml_hip.ERR_INVALID
        assert b"algo" in built.ggml_hip_last_error()


NEW_SYMBOLS = ("ggml_hip_mul_mat_f32", "ggml_hip_debug_f32w_auto_algo", "ggml_hip_debug_set_f32w_gemm_min_n",
               "ggml_hip_debug_set_f32w_gemm_ksplit", "ggml_hip_debug_f32w_gemm_ksplit", "ggml_hip_debug_set_f32_w")


def test_new_symbols_in_header_exports_and_binding(built):
    header = open(os.path.join(ROOT, "include", "ggml-hip.h")).read()
    exports = open(os.path.join(PKG, "exports.map")).read()
    assert re.search(r"global:\s*ggml_\*;", exports)        # every ggml_* name is exported, nothing else
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert getattr(built, name).argtypes is not None, name     # bound with a signature (and exported)
    assert ggml_hip.GGML_TYPE_F32 == 0 and callable(ggml_hip.mul_mat_f32)
