"""CPU checks of the Q5_K / Q4_K path: the numpy restatement (tests/q45k_ref.py) reproduces the fixtures the compiled
reference wrote (tests/golden/gen_golden_q45k.c) bit for bit; without a device a Q5_K weight is declined and kept on
a full-size host copy; the new entry points are declared, exported and bound."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import q45k_ref as R
from golden_io import GOLDEN, load, manifest
from hip_env import LIB_PATH, PKG, ggml_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (variant, qh, type name, fixture Ks)
TYPES = {"q5k": (True, "q5_K", (256, 2304, 4096)), "q4k": (False, "q4_K", (256, 2304))}
CASES = [(v, K) for v, (_, _, ks) in TYPES.items() for K in ks]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("variant,K", CASES)
def test_fixture_shapes_and_sizes(variant, K):
    qh, tname, _ = TYPES[variant]
    w = load(variant, f"w{K}_{tname}")
    assert w.shape == (24, R.block_bytes(qh) * K // 256)
    assert load(variant, f"x{K}_q8_K").shape == (3, 292 * K // 256)
    for entry in manifest(variant).values():
        assert entry["bytes"] <= 131072
        assert os.path.getsize(os.path.join(GOLDEN, entry["file"])) == entry["bytes"]


@pytest.mark.parametrize("variant,K", CASES)
def test_ref_q8_K_matches_fixture(variant, K):
    got, ref = R.quantize_q8_K(load(variant, f"x{K}_f32")), load(variant, f"x{K}_q8_K")
    assert np.array_equal(got, ref)                          # N(0, 1) rows: no all-zero block, so bsums too


@pytest.mark.parametrize("variant,K", CASES)
def test_ref_dequantize_matches_fixture(variant, K):
    qh, tname, _ = TYPES[variant]
    ref = load(variant, f"w{K}_dequant")
    got = R.dequantize_q45_K(load(variant, f"w{K}_{tname}")[:ref.shape[0]], K, qh)
    assert np.array_equal(bits(got), bits(ref))


@pytest.mark.parametrize("variant,K", CASES)
def test_ref_vec_dot_matches_fixture(variant, K):
    qh, tname, _ = TYPES[variant]
    wq, xq, y = load(variant, f"w{K}_{tname}"), load(variant, f"x{K}_q8_K"), load(variant, f"y{K}_vec_dot")
    assert np.array_equal(bits(R.vec_dot_avx2(wq, xq, K, qh)), bits(y))
    y_exact, s_abs = R.block_terms(wq, xq, K, qh)            # and the exact terms agree with it within fp32 sums
    assert np.all(np.abs(y_exact - y) <= 1e-6 * s_abs + 1e-30)
    # the dequantized weights times the q8_K values give the same sums (the terms decode the blocks correctly)
    dx, q8, _ = R.split_q8_K(xq, K)
    xdq = (dx[:, :, None].astype(np.float64) * q8).reshape(3, K)
    y_deq = xdq @ R.dequantize_q45_K(wq, K, qh).astype(np.float64).T
    assert np.all(np.abs(y_deq - y_exact) <= 1e-5 * s_abs + 1e-30)


@pytest.mark.parametrize("qh", [True, False])
def test_gemv_schedule_within_bound_of_exact_terms(qh):
    """the device GEMV's fp32 order, restated, stays within the parity bound of the exact terms on random blocks
    (zero, negative and subnormal d / dmin, scales and mins of 0 and 63 included)."""
    rng = np.random.default_rng(45 + qh)
    K, M, N = 2304, 16, 2
    wq = R.random_q45_K(rng, M, K, qh)
    x = rng.standard_normal((N, K)).astype(np.float32)
    d, dmin, sc, m, q = R.split_q45_K(wq, K, qh)
    assert (d == 0).any() and (d < 0).any() and (dmin < 0).any()
    assert (sc == 0).all(axis=2).any() and (sc == 63).all(axis=2).any() and (m == 63).all(axis=2).any()
    assert q.max() == (31 if qh else 15) and q.min() == 0
    y = R.gemv_schedule(wq, x, K, qh)
    y_exact, s_abs = R.block_terms(wq, R.quantize_q8_K(x), K, qh)
    assert np.all(np.abs(y - y_exact) <= 1e-3 * np.abs(y_exact) + 1e-6 * s_abs)
    assert np.array_equal(bits(R.gemv_schedule(wq, 2 * x, K, qh)), bits(2 * y))


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(LIB_PATH):
        subprocess.check_call(["make", "-s", "-C", PKG, "-j4"])
    return ggml_hip.load()


def test_q5_K_tensor_without_device_is_declined_on_full_host_copy(built):
    """No HIP device: can_mul_mat declines a Q5_K weight, and ggml_hip_transform_tensor leaves it on the CPU on a
    host copy of all 176 * K / 256 * M bytes (the loader may free its buffer after the call)."""
    lib = built
    if lib.ggml_hip_device_count() > 0:
        pytest.skip("a HIP device is present")
    K, M = 2304, 24
    src = np.ascontiguousarray(load("q5k", f"w{K}_q5_K"))
    nbytes = 176 * K // 256 * M
    assert src.nbytes == nbytes
    staged = src.copy()
    w = ggml_hip.make_tensor(ggml_hip.GGML_TYPE_Q5_K, (K, M), backend=ggml_hip.GGML_BACKEND_GPU_SPLIT)
    assert (w.nb[0], w.nb[1]) == (176, 176 * K // 256)
    x = ggml_hip.make_tensor(ggml_hip.GGML_TYPE_F32, (K, 64))
    y = ggml_hip.make_tensor(ggml_hip.GGML_TYPE_F32, (M, 64))
    assert not lib.ggml_hip_can_mul_mat(ctypes.byref(w), ctypes.byref(x), ctypes.byref(y))
    lib.ggml_hip_transform_tensor(staged.ctypes.data_as(ctypes.c_void_p), ctypes.byref(w))
    assert w.backend == ggml_hip.GGML_BACKEND_CPU and not w.extra
    assert w.data and w.data != staged.ctypes.data
    staged[:] = 0                                            # the copy is the backend's own
    held = np.ctypeslib.as_array(ctypes.cast(w.data, ctypes.POINTER(ctypes.c_uint8)), shape=(nbytes,))
    assert np.array_equal(held.reshape(src.shape), src)
    del held
    lib.ggml_hip_free_data(ctypes.byref(w))
    assert not w.data


def test_q4_K_switch_is_off_by_default_and_returns_the_previous_value(built):
    lib = built
    if os.environ.get("GGML_HIP_Q4_K"):
        pytest.skip("GGML_HIP_Q4_K is set in the environment")
    prev = lib.ggml_hip_debug_set_q4_K(1)
    try:
        assert prev == 0                                     # off unless asked for
        assert lib.ggml_hip_debug_set_q4_K(0) == 1
        assert lib.ggml_hip_debug_set_q4_K(5) == 0           # any nonzero value is "on"
        assert lib.ggml_hip_debug_set_q4_K(0) == 1
    finally:
        lib.ggml_hip_debug_set_q4_K(prev)


NEW_SYMBOLS = ("ggml_hip_mul_mat_q5_K", "ggml_hip_mul_mat_q4_K", "ggml_hip_dequantize_q5_K", "ggml_hip_dequantize_q4_K",
               "ggml_hip_debug_set_q4_K")


def test_new_symbols_in_header_exports_and_binding(built):
    header = open(os.path.join(ROOT, "include", "ggml-hip.h")).read()
    exports = open(os.path.join(PKG, "exports.map")).read()
    assert re.search(r"global:\s*ggml_\*;", exports)        # every ggml_* name is exported, nothing else
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert getattr(built, name).argtypes is not None, name     # bound with a signature (and exported)
    assert (ggml_hip.GGML_TYPE_Q4_K, ggml_hip.GGML_TYPE_Q5_K) == (12, 13)
    for f in ("mul_mat_q5_K", "mul_mat_q4_K", "dequantize_q5_K", "dequantize_q4_K"):
        assert callable(getattr(ggml_hip, f)), f
    src = open(os.path.join(PKG, "csrc", "ggml_abi.h")).read()
    assert re.search(r"\bTYPE_Q4_K = 12\b", src) and re.search(r"\bTYPE_Q5_K = 13\b", src)
    assert "q45_k" in open(os.path.join(PKG, "Makefile")).read()


def test_status_codes_without_device(built):
    """argument checks that come before any device use"""
    lib = built
    for f in (lib.ggml_hip_dequantize_q5_K, lib.ggml_hip_dequantize_q4_K):
        assert f(None, 256, 1, None, None) == ggml_hip.ERR_INVALID
        assert f(ctypes.c_void_p(16), 128, 1, ctypes.c_void_p(16), None) == ggml_hip.ERR_INVALID   # K % 256
