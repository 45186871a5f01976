"""CPU checks of the Q3_K / Q2_K path: the numpy restatement (tests/q23k_ref.py) reproduces the fixtures the compiled
reference wrote (tests/golden/gen_golden_q23k.c) bit for bit; without a device a Q3_K weight is declined and kept on
a full-size host copy; the new entry points are declared, exported and bound."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import q23k_ref as R
from golden_io import GOLDEN, load, manifest
from hip_env import LIB_PATH, PKG, ggml_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (variant, q3, type name, fixture Ks)
TYPES = {"q3k": (True, "q3_K", (256, 768, 4096)), "q2k": (False, "q2_K", (256, 768, 4096))}
CASES = [(v, K) for v, (_, _, ks) in TYPES.items() for K in ks]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("variant,K", CASES)
def test_fixture_shapes_and_sizes(variant, K):
    q3, tname, _ = TYPES[variant]
    w = load(variant, f"w{K}_{tname}")
    assert w.shape == (24, R.block_bytes(q3) * K // 256)
    assert load(variant, f"x{K}_q8_K").shape == (3, 292 * K // 256)
    assert load(variant, f"w{K}_dequant").shape == (8, K)
    assert load(variant, f"y{K}_vec_dot").shape == (3, 24)
    for entry in manifest(variant).values():
        assert entry["bytes"] <= 131072
        assert os.path.getsize(os.path.join(GOLDEN, entry["file"])) == entry["bytes"]


@pytest.mark.parametrize("variant,K", CASES)
def test_ref_q8_K_matches_fixture(variant, K):
    got, ref = R.quantize_q8_K(load(variant, f"x{K}_f32")), load(variant, f"x{K}_q8_K")
    assert np.array_equal(got, ref)                          # N(0, 1) rows: no all-zero block, so bsums too


@pytest.mark.parametrize("variant,K", CASES)
def test_ref_dequantize_matches_fixture(variant, K):
    q3, tname, _ = TYPES[variant]
    ref = load(variant, f"w{K}_dequant")
    got = R.dequantize(load(variant, f"w{K}_{tname}")[:ref.shape[0]], K, q3)
    assert np.array_equal(bits(got), bits(ref))


@pytest.mark.parametrize("variant,K", CASES)
def test_ref_vec_dot_matches_fixture(variant, K):
    q3, tname, _ = TYPES[variant]
    wq, xq, y = load(variant, f"w{K}_{tname}"), load(variant, f"x{K}_q8_K"), load(variant, f"y{K}_vec_dot")
    assert np.array_equal(bits(R.vec_dot_avx2(wq, xq, K, q3)), bits(y))
    # and the exact terms agree with it within fp32 sums.  The AVX2 dot rounds eight per-lane chains, whose terms can
    # cancel inside a superblock (the signed Q3_K scales and values), so its rounding error scales with the sum of
    # the |lane terms|, not with S_abs' |superblock terms|: at most (8 nb + 3) roundings of 2^-24 each, far below 1e-6
    y_exact, s_abs = R.block_terms(wq, xq, K, q3)
    dw, dminw, dx, lanes, prod = R._int_terms(wq, xq, K, q3)
    dd = dx.astype(np.float64)[:, None, :, None]
    lane_abs = (np.abs(dd * dw.astype(np.float64)[None, :, :, None] * lanes)
                + np.abs(dd * dminw.astype(np.float64)[None, :, :, None] * prod)).sum(axis=(2, 3))
    assert np.all(lane_abs >= s_abs * (1 - 1e-12))
    assert np.all(np.abs(y_exact - y) <= 1e-6 * lane_abs + 1e-30)
    # the dequantized weights times the q8_K values give the same sums (the terms decode the blocks correctly)
    dx, q8, _ = R.split_q8_K(xq, K)
    xdq = (dx[:, :, None].astype(np.float64) * q8).reshape(3, K)
    y_deq = xdq @ R.dequantize(wq, K, q3).astype(np.float64).T
    assert np.all(np.abs(y_deq - y_exact) <= 1e-5 * s_abs + 1e-30)


@pytest.mark.parametrize("q3", [True, False])
def test_random_blocks_cover_the_specials(q3):
    rng = np.random.default_rng(23 + q3)
    K, M = 2304, 16
    wq = R.random_q23_K(rng, M, K, q3)
    assert wq.shape == (M, R.block_bytes(q3) * K // 256) and wq.dtype == np.uint8
    if q3:
        d, sc, q = R.split_q3_K(wq, K)
        assert (sc == -32).all(axis=2).any() and (sc == 31).all(axis=2).any()
        assert sc.min() == -32 and sc.max() == 31 and q.min() == -4 and q.max() == 3
        assert (q >= 0).all(axis=(2, 3)).any() and (q < 0).all(axis=(2, 3)).any()    # hmask all set / all clear
    else:
        d, dmin, sc, m, q = R.split_q2_K(wq, K)
        assert (dmin == 0).any() and (dmin < 0).any()
        assert (np.abs(dmin[dmin != 0]) < 6.2e-5).any()                             # an fp16 subnormal
        assert ((sc == 0) & (m == 0)).all(axis=2).any() and ((sc == 15) & (m == 15)).all(axis=2).any()
        assert q.min() == 0 and q.max() == 3
    assert (d == 0).any() and (d < 0).any() and (np.abs(d[d != 0]) < 6.2e-5).any()


@pytest.mark.parametrize("q3", [True, False])
def test_gemv_schedule_within_bound_of_exact_terms(q3):
    """the device GEMV's fp32 order, restated, stays within the parity bound of the exact terms on the special
    blocks, and x -> 2x doubles it bitwise."""
    rng = np.random.default_rng(23 + q3)
    K, M, N = 2304, 16, 2
    wq = R.random_q23_K(rng, M, K, q3)
    x = rng.standard_normal((N, K)).astype(np.float32)
    y = R.gemv_schedule(wq, x, K, q3)
    y_exact, s_abs = R.block_terms(wq, R.quantize_q8_K(x), K, q3)
    assert np.all(np.abs(y - y_exact) <= 1e-3 * np.abs(y_exact) + 1e-6 * s_abs)
    assert np.array_equal(bits(R.gemv_schedule(wq, 2 * x, K, q3)), bits(2 * y))


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(LIB_PATH):
        subprocess.check_call(["make", "-s", "-C", PKG, "-j4"])
    return ggml_hip.load()


def test_q3_K_tensor_without_device_is_declined_on_full_host_copy(built):
    """No HIP device: can_mul_mat declines a Q3_K weight, and ggml_hip_transform_tensor leaves it on the CPU on a
    host copy of all 110 * K / 256 * M bytes (the loader may free its buffer after the call)."""
    lib = built
    if lib.ggml_hip_device_count() > 0:
        pytest.skip("a HIP device is present")
    K, M = 768, 24
    src = np.ascontiguousarray(load("q3k", f"w{K}_q3_K"))
    nbytes = 110 * K // 256 * M
    assert src.nbytes == nbytes
    staged = src.copy()
    w = ggml_hip.make_tensor(ggml_hip.GGML_TYPE_Q3_K, (K, M), backend=ggml_hip.GGML_BACKEND_GPU_SPLIT)
    assert (w.nb[0], w.nb[1]) == (110, 110 * K // 256)
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


NEW_SYMBOLS = ("ggml_hip_mul_mat_q3_K", "ggml_hip_mul_mat_q2_K", "ggml_hip_dequantize_q3_K", "ggml_hip_dequantize_q2_K",
               "ggml_hip_debug_q23k_auto_algo")


def test_new_symbols_in_header_exports_and_binding(built):
    header = open(os.path.join(ROOT, "include", "ggml-hip.h")).read()
    exports = open(os.path.join(PKG, "exports.map")).read()
    assert re.search(r"global:\s*ggml_\*;", exports)        # every ggml_* name is exported, nothing else
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert getattr(built, name).argtypes is not None, name     # bound with a signature (and exported)
    assert (ggml_hip.GGML_TYPE_Q2_K, ggml_hip.GGML_TYPE_Q3_K) == (10, 11)
    for f in ("mul_mat_q3_K", "mul_mat_q2_K", "dequantize_q3_K", "dequantize_q2_K"):
        assert callable(getattr(ggml_hip, f)), f
    src = open(os.path.join(PKG, "csrc", "ggml_abi.h")).read()
    assert re.search(r"\bTYPE_Q2_K = 10\b", src) and re.search(r"\bTYPE_Q3_K = 11\b", src)
    assert re.search(r"^KERNELS\s*=.*\bq23_k\b", open(os.path.join(PKG, "Makefile")).read(), re.M)


def test_status_codes_without_device(built):
    """argument checks that come before any device use"""
    lib = built
    for f in (lib.ggml_hip_dequantize_q3_K, lib.ggml_hip_dequantize_q2_K):
        assert f(None, 256, 1, None, None) == ggml_hip.ERR_INVALID
        assert f(ctypes.c_void_p(16), 128, 1, ctypes.c_void_p(16), None) == ggml_hip.ERR_INVALID   # K % 256
    for gtype in (ggml_hip.GGML_TYPE_Q3_K, ggml_hip.GGML_TYPE_Q2_K):
        assert lib.ggml_hip_debug_q23k_auto_algo(gtype, 4096, 4096, 1) == 1
        assert lib.ggml_hip_debug_q23k_auto_algo(gtype, 4096, 4096, 512) == 1      # no GEMM: the GEMV's column tiles
        assert lib.ggml_hip_debug_q23k_auto_algo(gtype, 16384, 64, 1) == 1
        assert lib.ggml_hip_debug_q23k_auto_algo(gtype, 17920, 64, 1) == 4         # beyond the GEMV's K
        assert lib.ggml_hip_debug_q23k_auto_algo(gtype, 100, 64, 1) == ggml_hip.ERR_INVALID
    assert lib.ggml_hip_debug_q23k_auto_algo(ggml_hip.GGML_TYPE_Q5_K, 4096, 64, 1) == ggml_hip.ERR_INVALID
