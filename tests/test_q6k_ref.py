"""CPU checks of the Q6_K path: the numpy restatement (tests/q6k_ref.py) reproduces the fixtures the compiled
reference wrote (tests/golden/gen_golden_q6k.c) bit for bit; a Q6_K tensor the backend cannot place on a device
gets a full-size host copy; the type table matches the reference's."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

import q6k_ref as R
from golden_io import GOLDEN, load
from hip_env import LIB_PATH, PKG, ggml_hip

KS = (256, 2304, 4096)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_q8k_equal(got, ref, K):
    """d bits, qs and bsums of block_q8_K rows; bsums skipped where amax == 0 (the reference leaves them unwritten)."""
    dg, qg, bg = R.split_q8_K(got, K)
    dr, qr, br = R.split_q8_K(ref, K)
    assert np.array_equal(bits(dg), bits(dr))
    assert np.array_equal(qg, qr)
    live = (dr != 0) | (qr != 0).any(axis=2)
    assert np.array_equal(bg[live], br[live])


@pytest.mark.parametrize("K", KS)
def test_ref_q8_K_matches_fixture(K):
    assert_q8k_equal(R.quantize_q8_K(load("q6k", f"x{K}_f32")), load("q6k", f"x{K}_q8_K"), K)


def test_ref_q8_K_crafted_blocks():
    x, ref = load("q6k", "craft_f32"), load("q6k", "craft_q8_K")
    assert_q8k_equal(R.quantize_q8_K(x), ref, 256)
    d, q, _ = R.split_q8_K(ref, 256)
    assert d[0, 0] == 0 and not q[0].any()                                  # all-zero block
    assert (q[1, 0, 5], q[1, 0, 9], d[1, 0]) == (-128, 127, np.float32(-0.015625))   # +max first: iscale < 0
    assert (q[2, 0, 5], q[2, 0, 9], d[2, 0]) == (-128, 127, np.float32(0.015625))    # -max first: iscale > 0
    a = np.abs(x[x != 0])
    assert a.min() >= 2.0 ** -100 and a.max() <= 2.0 ** 100


@pytest.mark.parametrize("K", KS)
def test_ref_dequantize_matches_fixture(K):
    ref = load("q6k", f"w{K}_dequant")
    got = R.dequantize_q6_K(load("q6k", f"w{K}_q6_K")[:ref.shape[0]], K)
    assert np.array_equal(bits(got), bits(ref))


@pytest.mark.parametrize("K", KS)
def test_ref_vec_dot_matches_fixture(K):
    wq, xq, y = load("q6k", f"w{K}_q6_K"), load("q6k", f"x{K}_q8_K"), load("q6k", f"y{K}_vec_dot")
    assert np.array_equal(bits(R.vec_dot_avx2(wq, xq, K)), bits(y))
    y_exact, s_abs = R.block_terms(wq, xq, K)                # and the exact terms agree with it within fp32 sums
    assert np.all(np.abs(y_exact - y) <= 1e-6 * s_abs + 1e-30)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB_PATH):
        subprocess.check_call(["make", "-s", "-C", PKG, "-j4"])
    return ggml_hip.load()


def test_q6_K_tensor_without_device_keeps_full_host_copy(lib):
    """No HIP device: ggml_hip_transform_tensor leaves a Q6_K tensor on the CPU, on a host copy of all
    210 * K / 256 * M bytes (the loader may free its buffer after the call), and free_data releases it."""
    if lib.ggml_hip_device_count() > 0:
        pytest.skip("a HIP device is present")
    K, M = 2304, 24
    src = np.ascontiguousarray(load("q6k", f"w{K}_q6_K"))
    nbytes = 210 * K // 256 * M
    assert src.nbytes == nbytes
    staged = src.copy()
    w = ggml_hip.make_tensor(ggml_hip.GGML_TYPE_Q6_K, (K, M), backend=ggml_hip.GGML_BACKEND_GPU_SPLIT)
    assert (w.nb[0], w.nb[1]) == (210, 210 * K // 256)
    lib.ggml_hip_transform_tensor(staged.ctypes.data_as(ctypes.c_void_p), ctypes.byref(w))
    assert w.backend == ggml_hip.GGML_BACKEND_CPU and not w.extra
    assert w.data and w.data != staged.ctypes.data
    staged[:] = 0                                            # the copy is the backend's own
    held = np.ctypeslib.as_array(ctypes.cast(w.data, ctypes.POINTER(ctypes.c_uint8)), shape=(nbytes,))
    assert np.array_equal(held.reshape(src.shape), src)
    del held
    lib.ggml_hip_free_data(ctypes.byref(w))
    assert not w.data


@pytest.mark.parametrize("gtype,size", [(12, 144), (10, 84), (15, 292)])
def test_declined_k_quant_without_device_keeps_full_host_copy(lib, gtype, size):
    """Q4_K / Q2_K / Q8_K stay declined; their host copy has the size gabi::type_size / blck_size give
    (size * K / 256 * M bytes), read back through the tensor."""
    if lib.ggml_hip_device_count() > 0:
        pytest.skip("a HIP device is present")
    K, M = 512, 9
    nbytes = size * K // 256 * M
    src = (np.arange(nbytes, dtype=np.uint32) * 7 + 3).astype(np.uint8)
    staged = src.copy()
    w = ggml_hip.make_tensor(gtype, (K, M), backend=ggml_hip.GGML_BACKEND_GPU)
    w.nb[0], w.nb[1] = size, size * K // 256
    w.nb[2] = w.nb[3] = w.nb[1] * M
    x = ggml_hip.make_tensor(ggml_hip.GGML_TYPE_F32, (K, 64))
    y = ggml_hip.make_tensor(ggml_hip.GGML_TYPE_F32, (M, 64))
    assert not lib.ggml_hip_can_mul_mat(ctypes.byref(w), ctypes.byref(x), ctypes.byref(y))
    lib.ggml_hip_transform_tensor(staged.ctypes.data_as(ctypes.c_void_p), ctypes.byref(w))
    assert w.backend == ggml_hip.GGML_BACKEND_CPU and not w.extra and w.data != staged.ctypes.data
    staged[:] = 0
    held = np.ctypeslib.as_array(ctypes.cast(w.data, ctypes.POINTER(ctypes.c_uint8)), shape=(nbytes,))
    assert np.array_equal(held, src)
    del held
    lib.ggml_hip_free_data(ctypes.byref(w))
    assert not w.data


def test_type_table_matches_reference_sizes():
    """csrc/ggml_abi.h's TYPE_TABLE equals GGML_TYPE_SIZE / GGML_BLCK_SIZE of a k-quants build for all 19 types
    (fixture written from the compiled reference by tests/golden/gen_golden_q6k.c; 4 and 5 are removed types)."""
    ref = json.load(open(os.path.join(GOLDEN, "ggml_type_sizes.json")))
    src = open(os.path.join(PKG, "csrc", "ggml_abi.h")).read()
    assert re.search(r"\bTYPE_COUNT = 19\b", src)
    rows = {int(t): (int(s), int(b), name) for t, s, b, name in
            re.findall(r"\{\s*(\d+),\s*(\d+),\s*(\d+)\s*\},?\s*//\s*(\w+)", src)}
    assert sorted(rows) == list(range(19))
    assert len(ref) == 17
    for t in range(19):
        size, blck, name = rows[t]
        if str(t) not in ref:
            assert t in (4, 5) and (size, blck) == (0, 0)
            continue
        assert (size, blck, name) == (ref[str(t)]["size"], ref[str(t)]["blck"], ref[str(t)]["name"]), t
    # spot values the loader depends on (ggml.c:3611-3655)
    assert rows[14][:2] == (210, 256) and rows[15][:2] == (292, 256) and rows[12][:2] == (144, 256)
    assert re.search(r"\bTYPE_Q6_K = 14\b", src)
