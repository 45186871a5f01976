"""CPU checks of the Q8_0-weight path: the numpy restatement (tests/q8_0w_ref.py) reproduces the fixtures the
compiled reference wrote (tests/golden/gen_golden_q8_0w.c) bit for bit; the rule behind algo 0 of
ggml_hip_mul_mat_q8_0 (no device needed); a Q8_0 tensor the backend cannot place on a device keeps a full-size
host copy; the new entry points are in the header, the export map and the binding."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import q8_0w_ref as R
from golden_io import load
from hip_env import LIB_PATH, PKG, ROOT, ggml_hip

KS = (64, 2304, 4160)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("K", KS)
def test_ref_dequantize_matches_fixture(K):
    ref = load("q8w", f"w{K}_dequant")
    got = R.dequantize_q8_0(load("q8w", f"w{K}_q8_0")[:ref.shape[0]], K)
    assert np.array_equal(bits(got), bits(ref))


@pytest.mark.parametrize("K", KS)
def test_ref_activations_match_oracle_quantizer(K):
    import oracle as O
    assert np.array_equal(O.quantize_q8_0(load("q8w", f"x{K}_f32"), "avx2"), load("q8w", f"x{K}_q8_0"))


@pytest.mark.parametrize("K", KS)
def test_ref_vec_dot_matches_fixture(K):
    wq, xq, y = load("q8w", f"w{K}_q8_0"), load("q8w", f"x{K}_q8_0"), load("q8w", f"y{K}_vec_dot")
    assert np.array_equal(bits(R.vec_dot_avx2(wq, xq, K)), bits(y))
    y_exact, s_abs = R.block_terms(wq, xq, K)                # and the exact terms agree with it within fp32 sums
    assert np.all(np.abs(y_exact - y) <= 1e-6 * s_abs + 1e-30)


def test_ref_crafted_blocks():
    wq, xq = load("q8w", "craft_q8_0"), load("q8w", "craft_x_q8_0")
    assert np.array_equal(bits(R.dequantize_q8_0(wq, 64)), bits(load("q8w", "craft_dequant")))
    y = load("q8w", "craft_y")
    assert np.array_equal(bits(R.vec_dot_avx2(wq, xq, 64)), bits(y))
    import oracle as O
    assert np.array_equal(O.quantize_q8_0(load("q8w", "craft_x_f32"), "avx2"), xq)
    # what the rows are: all -128, all +127, d = 0 / -0, subnormal d; x rows 1 and 2 at +-amax
    d, q = R.split_q8_0(wq, 64)
    assert (q[0] == -128).all() and (q[1] == 127).all() and set(np.unique(q[2])) == {-127, 127}
    assert d[3, 0] == 0 and d[3, 1] == 0 and np.signbit(d[3, 1]) and not np.signbit(d[3, 0])
    assert d[4, 0] == np.float32(2.0 ** -24) and d[4, 1] == -np.float32(1023 * 2.0 ** -24)
    _, qx = R.split_q8_0(xq, 64)
    assert set(np.unique(qx[1])) == {-127, 127} and (qx[2] == 127).all() and not qx[3].any()
    # the largest block sums, exact: -128 * 127 * 32 and 127 * 127 * 32 per block
    _, _, lanes = R._lane_sums(wq, xq, 64)
    isum = lanes.sum(axis=3)
    assert (isum[2, 0] == -128 * 127 * 32).all() and (isum[2, 1] == 127 * 127 * 32).all()
    assert (isum[1, 2] == [127 * 127 * 32, -127 * 127 * 32]).all()
    assert (y[:, 3] == 0).all() and (y[3] == 0).all()


def test_fmaf32_matches_libm():
    """The round-to-odd float32 fma of the restatement against libm's fmaf on the operand shapes it is used for
    (a float32 scale, an integer below 2^17, a float32 accumulator), ties and cancellations included."""
    libm = ctypes.CDLL("libm.so.6")
    libm.fmaf.restype = ctypes.c_float
    libm.fmaf.argtypes = [ctypes.c_float] * 3
    rng = np.random.default_rng([0x80, 1])
    n = 4000
    a = (rng.standard_normal(n) * np.exp2(rng.integers(-30, 10, n))).astype(np.float32)
    b = rng.integers(-65024, 65025, n).astype(np.float32)
    c = (rng.standard_normal(n) * np.exp2(rng.integers(-30, 24, n))).astype(np.float32)
    c[::7] = (-a[::7].astype(np.float64) * b[::7]).astype(np.float32)         # near cancellation
    a[1::11] = np.float32(1 + 2.0 ** -23)                                    # products that end in a half ulp
    b[1::11] = 3
    c[1::11] = np.float32(2.0 ** 2)
    got = R.fmaf32(a, b, c)
    ref = np.array([libm.fmaf(x, y, z) for x, y, z in zip(a.tolist(), b.tolist(), c.tolist())], np.float32)
    assert np.array_equal(bits(got), bits(ref))
    assert bits(R.fmaf32(np.float32([1.5]), np.float32([1.0]), np.float32([math.ldexp(1.0, 24)])))[0] == \
           bits(np.float32([libm.fmaf(1.5, 1.0, math.ldexp(1.0, 24))]))[0]


def test_gemv_schedule_properties():
    """The restated GEMV order (64 lane chains and the wave tree): within the parity bound of the exact-mode
    restatement on the same inputs, x -> 2x bitwise, and a row's and a column's y independent of what is passed with
    it.  K = 64: one pair; 4160: 65 pairs (lane 0 a two-pair chain); 11008: 172 pairs."""
    import oracle as O
    from parity import check_y
    for K in (64, 4160, 11008):
        rng = np.random.default_rng([0x80, 3, K])
        M, N = 7, 3
        wq = R.random_q8_0(rng, M, K)
        x = rng.standard_normal((N, K)).astype(np.float32)
        y = R.gemv_schedule(wq, x, K)
        xq = O.quantize_q8_0(x, "avx2")
        check_y(y, R.vec_dot_avx2(wq, xq, K), R.block_terms(wq, xq, K)[1], rtol=1e-3, atol_blocks=1e-6)
        assert np.array_equal(bits(R.gemv_schedule(wq, 2 * x, K)), bits(2 * y))
        assert np.array_equal(bits(R.gemv_schedule(wq[2:5], x[1:2], K)), bits(y[1:2, 2:5]))
        assert np.any(y != 0)


def test_q4_0_as_q8_0_keeps_the_values():
    import oracle as O
    from parity import split_q4_0
    K = 128
    w4q, _ = O.quantize_q4_0((np.random.default_rng([0x80, 2]).standard_normal((5, K)) * 0.02).astype(np.float32))
    d4, w4 = split_q4_0(w4q, K)
    d8, w8 = R.split_q8_0(R.q4_0_as_q8_0(w4q, K), K)
    assert np.array_equal(bits(d4), bits(d8)) and np.array_equal(w4, w8)
    assert np.array_equal(bits(R.dequantize_q8_0(R.q4_0_as_q8_0(w4q, K), K)), bits(O.dequantize_q4_0(w4q, K)))


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(LIB_PATH):
        subprocess.check_call(["make", "-s", "-C", PKG, "-j4"])
    return ggml_hip.load()


@pytest.fixture
def lib(built):
    L = built
    exact, min_n = L.ggml_hip_get_exact(), L.ggml_hip_debug_set_q8_0_gemm_min_n(-1)
    env = os.environ.pop("GGML_HIP_Q8_0_GEMM_MIN_N", None)
    L.ggml_hip_set_exact(0)
    yield L
    os.environ.pop("GGML_HIP_Q8_0_GEMM_MIN_N", None)
    if env is not None:
        os.environ["GGML_HIP_Q8_0_GEMM_MIN_N"] = env
    L.ggml_hip_debug_set_q8_0_gemm_min_n(min_n)
    L.ggml_hip_set_exact(exact)


def test_auto_algo_rule(lib):
    auto = lib.ggml_hip_debug_q8_0_auto_algo
    lib.ggml_hip_debug_set_q8_0_gemm_min_n(-1)
    min_n = lib.ggml_hip_debug_set_q8_0_gemm_min_n(-1)      # the default (no environment value)
    assert min_n >= 9
    for N in (1, 8, min_n - 1):
        assert auto(4096, 4096, N) == 1
    for N in (min_n, min_n + 1, 512):
        assert auto(4096, 4096, N) == 2
    assert auto(11008, 4096, 1) == 1 and auto(64, 1, 1) == 1
    lib.ggml_hip_set_exact(1)
    for K, N in ((4096, 1), (4096, 512), (64, 9)):
        assert auto(K, 100, N) == 4
    lib.ggml_hip_set_exact(0)
    assert auto(96, 4, 1) == ggml_hip.ERR_INVALID             # K % 64
    assert auto(4096, 0, 1) == ggml_hip.ERR_INVALID


def test_min_n_setter_and_environment(lib):
    auto, setter = lib.ggml_hip_debug_q8_0_auto_algo, lib.ggml_hip_debug_set_q8_0_gemm_min_n
    default = setter(100)
    assert setter(100) == 100                               # returns the previous value
    assert auto(4096, 64, 99) == 1 and auto(4096, 64, 100) == 2
    assert setter(3) == 100 and setter(-1) == 9             # never below 9
    assert setter(-1) == default
    os.environ["GGML_HIP_Q8_0_GEMM_MIN_N"] = "77"
    setter(-1)                                              # re-reads the environment
    assert setter(-1) == 77
    assert auto(4096, 64, 76) == 1 and auto(4096, 64, 77) == 2
    os.environ["GGML_HIP_Q8_0_GEMM_MIN_N"] = "2"            # below 9 counts as 9
    setter(-1)
    assert setter(-1) == 9
    del os.environ["GGML_HIP_Q8_0_GEMM_MIN_N"]
    setter(-1)
    assert setter(-1) == default


def test_q8_0_tensor_without_device_is_declined_on_full_host_copy(built):
    """No HIP device: can_mul_mat declines a Q8_0 weight, and ggml_hip_transform_tensor leaves it on the CPU on a
    host copy of all 34 * K / 32 * M bytes (the loader may free its buffer after the call)."""
    lib = built
    if lib.ggml_hip_device_count() > 0:
        pytest.skip("a HIP device is present")
    K, M = 2304, 24
    src = np.ascontiguousarray(load("q8w", f"w{K}_q8_0"))
    nbytes = 34 * K // 32 * M
    assert src.nbytes == nbytes
    staged = src.copy()
    w = ggml_hip.make_tensor(ggml_hip.GGML_TYPE_Q8_0, (K, M), backend=ggml_hip.GGML_BACKEND_GPU_SPLIT)
    assert (w.nb[0], w.nb[1]) == (34, 34 * K // 32)
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


NEW_SYMBOLS = ("ggml_hip_mul_mat_q8_0", "ggml_hip_dequantize_q8_0", "ggml_hip_debug_q8_0_auto_algo",
               "ggml_hip_debug_set_q8_0_gemm_min_n")


def test_new_symbols_in_header_exports_and_binding(built):
    header = open(os.path.join(ROOT, "include", "ggml-hip.h")).read()
    exports = open(os.path.join(PKG, "exports.map")).read()
    assert re.search(r"global:\s*ggml_\*;", exports)        # every ggml_* name is exported, nothing else
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert getattr(built, name).argtypes is not None, name     # bound with a signature (and exported)
    assert ggml_hip.GGML_TYPE_Q8_0 == 8
    assert callable(ggml_hip.mul_mat_q8_0) and callable(ggml_hip.dequantize_q8_0)
    src = open(os.path.join(PKG, "csrc", "ggml_abi.h")).read()
    assert re.search(r"\bTYPE_Q8_0 = 8\b", src) and re.search(r"\{\s*8,\s*34,\s*32\s*\}", src)
