"""CPU checks of the Q4_1 / Q5_0 / Q5_1 weight path: the numpy restatement (tests/q5x_ref.py) reproduces the fixtures
the compiled reference wrote (tests/golden/gen_golden_q5x.c) bit for bit, the weight quantizers included; the rule
behind algo 0 of the three mul_mats (no device needed); a tensor of each type the backend cannot place on a device
keeps a full-size host copy; the new entry points are in the header, the export map and the binding."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import q5x_ref as R
from golden_io import GOLDEN, load, manifest
from hip_env import LIB_PATH, PKG, ROOT, ggml_hip

KS = (64, 2304, 4160)
TYPES = R.VARIANTS
NAME = {"q41": "q4_1", "q50": "q5_0", "q51": "q5_1"}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("t", TYPES)
def test_ref_dequantize_matches_fixture(t, K):
    ref = load(t, f"w{K}_dequant")
    got = R.dequantize(t, load(t, f"w{K}_q")[:ref.shape[0]], K)
    assert np.array_equal(bits(got), bits(ref))


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("t", TYPES)
def test_ref_weight_quantizer_matches_fixture(t, K):
    w = load(t, f"w{K}_f32")
    assert np.array_equal(R.quantize_w(t, w), load(t, f"w{K}_q")[:w.shape[0]])


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("t", TYPES)
def test_ref_activation_quantizer_matches_fixture(t, K):
    xq = load(t, f"x{K}_q")
    assert xq.shape[1] == (40 if R.has_min(t) else 34) * K // 32
    assert np.array_equal(R.quantize_x(t, load(t, f"x{K}_f32")), xq)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("t", TYPES)
def test_ref_vec_dot_matches_fixture(t, K):
    wq, xq, y = load(t, f"w{K}_q"), load(t, f"x{K}_q"), load(t, f"y{K}_vec_dot")
    assert np.array_equal(bits(R.vec_dot_avx2(t, wq, xq, K)), bits(y))
    y_exact, s_abs = R.block_terms(t, wq, xq, K)             # and the exact terms agree with it within fp32 sums
    assert np.all(np.abs(y_exact - y) <= 1e-6 * s_abs + 1e-30)


@pytest.mark.parametrize("t", ["q41", "q51"])
def test_fixtures_settle_summs_as_multiply_then_add(t):
    """summs += fp32(m) * s: the compiled reference rounds the product to float32 before the add; the fma form
    disagrees with its fixtures."""
    for K in (2304, 4160):
        wq, xq, y = load(t, f"w{K}_q"), load(t, f"x{K}_q"), load(t, f"y{K}_vec_dot")
        assert not np.array_equal(bits(R.vec_dot_avx2(t, wq, xq, K, summs_fma=True)), bits(y))


@pytest.mark.parametrize("t", TYPES)
def test_ref_crafted_blocks(t):
    wq, xq = load(t, "craft_q"), load(t, "craft_x_q")
    assert np.array_equal(bits(R.dequantize(t, wq, 64)), bits(load(t, "craft_dequant")))
    y = load(t, "craft_y")
    assert np.array_equal(bits(R.vec_dot_avx2(t, wq, xq, 64)), bits(y))
    assert np.array_equal(R.quantize_x(t, load(t, "craft_x_f32")), xq)
    # what the rows are
    d, m, q = R.split(t, wq, 64)
    top = 31 if R.has_qh(t) else 15
    assert (q[0, 0] == 0).all() and (q[0, 1] == top).all()
    if R.has_qh(t):
        # 0xF0 bytes: elements 0 .. 15 are 0, 16 .. 31 are 15; qh = 0xAAAAAAAA adds 16 to the odd elements
        assert (q[1, 0] == np.concatenate([np.tile([0, 16], 8), np.tile([15, 31], 8)])).all()
        assert ((q[2, 0] >> 4) == np.repeat([1, 0], 16)).all()                # qh = 0x0000FFFF: elements 0 .. 15
        assert ((q[2, 1] >> 4) == np.repeat([0, 1], 16)).all()                # qh = 0xFFFF0000: elements 16 .. 31
        assert np.array_equal(q[2, 0] & 15, q[2, 1] & 15)
        assert (q[5, 0] == 16).all() and (q[5, 1] == 15).all()
    else:
        assert (q[1, 0] == np.repeat([0, 15], 16)).all()
    assert d[3, 0] == 0 and d[3, 1] == 0 and np.signbit(d[3, 1]) and not np.signbit(d[3, 0])
    assert d[4, 0] == np.float32(2.0 ** -24) and d[4, 1] == -np.float32(1023 * 2.0 ** -24)
    if R.has_min(t):
        assert m[3, 0] == 0 and np.signbit(m[3, 1]) and m[4, 1] == np.float32(2.0 ** -24)
        assert d[5, 0] < 0 < m[5, 0] and m[5, 1] < 0 < d[5, 1]
    dx, sx, qx = R.split_x(t, xq, 64)
    assert set(np.unique(qx[1])) == {-127, 127} and (qx[2] == 127).all() and not qx[3].any()
    if R.has_min(t):                                                          # the largest s: d * 4064
        assert np.array_equal(bits(sx[2]), bits((dx[2] * np.float32(4064)).astype(np.float32)))
    assert (y[3] == 0).all() and (y[:, 3] == 0).all()


@pytest.mark.parametrize("t", TYPES)
def test_gemv_schedule_properties(t):
    """The restated GEMV order (64 lane chains and the wave tree): within the parity bound of the exact-mode
    restatement on the same inputs, x -> 2x bitwise, and a row's and a column's y independent of what is passed with
    it.  K = 64: one pair; 4160: 65 pairs (lane 0 a two-pair chain); 11008: 172 pairs."""
    from parity import check_y
    for K in (64, 4160, 11008):
        rng = np.random.default_rng([0x51, 2, R.TYPES[t][0], K])
        M, N = 7, 3
        wq = R.random_blocks(rng, M, K, R.has_qh(t), R.has_min(t))
        x = rng.standard_normal((N, K)).astype(np.float32)
        y = R.gemv_schedule(t, wq, x, K)
        xq = R.quantize_x(t, x)
        check_y(y, R.vec_dot_avx2(t, wq, xq, K), R.block_terms(t, wq, xq, K)[1], rtol=1e-3, atol_blocks=1e-6)
        assert np.array_equal(bits(R.gemv_schedule(t, wq, 2 * x, K)), bits(2 * y))
        assert np.array_equal(bits(R.gemv_schedule(t, wq[2:5], x[1:2], K)), bits(y[1:2, 2:5]))
        assert np.any(y != 0)


def test_random_blocks_hold_the_specials():
    for t in TYPES:
        wq = R.random_blocks(np.random.default_rng([0x51, 1]), 5, 256, R.has_qh(t), R.has_min(t))
        assert wq.shape == (5, 8 * R.block_bytes(t))
        b = wq.reshape(40, R.block_bytes(t))
        dbits = b[:, 0:2].copy().view("<u2")[:, 0]
        assert {0x0000, 0x8000, 0x0001, 0x83FF} <= set(dbits.tolist())
        o = 2 + 2 * R.has_min(t)
        if R.has_qh(t):
            qh = b[:, o:o + 4].copy().view("<u4")[:, 0]
            assert set(R.SPECIAL_QH) <= set(qh.tolist())
            o += 4
        for v in (0x00, 0xFF, 0xF0):
            assert (b[:, o:] == v).all(axis=1).any()
        assert np.isfinite(R.dequantize(t, wq, 256)).all()


def test_fixture_sizes():
    total = 0
    for t in TYPES:
        for entry in manifest(t).values():
            n = os.path.getsize(os.path.join(GOLDEN, entry["file"]))
            assert n == entry["bytes"] <= 147456
            total += n
    assert total < 1_500_000


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(LIB_PATH):
        subprocess.check_call(["make", "-s", "-C", PKG, "-j4"])
    return ggml_hip.load()


@pytest.fixture
def lib(built):
    L = built
    exact, min_n = L.ggml_hip_get_exact(), L.ggml_hip_debug_set_q5_0_gemm_min_n(-1)
    env = os.environ.pop("GGML_HIP_Q5_0_GEMM_MIN_N", None)
    L.ggml_hip_set_exact(0)
    yield L
    os.environ.pop("GGML_HIP_Q5_0_GEMM_MIN_N", None)
    if env is not None:
        os.environ["GGML_HIP_Q5_0_GEMM_MIN_N"] = env
    L.ggml_hip_debug_set_q5_0_gemm_min_n(min_n)
    L.ggml_hip_set_exact(exact)


def test_auto_algo_rule(lib):
    lib.ggml_hip_debug_set_q5_0_gemm_min_n(-1)
    min_n = lib.ggml_hip_debug_set_q5_0_gemm_min_n(-1)      # the default (no environment value)
    assert min_n >= 9
    auto = lib.ggml_hip_debug_q5_0_auto_algo
    for N in (1, 8, min_n - 1):
        assert auto(4096, 4096, N) == 1
    for N in (min_n, min_n + 1, 512):
        assert auto(4096, 4096, N) == 2
    assert auto(11008, 4096, 1) == 1 and auto(64, 1, 1) == 1
    assert auto(52416, 4, 1) == 1 and auto(52480, 4, 1) == 2          # 1638 blocks fit the GEMV's LDS, 1640 do not
    for name in ("q4_1", "q5_1"):                                      # no GEMM: the GEMV at every N, exact past its K
        auto = getattr(lib, f"ggml_hip_debug_{name}_auto_algo")
        for N in (1, 8, min_n, 512, 100000):
            assert auto(4096, 4096, N) == 1
        assert auto(52416, 4, 1) == 1 and auto(52480, 4, 1) == 4 and auto(52480, 4, 512) == 4
    lib.ggml_hip_set_exact(1)
    for name in NAME.values():
        auto = getattr(lib, f"ggml_hip_debug_{name}_auto_algo")
        for K, N in ((4096, 1), (4096, 512), (64, 9)):
            assert auto(K, 100, N) == 4
    lib.ggml_hip_set_exact(0)
    for name in NAME.values():
        auto = getattr(lib, f"ggml_hip_debug_{name}_auto_algo")
        assert auto(96, 4, 1) == ggml_hip.ERR_INVALID             # K % 64
        assert auto(4096, 0, 1) == ggml_hip.ERR_INVALID


def test_min_n_setter_and_environment(lib):
    auto, setter = lib.ggml_hip_debug_q5_0_auto_algo, lib.ggml_hip_debug_set_q5_0_gemm_min_n
    default = setter(100)
    assert setter(100) == 100                               # returns the previous value
    assert auto(4096, 64, 99) == 1 and auto(4096, 64, 100) == 2
    assert lib.ggml_hip_debug_q5_1_auto_algo(4096, 64, 100) == 1
    assert setter(3) == 100 and setter(-1) == 9             # never below 9
    assert setter(-1) == default
    os.environ["GGML_HIP_Q5_0_GEMM_MIN_N"] = "77"
    setter(-1)                                              # re-reads the environment
    assert setter(-1) == 77
    assert auto(4096, 64, 76) == 1 and auto(4096, 64, 77) == 2
    del os.environ["GGML_HIP_Q5_0_GEMM_MIN_N"]
    setter(-1)
    assert setter(-1) == default
    q8 = lib.ggml_hip_debug_set_q8_0_gemm_min_n(-1)         # Q8_0's threshold is its own
    setter(50)
    assert lib.ggml_hip_debug_set_q8_0_gemm_min_n(-1) == q8
    setter(-1)


@pytest.mark.parametrize("t", TYPES)
def test_tensor_without_device_is_declined_on_full_host_copy(built, t):
    """No HIP device: can_mul_mat declines a weight of the type, and ggml_hip_transform_tensor leaves it on the CPU on
    a host copy of all B * K / 32 * M bytes (the loader may free its buffer after the call)."""
    lib = built
    if lib.ggml_hip_device_count() > 0:
        pytest.skip("a HIP device is present")
    K, M, B = 2304, 24, R.block_bytes(t)
    src = np.ascontiguousarray(load(t, f"w{K}_q"))
    nbytes = B * K // 32 * M
    assert src.nbytes == nbytes
    staged = src.copy()
    w = ggml_hip.make_tensor(R.TYPES[t][0], (K, M), backend=ggml_hip.GGML_BACKEND_GPU_SPLIT)
    assert (w.nb[0], w.nb[1]) == (B, B * K // 32)
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


NEW_SYMBOLS = tuple(f"ggml_hip_{kind}_{n}" for n in NAME.values() for kind in ("mul_mat", "dequantize")) + \
    tuple(f"ggml_hip_debug_{n}_auto_algo" for n in NAME.values()) + \
    ("ggml_hip_quantize_q8_1", "ggml_hip_debug_set_q5_0_gemm_min_n")


def test_new_symbols_in_header_exports_and_binding(built):
    header = open(os.path.join(ROOT, "include", "ggml-hip.h")).read()
    exports = open(os.path.join(PKG, "exports.map")).read()
    assert re.search(r"global:\s*ggml_\*;", exports)        # every ggml_* name is exported, nothing else
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert getattr(built, name).argtypes is not None, name     # bound with a signature (and exported)
    assert getattr(built, "ggml_hip_debug_set_q5x_gemv_policy").argtypes is not None
    assert (ggml_hip.GGML_TYPE_Q4_1, ggml_hip.GGML_TYPE_Q5_0, ggml_hip.GGML_TYPE_Q5_1) == (3, 6, 7)
    for n in NAME.values():
        assert callable(getattr(ggml_hip, "mul_mat_" + n)) and callable(getattr(ggml_hip, "dequantize_" + n))
    assert callable(ggml_hip.quantize_q8_1)
    src = open(os.path.join(PKG, "csrc", "ggml_abi.h")).read()
    for pat in (r"\bTYPE_Q4_1 = 3\b", r"\bTYPE_Q5_0 = 6\b", r"\bTYPE_Q5_1 = 7\b", r"\{\s*3,\s*20,\s*32\s*\}",
                r"\{\s*6,\s*22,\s*32\s*\}", r"\{\s*7,\s*24,\s*32\s*\}"):
        assert re.search(pat, src), pat
