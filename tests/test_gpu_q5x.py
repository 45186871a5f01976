"""Q4_1 / Q5_0 / Q5_1 WEIGHTS x F32 mul_mat on the device (csrc/blk32_w.hip): exact mode bit-identical to the reference's
AVX2 ggml_vec_dot_q4_1_q8_1 / _q5_0_q8_0 / _q5_1_q8_1, the fused GEMV within the parity bound under every launch
policy and tiling, Q5_0's per-call int8 image + k_gemm8 prefill path (bitwise Q8_0's on equal values), the
dequantizers and the q8_1 quantizer, graph capture, status codes and the ggml hook path on hand-built tensors.
References: the fixtures the compiled reference wrote (tests/golden/{q41,q50,q51}_*) and their numpy restatement
tests/q5x_ref.py; weights beyond the fixtures come from the restated reference quantizers."""
import ctypes
import functools

import numpy as np
import pytest

import oracle as O
import q5x_ref as R
import q8_0w_ref as R8
from golden_io import load
from hip_env import ggml_hip, gpu_available
from parity import check_y

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason="needs a HIP device and libggml_hip.so")]

DB = ggml_hip.DeviceBuffer
KS = (64, 2304, 4160)
GEMV, GEMM, EXACT = 1, 2, 4
TYPES = R.VARIANTS
NAME = {"q41": "q4_1", "q50": "q5_0", "q51": "q5_1"}
GTYPE = {t: R.TYPES[t][0] for t in TYPES}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_bitwise(got, ref):
    diff = np.flatnonzero(bits(got).ravel() != bits(ref).ravel())
    assert diff.size == 0, f"{diff.size} of {got.size} differ; first at {diff[:4]}: {np.ravel(got)[diff[:4]]} vs " \
                           f"{np.ravel(ref)[diff[:4]]}"


def rng_for(*key):
    return np.random.default_rng([0x51, *key])


def quantized_weights(t, rng, M, K):
    """Rows of N(0, 0.02) weights through the restated reference quantizer of the type."""
    return np.ascontiguousarray(R.quantize_w(t, (rng.standard_normal((M, K)) * 0.02).astype(np.float32)))


def split(t, wq, x, K):
    """(y_ref f32 [N, M], S_abs f64 [N, M], y_exact f64 [N, M]) of the weights against the quantized x: y_ref is the
    restatement of the reference's AVX2 vec_dot, S_abs = sum_b (|d_w d_x isum_b| + |m_w s_b|)."""
    xq = R.quantize_x(t, x)
    y_exact, s_abs = R.block_terms(t, wq, xq, K)
    return R.vec_dot_avx2(t, wq, xq, K), s_abs, y_exact


def gpu_mul_mat(t, wq, K, x, algo=0, ldy=None, fill=None, w_off=0):
    M, N = wq.shape[0], x.shape[0]
    ld = M if ldy is None else ldy
    if w_off:
        host = np.zeros(w_off + wq.nbytes + 64, np.uint8)
        host[w_off:w_off + wq.nbytes] = wq.ravel()
        wd = DB.from_array(host)
    else:
        wd = DB.from_array(wq)
    xd = DB.from_array(x)
    yd = DB.from_array(np.full((N, ld), np.float32(0 if fill is None else fill), np.float32))
    getattr(ggml_hip, "mul_mat_" + NAME[t])(wd, K, M, xd, N, yd, algo=algo, ldy=ld, w_off=w_off)
    return yd.download((N, ld), np.float32)


@pytest.fixture
def exact_off():
    L = ggml_hip.load()
    prev = L.ggml_hip_get_exact()
    L.ggml_hip_set_exact(0)
    yield L
    L.ggml_hip_set_exact(prev)


@pytest.fixture
def policy():
    L = ggml_hip.load()
    yield lambda mp, depth, wg: ggml_hip.check(L.ggml_hip_debug_set_q5x_gemv_policy(mp, depth, wg), "policy")
    L.ggml_hip_debug_set_q5x_gemv_policy(-1, 0, 0)


# ---- exact mode -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("t", TYPES)
def test_exact_fixture_bitwise(exact_off, t, K):
    wq, x, y = load(t, f"w{K}_q"), load(t, f"x{K}_f32"), load(t, f"y{K}_vec_dot")
    assert_bitwise(gpu_mul_mat(t, wq, K, x, algo=EXACT), y)                    # N = 3
    assert_bitwise(gpu_mul_mat(t, wq, K, x[:1], algo=EXACT), y[:1])            # N = 1
    assert_bitwise(y, R.vec_dot_avx2(t, wq, load(t, f"x{K}_q"), K))            # the restatement
    exact_off.ggml_hip_set_exact(1)
    assert_bitwise(gpu_mul_mat(t, wq, K, x, algo=0), y)


@pytest.mark.parametrize("t", TYPES)
def test_exact_crafted_blocks_bitwise(exact_off, t):
    wq, x, y = load(t, "craft_q"), load(t, "craft_x_f32"), load(t, "craft_y")
    assert_bitwise(gpu_mul_mat(t, wq, 64, x, algo=EXACT), y)
    assert_bitwise(gpu_mul_mat(t, wq, 64, x[2:3], algo=EXACT), y[2:3])


@pytest.mark.parametrize("t", TYPES)
def test_exact_long_row_bitwise(exact_off, t):
    K, M, N = 11008, 5, 3
    rng = rng_for(1, GTYPE[t])
    wq = quantized_weights(t, rng, M, K)
    x = rng.standard_normal((N, K)).astype(np.float32)
    y_ref = R.vec_dot_avx2(t, wq, R.quantize_x(t, x), K)
    assert_bitwise(gpu_mul_mat(t, wq, K, x, algo=EXACT), y_ref)
    assert_bitwise(gpu_mul_mat(t, wq, K, x[:1], algo=EXACT), y_ref[:1])


@pytest.mark.parametrize("t", TYPES)
def test_exact_full_range_blocks_bitwise(exact_off, t):
    K, M, N = 2304, 33, 9
    rng = rng_for(2, GTYPE[t])
    wq = R.random_blocks(rng, M, K, R.has_qh(t), R.has_min(t))
    x = rng.standard_normal((N, K)).astype(np.float32)
    y = gpu_mul_mat(t, wq, K, x, algo=EXACT, ldy=40, fill=2.5)
    assert np.all(y[:, M:] == np.float32(2.5))
    assert_bitwise(y[:, :M], R.vec_dot_avx2(t, wq, R.quantize_x(t, x), K))


# ---- GEMV -------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def gemv_pin_case(t, K, M):
    """Weights (quantized rows, the first min(M // 2, 64) of them full-range blocks with the crafted ones), 9
    activation rows and the restated GEMV order on them: computed once per type and shape, shared by the token
    counts."""
    rng = rng_for(20, GTYPE[t], K, M)
    wq = quantized_weights(t, rng, M, K)
    ns = min(M // 2, 64)
    if ns:
        wq[:ns] = R.random_blocks(rng, ns, K, R.has_qh(t), R.has_min(t), special=True)
    x = rng.standard_normal((9, K)).astype(np.float32)
    y = R.gemv_schedule(t, wq, x, K)
    for a in (wq, x, y):
        a.setflags(write=False)
    return wq, x, y


@pytest.mark.parametrize("N", [1, 3, 8, 9])
@pytest.mark.parametrize("K,M", [(64, 1), (64, 8209), (4160, 33)])
@pytest.mark.parametrize("t", TYPES)
def test_gemv_bitwise_restated_schedule(exact_off, t, K, M, N):
    """algo = GEMV is bitwise q5x_ref.gemv_schedule.  K = 64: one pair and 63 idle lanes; 4160: 65 pairs, a second
    chunk of one pair; M = 8209 at K = 64: more rows than waves under the auto grid rule, so the ring crosses
    row ends; M = 33: the last workgroup holds one row; N = 8: the full token tile, 9: a tile of 8 and one of 1."""
    wq, x, y_ref = gemv_pin_case(t, K, M)
    assert_bitwise(gpu_mul_mat(t, wq, K, x[:N], algo=GEMV), y_ref[:N])


@functools.lru_cache(maxsize=None)
def gemv_case(t, K):
    """Weights (130 rows, the crafted rows first at K = 64), 8 activation rows, and their reference: computed once
    per type and K and shared by the GEMV tests."""
    rng = rng_for(3, GTYPE[t], K)
    wq = quantized_weights(t, rng, 130, K)
    x = rng.standard_normal((8, K)).astype(np.float32)
    if K == 64:
        wq[:7] = load(t, "craft_q")
        x[6:8] = load(t, "craft_x_f32")[1:3]
    y_ref, s_abs, _ = split(t, wq, x, K)
    for a in (wq, x, y_ref, s_abs):
        a.setflags(write=False)
    return wq, x, y_ref, s_abs


@pytest.mark.parametrize("K,M", [(K, M) for K in (64, 4096, 4160, 11008) for M in (1, 65, 130)])
@pytest.mark.parametrize("t", TYPES)
def test_gemv_within_parity_bound(exact_off, t, K, M):
    """N = 1, 2, 8; the project's bound 1e-3 |y| + 1e-6 S_abs against the AVX2 restatement.  K = 64: one pair; 4096:
    one full wave-load; 4160: 65 pairs; 11008: two full loads and a ragged tail (and token tiles of 4).  M = 1, 65,
    130: ragged waves and more than one workgroup."""
    wq, x, y_ref, s_abs = gemv_case(t, K)
    for N in (1, 2, 8):
        y = gpu_mul_mat(t, np.ascontiguousarray(wq[:M]), K, x[:N], algo=GEMV, ldy=M + 3, fill=-7.5)
        assert np.all(y[:, M:] == np.float32(-7.5))                          # ldy > M: the gap untouched
        check_y(y[:, :M], y_ref[:N, :M], s_abs[:N, :M], rtol=1e-3, atol_blocks=1e-6)


@pytest.mark.parametrize("t", TYPES)
def test_gemv_mean_shifted_activations_against_exact_value(exact_off, t):
    """x ~ N(1, 1): with a minimum the d * isum and m * s sums are large and opposite.  Checked against the exact
    value (f64) of the quantized operands with the same bound: the reference's own two separate chains are up to a
    third of the bound away from it on such inputs by their own rounding, the GEMV's adjacent pair of terms is not."""
    K, M, N = 4096, 65, 8
    rng = rng_for(4, GTYPE[t])
    wq = quantized_weights(t, rng, M, K)
    x = (rng.standard_normal((N, K)) + 1.0).astype(np.float32)
    _, s_abs, y_exact = split(t, wq, x, K)
    check_y(gpu_mul_mat(t, wq, K, x, algo=GEMV), y_exact, s_abs, rtol=1e-3, atol_blocks=1e-6)


@pytest.mark.parametrize("off", [4, 8, 12])
@pytest.mark.parametrize("t", TYPES)
def test_weight_base_offset_in_allocation(exact_off, t, off):
    """The weight at 4, 8 and 12 bytes inside a larger allocation, K = 64: nothing relies on more than 4-byte
    alignment, in the GEMV and in the exact kernel."""
    K, M = 64, 37
    wq, x, y_ref, s_abs = gemv_case(t, K)
    w = np.ascontiguousarray(wq[:M])
    base = gpu_mul_mat(t, w, K, x, algo=GEMV)
    check_y(base, y_ref[:, :M], s_abs[:, :M], rtol=1e-3, atol_blocks=1e-6)
    assert_bitwise(gpu_mul_mat(t, w, K, x, algo=GEMV, w_off=off), base)
    assert_bitwise(gpu_mul_mat(t, w, K, x[:3], algo=EXACT, w_off=off), gpu_mul_mat(t, w, K, x[:3], algo=EXACT))
    assert_bitwise(gpu_mul_mat(t, w, K, x[:3], algo=EXACT, w_off=off), y_ref[:3, :M])


@pytest.mark.parametrize("K", [64, 4160, 11008])
@pytest.mark.parametrize("t", TYPES)
def test_gemv_launch_policies_bitwise(exact_off, policy, t, K):
    wq, x, _, _ = gemv_case(t, K)
    ref = {N: gpu_mul_mat(t, wq, K, x[:N], algo=GEMV) for N in (1, 3)}
    for mp, depth, wg in ((0, 1, 1), (1, 2, 2), (2, 1, 2), (2, 2, 1), (1, 1, 1)):
        policy(mp, depth, wg)
        for N in (1, 3):
            assert_bitwise(gpu_mul_mat(t, wq, K, x[:N], algo=GEMV), ref[N])


@pytest.mark.parametrize("N", [9, 17])
@pytest.mark.parametrize("t", TYPES)
def test_gemv_column_tiles_bitwise_per_tile_calls(exact_off, t, N):
    K, M = 4160, 37
    rng = rng_for(5, GTYPE[t], N)
    wq = quantized_weights(t, rng, M, K)
    x = rng.standard_normal((N, K)).astype(np.float32)
    y = gpu_mul_mat(t, wq, K, x, algo=GEMV)
    for n0 in range(0, N, 8):
        assert_bitwise(y[n0:n0 + 8], gpu_mul_mat(t, wq, K, x[n0:n0 + 8], algo=GEMV))
    y_ref, s_abs, _ = split(t, wq, x, K)
    check_y(y, y_ref, s_abs, rtol=1e-3, atol_blocks=1e-6)


@pytest.mark.parametrize("t", TYPES)
def test_doubling_x_doubles_y_bitwise(exact_off, t):
    K, M, N = 4160, 50, 3
    rng = rng_for(6, GTYPE[t])
    wq = quantized_weights(t, rng, M, K)
    x = rng.standard_normal((N, K)).astype(np.float32)
    for algo in (GEMV, EXACT) + ((GEMM,) if t == "q50" else ()):
        assert_bitwise(gpu_mul_mat(t, wq, K, 2 * x, algo=algo), 2 * gpu_mul_mat(t, wq, K, x, algo=algo))


# ---- Q5_0 GEMM ----------------------------------------------------------------------------------------------

def q5_0_as_q8_0(wq, K):
    """A Q5_0 matrix as Q8_0 rows with the same values: qs = q - 16 in element order, the same fp16 d."""
    d, _, q = R.split("q50", wq, K)
    M, nb = d.shape
    out = np.empty((M, nb, 34), np.uint8)
    out[:, :, 0:2] = np.ascontiguousarray(wq).reshape(M, nb, 22)[:, :, 0:2]
    out[:, :, 2:] = (q - 16).astype(np.int8).view(np.uint8)
    return out.reshape(M, nb * 34)


@pytest.mark.parametrize("K,N", [(K, N) for K in (64, 4160) for N in (9, 129)])
def test_q5_0_gemm_bitwise_q8_0_twin(exact_off, K, N):
    """A Q5_0 matrix and its Q8_0 twin give byte-identical k_gemm8 images, so algo 2 is bitwise
    ggml_hip_mul_mat_q8_0's.  M = 70: a ragged 64-row tile."""
    M = 70
    rng = rng_for(7, K, N)
    wq = R.random_blocks(rng, M, K, True, False) if K == 64 else quantized_weights("q50", rng, M, K)
    w8 = q5_0_as_q8_0(wq, K)
    assert np.array_equal(bits(R8.dequantize_q8_0(w8, K)), bits(R.dequantize("q50", wq, K)))
    x = rng.standard_normal((N, K)).astype(np.float32)
    y5 = gpu_mul_mat("q50", wq, K, x, algo=GEMM)
    w8d, xd, yd = DB.from_array(w8), DB.from_array(x), DB(N * M * 4)
    ggml_hip.mul_mat_q8_0(w8d, K, M, xd, N, yd, algo=GEMM)
    assert_bitwise(y5, yd.download((N, M), np.float32))
    assert np.any(y5 != 0)


@pytest.mark.parametrize("M,N", [(64, 9), (70, 130)])
def test_q5_0_gemm_full_range_within_parity_bound(exact_off, M, N):
    K = 4160
    rng = rng_for(8, M, N)
    wq = R.random_blocks(rng, M, K, True, False)
    x = rng.standard_normal((N, K)).astype(np.float32)
    x[0], x[1, ::2], x[1, 1::2] = 2.0, 2.0, -2.0                              # x at +-amax: every q = +-127
    y_ref, s_abs, _ = split("q50", wq, x, K)
    y = gpu_mul_mat("q50", wq, K, x, algo=GEMM, ldy=M + 5, fill=-7.5)
    assert np.all(y[:, M:] == np.float32(-7.5))
    check_y(y[:, :M], y_ref, s_abs, rtol=1e-3, atol_blocks=1e-6)


def test_q5_0_auto_switches_at_the_threshold(exact_off):
    L = exact_off
    K, M = 256, 70
    rng = rng_for(9)
    wq = quantized_weights("q50", rng, M, K)
    x = rng.standard_normal((12, K)).astype(np.float32)
    prev = L.ggml_hip_debug_set_q5_0_gemm_min_n(12)
    try:
        assert L.ggml_hip_debug_q5_0_auto_algo(K, M, 11) == GEMV and L.ggml_hip_debug_q5_0_auto_algo(K, M, 12) == GEMM
        assert L.ggml_hip_debug_q4_1_auto_algo(K, M, 12) == GEMV and L.ggml_hip_debug_q5_1_auto_algo(K, M, 512) == GEMV
        assert_bitwise(gpu_mul_mat("q50", wq, K, x[:11], algo=0), gpu_mul_mat("q50", wq, K, x[:11], algo=GEMV))
        assert_bitwise(gpu_mul_mat("q50", wq, K, x, algo=0), gpu_mul_mat("q50", wq, K, x, algo=GEMM))
    finally:
        L.ggml_hip_debug_set_q5_0_gemm_min_n(prev)


# ---- dequantize, quantize, capture, status ------------------------------------------------------------------

@pytest.mark.parametrize("t", TYPES)
def test_dequantize_bitwise(t):
    cases = [(K, load(t, f"w{K}_q"), load(t, f"w{K}_dequant")) for K in KS]
    cases.append((64, load(t, "craft_q"), load(t, "craft_dequant")))
    for K, wq, ref in cases:
        wq = np.ascontiguousarray(wq[:ref.shape[0]])
        wd, od = DB.from_array(wq), DB(ref.nbytes)
        getattr(ggml_hip, "dequantize_" + NAME[t])(wd, K, ref.shape[0], od)
        assert_bitwise(od.download(ref.shape, np.float32), ref)


def test_quantize_q8_1_bitwise():
    cases = [(K, load(t, f"x{K}_f32"), load(t, f"x{K}_q")) for K in KS for t in ("q41", "q51")]
    cases.append((64, load("q51", "craft_x_f32"), load("q51", "craft_x_q")))   # N(0, 1), +-amax, all +amax, zeros
    for K, x, ref in cases:
        xd, od = DB.from_array(x), DB(ref.nbytes)
        ggml_hip.quantize_q8_1(xd, K, x.shape[0], od)
        assert np.array_equal(od.download(ref.shape, np.uint8), ref)
    _, s, q = R.split_q8_1(load("q51", "craft_x_q"), 64)
    assert (q[2] == 127).all() and not q[3].any() and (s[3] == 0).all()


@pytest.mark.parametrize("t", TYPES)
def test_graph_capture_replays(exact_off, t):
    L = exact_off
    K, M, N = 2304, 70, 20
    rng = rng_for(10, GTYPE[t])
    wq = quantized_weights(t, rng, M, K)
    x = rng.standard_normal((N, K)).astype(np.float32)
    algo_n = GEMM if t == "q50" else GEMV
    mm = getattr(ggml_hip, "mul_mat_" + NAME[t])
    eager1, eagerN = gpu_mul_mat(t, wq, K, x[:1], algo=GEMV), gpu_mul_mat(t, wq, K, x, algo=algo_n)
    wd, xd, y1d, yNd = DB.from_array(wq), DB.from_array(x), DB(M * 4), DB(N * M * 4)
    ggml_hip.check(L.ggml_hip_reserve_workspace_mm(K, N, M), "reserve")
    s = L.ggml_hip_default_stream()
    g = ggml_hip.Graph(s)
    with g:
        mm(wd, K, M, xd, 1, y1d, algo=GEMV, stream=s)
        mm(wd, K, M, xd, N, yNd, algo=algo_n, stream=s)
    for _ in range(2):
        ggml_hip.check(L.ggml_hip_memset(y1d.ptr, 0xFF, M * 4, s))
        ggml_hip.check(L.ggml_hip_memset(yNd.ptr, 0xFF, N * M * 4, s))
        g.launch()
        ggml_hip.check(L.ggml_hip_stream_synchronize(s))
        assert_bitwise(y1d.download((1, M), np.float32), eager1)
        assert_bitwise(yNd.download((N, M), np.float32), eagerN)


@pytest.mark.parametrize("t", TYPES)
def test_status_codes(exact_off, t):
    L = exact_off
    b = DB(1 << 16)
    mm = getattr(L, "ggml_hip_mul_mat_" + NAME[t])
    dq = getattr(L, "ggml_hip_dequantize_" + NAME[t])
    valid = (0, 1, 2, 4) if t == "q50" else (0, 1, 4)
    assert mm(b.ptr, 96, 4, b.ptr, 1, b.ptr, 4, 0, None) == ggml_hip.ERR_INVALID        # K % 64
    assert mm(b.ptr, 32, 4, b.ptr, 1, b.ptr, 4, 0, None) == ggml_hip.ERR_INVALID
    assert dq(b.ptr, 48, 1, b.ptr, None) == ggml_hip.ERR_INVALID
    assert mm(b.ptr, 64, 4, b.ptr, 1, b.ptr, 3, 0, None) == ggml_hip.ERR_INVALID         # ldy < M
    for algo in [a for a in (2, 3, 5, 6, -1, 9) if a not in valid]:
        assert mm(b.ptr, 64, 4, b.ptr, 1, b.ptr, 4, algo, None) == ggml_hip.ERR_INVALID  # algo
    assert mm(None, 64, 4, b.ptr, 1, b.ptr, 4, 0, None) == ggml_hip.ERR_INVALID
    assert mm(b.ptr, 64, 4, b.ptr, 0, b.ptr, 4, 0, None) == ggml_hip.OK                  # N = 0
    for algo in (3, 5, 6, -1):
        assert mm(b.ptr, 64, 4, b.ptr, 0, b.ptr, 4, algo, None) == ggml_hip.OK           # N = 0 returns before the algo check
    assert mm(b.ptr, 64, 4, None, 1, b.ptr, 4, 0, None) == ggml_hip.ERR_INVALID
    assert mm(b.ptr, 64, 4, b.ptr, 1, None, 4, 0, None) == ggml_hip.ERR_INVALID
    assert mm(b.ptr, 64, 4, b.ptr + 4, 1, b.ptr, 4, 0, None) == ggml_hip.ERR_INVALID     # x not 16-byte aligned
    assert mm(b.ptr, 64, 4, b.ptr, 1, b.ptr + 2, 4, 0, None) == ggml_hip.ERR_INVALID     # y not 4-byte aligned
    assert mm(b.ptr + 2, 64, 4, b.ptr, 1, b.ptr, 4, 0, None) == ggml_hip.ERR_INVALID     # W not 4-byte aligned
    for algo in valid:
        assert mm(b.ptr, 64, 4, b.ptr, 1, b.ptr, 4, algo, None) == ggml_hip.OK
    assert L.ggml_hip_quantize_q8_1(b.ptr, 48, 1, b.ptr, None) == ggml_hip.ERR_INVALID
    assert L.ggml_hip_quantize_q8_1(b.ptr, 64, 1, b.ptr + 2, None) == ggml_hip.ERR_INVALID
    ggml_hip.synchronize()


@pytest.mark.parametrize("t", TYPES)
def test_k_past_the_gemv_lds(exact_off, t):
    """K = 52480: 1640 blocks, one token's 40 bytes per block are past the GEMV's 64 KiB of LDS.  Algo 1 is refused
    before any launch; auto runs the exact kernel (Q5_0: the GEMM)."""
    L = exact_off
    K, M = 52480, 3
    rng = rng_for(11, GTYPE[t])
    wq = quantized_weights(t, rng, M, K)
    x = rng.standard_normal((1, K)).astype(np.float32)
    wd, xd, yd = DB.from_array(wq), DB.from_array(x), DB(M * 4)
    mm = getattr(L, "ggml_hip_mul_mat_" + NAME[t])
    assert mm(wd.ptr, K, M, xd.ptr, 0, yd.ptr, M, 1, None) == ggml_hip.OK                # nothing to run
    assert mm(wd.ptr, K, M, xd.ptr, 1, yd.ptr, M, 1, None) == ggml_hip.ERR_UNSUPPORTED
    assert getattr(L, f"ggml_hip_debug_{NAME[t]}_auto_algo")(K, M, 1) == (GEMM if t == "q50" else EXACT)
    y = gpu_mul_mat(t, wq, K, x, algo=0)
    y_ref, s_abs, _ = split(t, wq, x, K)
    if t == "q50":
        check_y(y, y_ref, s_abs, rtol=1e-3, atol_blocks=1e-6)
    else:
        assert_bitwise(y, y_ref)


# ---- hook path ----------------------------------------------------------------------------------------------

def w_tensor(t, wq, K, M, backend=ggml_hip.GGML_BACKEND_CPU):
    return ggml_hip.make_tensor(GTYPE[t], (K, M), wq, backend=backend)


def mm_node(w, x_np, y_np):
    N, K = x_np.shape
    xt = ggml_hip.make_tensor(ggml_hip.GGML_TYPE_F32, (K, N), x_np)
    y = ggml_hip.make_tensor(ggml_hip.GGML_TYPE_F32, (y_np.shape[1], N), y_np)
    y.op = ggml_hip.GGML_OP_MUL_MAT
    y.src0 = ctypes.pointer(w)
    y.src1 = ctypes.pointer(xt)
    return y, xt


def forward(L, node):
    p = ggml_hip.GgmlComputeParams(ggml_hip.GGML_TASK_COMPUTE, 0, 1, 0, None)
    return L.ggml_hip_compute_forward(ctypes.byref(p), ctypes.byref(node))


def mul_mat_count(L):
    c = (ctypes.c_int64 * 68)()
    L.ggml_hip_debug_op_stats.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    L.ggml_hip_debug_op_stats(c, 68, 0)
    return c[ggml_hip.GGML_OP_MUL_MAT]


@pytest.mark.parametrize("t", TYPES)
def test_hook_can_mul_mat(exact_off, t):
    L = exact_off
    N, M = 64, 64
    B = R.block_bytes(t)
    K = 256                       # a large host weight at prefill and at decode (2^19 elements: the cache's threshold)
    w = w_tensor(t, np.zeros((2048, B * K // 32), np.uint8), K, 2048)
    assert (w.nb[0], w.nb[1]) == (B, B * K // 32)
    for n in (N, 1):
        y, xt = mm_node(w, np.zeros((n, K), np.float32), np.zeros((n, 2048), np.float32))
        assert L.ggml_hip_can_mul_mat(ctypes.byref(w), ctypes.byref(xt), ctypes.byref(y))
    K = 96                        # K % 64 != 0
    w = w_tensor(t, np.zeros((M, B * K // 32), np.uint8), K, M)
    y, xt = mm_node(w, np.zeros((N, K), np.float32), np.zeros((N, M), np.float32))
    assert not L.ggml_hip_can_mul_mat(ctypes.byref(w), ctypes.byref(xt), ctypes.byref(y))
    assert not forward(L, y)
    K = 128                       # non-contiguous src1
    w = w_tensor(t, np.zeros((M, B * K // 32), np.uint8), K, M)
    y, xt = mm_node(w, np.zeros((N, 2 * K), np.float32), np.zeros((N, M), np.float32))
    xt.ne[0] = K
    xt.nb[2] = xt.nb[3] = xt.nb[1] * N
    assert not L.ggml_hip_can_mul_mat(ctypes.byref(w), ctypes.byref(xt), ctypes.byref(y))
    assert not forward(L, y)
    xt.nb[1] = 4 * K
    xt.nb[2] = xt.nb[3] = xt.nb[1] * N
    assert L.ggml_hip_can_mul_mat(ctypes.byref(w), ctypes.byref(xt), ctypes.byref(y))


@pytest.mark.parametrize("backend", [ggml_hip.GGML_BACKEND_GPU, ggml_hip.GGML_BACKEND_GPU_SPLIT])
@pytest.mark.parametrize("N", [1, 33])
@pytest.mark.parametrize("t", TYPES)
def test_hook_transformed_weight(exact_off, t, backend, N):
    """A layer matrix's operand placement: weight uploaded by transform_tensor, host x, host dst; fast mode bitwise
    the tensor-free call, exact mode bitwise the restatement; free_data releases the upload."""
    L = exact_off
    K, M = 2304, 101
    rng = rng_for(12, GTYPE[t], N)
    wq = quantized_weights(t, rng, M, K)
    x = rng.standard_normal((N, K)).astype(np.float32)
    staged = wq.copy()
    w = w_tensor(t, staged, K, M, backend)
    L.ggml_hip_transform_tensor(staged.ctypes.data_as(ctypes.c_void_p), ctypes.byref(w))
    assert w.extra and w.backend == backend
    staged[:] = 0                                              # the loader frees its buffer
    y_np = np.zeros((N, M), np.float32)
    y, xt = mm_node(w, x, y_np)
    before = mul_mat_count(L)
    assert forward(L, y)
    assert mul_mat_count(L) == before + 1
    assert_bitwise(y_np, gpu_mul_mat(t, wq, K, x))
    L.ggml_hip_set_exact(1)
    y_np[:] = 0
    assert forward(L, y)
    assert_bitwise(y_np, R.vec_dot_avx2(t, wq, R.quantize_x(t, x), K))
    L.ggml_hip_free_data(ctypes.byref(w))
    assert not w.extra


@pytest.mark.parametrize("t", TYPES)
def test_hook_host_weight_residency_cache(exact_off, t):
    L = exact_off
    K, M = 256, 2048                                           # 2^19 elements: taken at N = 1
    rng = rng_for(13, GTYPE[t])
    wq = quantized_weights(t, rng, M, K)
    x = rng.standard_normal((1, K)).astype(np.float32)
    y_np = np.zeros((1, M), np.float32)
    w = w_tensor(t, wq, K, M)
    y, xt = mm_node(w, x, y_np)
    assert L.ggml_hip_can_mul_mat(ctypes.byref(w), ctypes.byref(xt), ctypes.byref(y))
    h, m, r = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    ggml_hip.check(L.ggml_hip_weight_cache_stats(ctypes.byref(h), ctypes.byref(m), ctypes.byref(r)))
    hits0, miss0 = h.value, m.value
    assert forward(L, y)
    ggml_hip.check(L.ggml_hip_weight_cache_stats(ctypes.byref(h), ctypes.byref(m), ctypes.byref(r)))
    assert (h.value, m.value) == (hits0, miss0 + 1)            # one miss ...
    first = y_np.copy()
    y_np[:] = 0
    assert forward(L, y)
    ggml_hip.check(L.ggml_hip_weight_cache_stats(ctypes.byref(h), ctypes.byref(m), ctypes.byref(r)))
    assert (h.value, m.value) == (hits0 + 1, miss0 + 1)        # ... then one hit
    assert_bitwise(y_np, first)
    assert_bitwise(y_np, gpu_mul_mat(t, wq, K, x))
    L.ggml_hip_weight_cache_invalidate(wq.ctypes.data_as(ctypes.c_void_p), wq.nbytes)


@pytest.mark.parametrize("t", TYPES)
def test_fusion_on_off_bitwise(exact_off, t):
    """A small graph on the device: a q4_0 mul_mat (held by the hook's scheduler when fusion is on), an add on its
    output, a mul_mat of the type on disjoint buffers, and a second q4_0 mul_mat after it.  The node of the type
    joins no group or chain; every output is bitwise the same with fusion on and off."""
    L = exact_off
    L.ggml_hip_debug_set_fuse.argtypes = [ctypes.c_int]
    GGML_OP_ADD = 2
    K, M4, M5 = 256, 48, 40
    rng = rng_for(14, GTYPE[t])
    w4q, _ = O.quantize_q4_0((rng.standard_normal((M4, K)) * 0.02).astype(np.float32))
    w4q = np.ascontiguousarray(w4q)
    w5q = quantized_weights(t, rng, M5, K)
    x4 = rng.standard_normal((1, K)).astype(np.float32)
    x5 = rng.standard_normal((1, K)).astype(np.float32)
    bias = rng.standard_normal((1, M4)).astype(np.float32)

    def run(fuse):
        ggml_hip.check(L.ggml_hip_debug_set_fuse(fuse))
        w4 = ggml_hip.make_tensor(ggml_hip.GGML_TYPE_Q4_0, (K, M4), w4q, backend=ggml_hip.GGML_BACKEND_GPU)
        L.ggml_hip_transform_tensor(w4q.ctypes.data_as(ctypes.c_void_p), ctypes.byref(w4))
        y4_host = np.zeros((1, M4), np.float32)
        y4, x4t = mm_node(w4, x4, y4_host)
        x4t.backend = ggml_hip.GGML_BACKEND_GPU
        L.ggml_hip_transform_tensor(x4.ctypes.data_as(ctypes.c_void_p), ctypes.byref(x4t))
        L.ggml_hip_assign_buffers_no_scratch(ctypes.byref(y4))
        assert y4.backend == ggml_hip.GGML_BACKEND_GPU and y4.extra
        bt = ggml_hip.make_tensor(ggml_hip.GGML_TYPE_F32, (M4, 1), bias, backend=ggml_hip.GGML_BACKEND_GPU)
        L.ggml_hip_transform_tensor(bias.ctypes.data_as(ctypes.c_void_p), ctypes.byref(bt))
        sum_host = np.zeros((1, M4), np.float32)
        st = ggml_hip.make_tensor(ggml_hip.GGML_TYPE_F32, (M4, 1), sum_host)
        st.op = GGML_OP_ADD
        st.src0, st.src1 = ctypes.pointer(y4), ctypes.pointer(bt)
        L.ggml_hip_assign_buffers_no_scratch(ctypes.byref(st))
        assert st.backend == ggml_hip.GGML_BACKEND_GPU and st.extra
        w5 = w_tensor(t, w5q, K, M5, ggml_hip.GGML_BACKEND_GPU)
        L.ggml_hip_transform_tensor(w5q.ctypes.data_as(ctypes.c_void_p), ctypes.byref(w5))
        y5_host = np.zeros((1, M5), np.float32)
        y5, _ = mm_node(w5, x5, y5_host)
        y4b_host = np.zeros((1, M4), np.float32)                # a q4_0 node after it, host dst
        y4b, x4bt = mm_node(w4, x4, y4b_host)
        assert forward(L, y4)
        assert forward(L, st)
        assert forward(L, y5)
        assert forward(L, y4b)
        for tt, host in ((y4, y4_host), (st, sum_host)):
            dev = ctypes.cast(tt.extra, ctypes.POINTER(ctypes.c_void_p * 16)).contents[0]
            ggml_hip.check(L.ggml_hip_memcpy_d2h(host.ctypes.data_as(ctypes.c_void_p), dev, host.nbytes, None))
        for tt in (st, y4, x4t, bt, w4, w5):
            L.ggml_hip_free_data(ctypes.byref(tt))
        return y4_host, sum_host, y5_host, y4b_host

    try:
        on = run(1)
        off = run(0)
    finally:
        L.ggml_hip_debug_set_fuse(1)
    for a, b in zip(on, off):
        assert_bitwise(a, b)
    assert_bitwise(on[2], gpu_mul_mat(t, w5q, K, x5))
    assert_bitwise(on[1], on[0] + bias)
    assert np.any(on[0] != 0)
