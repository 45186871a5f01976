"""F32 WEIGHTS x F32 mul_mat on the device through ggml_hip_mul_mat_f32 (csrc/f32_w.hip and the ROW_F32 row): the GEMV
(algo 1) bit for bit its numpy restatement (tests/f32w_ref.py gemv_schedule) on one ragged step, 256 + 32, two steps,
column tiles 8 + 8 + 1 and the 43 steps of K = 11008, with a row pitch and with special values; a column's bits
independent of its place; the exact kernel (algo 4) bit for bit ggml_vec_dot_f32's AVX2 schedule; every fast result
within the derived bound 1.01 K 2^-24 sum|w x| of the float64 sum; the auto rule on the device; guard bytes for algos
1, 4 and 12; status codes."""
import numpy as np
import pytest

import f32w_ref as R
import ggml_ops_ref as G
from hip_env import ggml_hip, gpu_available

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason="needs a HIP device and libggml_hip.so")]

DB = ggml_hip.DeviceBuffer
GEMV, EXACT, GEMM = 1, 4, 12
NG = len(R.GEMV_CASES)
IDS = ["K%d_M%d_N%d%s%s" % (c[0], c[1], c[2], "_ldy" if c[3] else "", "_special" if c[4] else "") for c in R.CASES]


def assert_bitwise(got, ref):
    diff = np.flatnonzero(G.bits(got).ravel() != G.bits(ref).ravel())
    assert diff.size == 0, f"{diff.size} of {got.size} differ; first at {diff[:4]}: {np.ravel(got)[diff[:4]]} vs " \
                           f"{np.ravel(ref)[diff[:4]]}"


def assert_within_bound(y, w, x):
    s64, sab = R.exact_terms(w, x)
    err = np.abs(y.astype(np.float64) - s64)
    lim = R.bound(w.shape[1], sab)
    print("max err / bound", float((err / (lim + 1e-300)).max()))
    assert np.isfinite(y).all()
    assert (err <= lim).all()


def gpu_mul_mat(w, x, algo, ldy=None, fill=0.0):
    M, K = w.shape
    N = x.shape[0]
    ld = M if ldy is None else ldy
    wd, xd = DB.from_array(w), DB.from_array(x)
    yd = DB.from_array(np.full((N, ld), np.float32(fill), np.float32))
    ggml_hip.mul_mat_f32(wd, K, M, xd, N, yd, algo=algo, ldy=ld)
    y = yd.download((N, ld), np.float32)
    for b in (wd, xd, yd):
        b.free()
    return y


@pytest.fixture
def exact_off():
    L = ggml_hip.load()
    prev = L.ggml_hip_get_exact()
    L.ggml_hip_set_exact(0)
    yield L
    L.ggml_hip_set_exact(prev)


@pytest.mark.parametrize("i", range(NG), ids=IDS[:NG])
def test_gemv_bitwise_the_restatement(exact_off, i):
    """(the special case holds a row whose only product is 2^-130 * 2^20: it survives only if subnormals are kept)"""
    K, M, N, pad, special = R.CASES[i]
    w, x = R.case(i)
    y = gpu_mul_mat(w, x, GEMV, ldy=M + pad, fill=2.5)
    assert_bitwise(y[:, :M], R.ref(i, "gemv"))
    assert (y[:, M:] == 2.5).all()                           # y beyond column M of each row is not written
    assert_within_bound(y[:, :M], w, x)
    if special:
        assert (y[:, 0] == np.float32(2.0 ** -110)).all()


def test_column_bits_do_not_depend_on_its_place(exact_off):
    """column j of an N = 17 call (tiles of 8, 8 and a ragged 1) = the N = 1 call on that column, and = its place in
    another tiling (the first 9 columns: 8 + 1)"""
    i = 3                                                    # K = 1504, M = 65, N = 17
    w, x = R.case(i)
    y17 = gpu_mul_mat(w, x, GEMV)
    assert_bitwise(y17, R.ref(i, "gemv"))
    for j in (0, 7, 8, 15, 16):
        assert_bitwise(gpu_mul_mat(w, x[j:j + 1], GEMV), y17[j:j + 1])
    assert_bitwise(gpu_mul_mat(w, x[:9], GEMV), y17[:9])
    assert_bitwise(gpu_mul_mat(w[20:23], x, GEMV), y17[:, 20:23])       # nor on M or the row's place


@pytest.mark.parametrize("i", [0, 3, 5, 4], ids=[IDS[i] for i in (0, 3, 5, 4)])
def test_exact_bitwise_vec_dot_f32(exact_off, i):
    """N = 1, N = 17, the special values, K = 11008; with a row pitch"""
    K, M, N, _, _ = R.CASES[i]
    w, x = R.case(i)
    y = gpu_mul_mat(w, x, EXACT, ldy=M + 1, fill=-1.5)
    assert_bitwise(y[:, :M], R.ref(i, "exact"))
    assert (y[:, M:] == -1.5).all()


def test_auto_on_the_device(exact_off):
    L = exact_off
    prev = L.ggml_hip_debug_set_f32w_gemm_min_n(17)
    try:
        i = 3                                                # K = 1504, M = 65, N = 17
        w, x = R.case(i)
        assert L.ggml_hip_debug_f32w_auto_algo(1504, 65, 16) == GEMV
        assert_bitwise(gpu_mul_mat(w, x[:16], 0), R.ref(i, "gemv")[:16])     # below the threshold
        assert L.ggml_hip_debug_f32w_auto_algo(1504, 65, 17) == GEMM
        assert_bitwise(gpu_mul_mat(w, x, 0), gpu_mul_mat(w, x, GEMM))        # at the threshold
        assert (G.bits(gpu_mul_mat(w, x, GEMM)) != G.bits(R.ref(i, "gemv"))).any()
        L.ggml_hip_set_exact(1)
        assert_bitwise(gpu_mul_mat(w, x, 0), R.ref(i, "exact"))
        assert_bitwise(gpu_mul_mat(w, x[:1], 0), R.ref(i, "exact")[:1])
        L.ggml_hip_set_exact(0)
        # a K the GEMV cannot take (one column's floats past the LDS): the exact kernel
        big = 32768 + 32
        assert L.ggml_hip_debug_f32w_auto_algo(big, 2, 1) == EXACT
        wb, xb = R.random_case(np.random.default_rng([0xF32, 77]), 2, big, 1)
        assert_bitwise(gpu_mul_mat(wb, xb, 0), R.mul_mat_f32(wb, xb))
    finally:
        L.ggml_hip_debug_set_f32w_gemm_min_n(prev)


@pytest.mark.parametrize("algo", [GEMV, EXACT, GEMM])
def test_guard_bytes(exact_off, algo):
    """w, x and y inside one buffer each with 4 KiB of a fixed pattern on both sides: the patterns stay, y's pitch
    columns stay, and poisoned guards (NaN floats around w and x) do not reach y"""
    L = exact_off
    K, M, N = 1600, 65, 9                                    # 6 steps of 256 and a ragged 64; 50 chunks: 2 slices of 25
    w, x = R.random_case(np.random.default_rng([0xF32, 99]), M, K, N)
    G4 = 4096
    ld = M + 3
    wb = np.full(G4 // 4 + M * K + G4 // 4, np.nan, np.float32)
    wb[G4 // 4:G4 // 4 + M * K] = w.ravel()
    xb = np.full(G4 // 4 + N * K + G4 // 4, np.nan, np.float32)
    xb[G4 // 4:G4 // 4 + N * K] = x.ravel()
    yb = np.full(G4 // 4 + N * ld + G4 // 4, -7.25, np.float32)
    wd, xd, yd = DB.from_array(wb), DB.from_array(xb), DB.from_array(yb)
    prev = L.ggml_hip_debug_set_f32w_gemm_ksplit(2)
    try:
        ggml_hip.mul_mat_f32(wd, K, M, xd, N, yd, algo=algo, ldy=ld, w_off=G4, x_off=G4, y_off=G4)
    finally:
        L.ggml_hip_debug_set_f32w_gemm_ksplit(prev)
    assert np.array_equal(G.bits(wd.download(wb.shape, np.float32)), G.bits(wb))
    assert np.array_equal(G.bits(xd.download(xb.shape, np.float32)), G.bits(xb))
    got = yd.download(yb.shape, np.float32)
    assert (got[:G4 // 4] == -7.25).all() and (got[-G4 // 4:] == -7.25).all()
    y = got[G4 // 4:-G4 // 4].reshape(N, ld)
    assert (y[:, M:] == -7.25).all()
    assert np.isfinite(y[:, :M]).all()
    ref = {GEMV: R.gemv_schedule, EXACT: R.mul_mat_f32, GEMM: lambda a, b: R.gemm_schedule(a, b, 2)}[algo](w, x)
    assert_bitwise(y[:, :M], ref)
    for b in (wd, xd, yd):
        b.free()


def test_status_codes(exact_off):
    L = exact_off
    K, M, N = 64, 4, 2
    wd, xd, yd = DB(M * K * 4 + 64), DB(N * K * 4), DB(N * (M + 1) * 4)
    call = lambda *a: L.ggml_hip_mul_mat_f32(*a)
    ok, inv, uns = ggml_hip.OK, ggml_hip.ERR_INVALID, ggml_hip.ERR_UNSUPPORTED
    for algo in (0, GEMV, EXACT, GEMM):
        assert call(wd.ptr, K, M, xd.ptr, N, yd.ptr, M, algo, None) == ok
        assert call(wd.ptr, K, M, xd.ptr, N, yd.ptr, M + 1, algo, None) == ok       # every algo has a row pitch
        assert call(wd.ptr, 48, M, xd.ptr, N, yd.ptr, M, algo, None) == inv         # K % 32
        assert call(wd.ptr + 4, K, M, xd.ptr, N, yd.ptr, M, algo, None) == inv      # w off its 16-byte alignment
        assert call(wd.ptr, K, M, xd.ptr, N, yd.ptr, M - 1, algo, None) == inv      # ldy < M
        assert call(wd.ptr, K, M, xd.ptr, 0, yd.ptr, M, algo, None) == ok           # N == 0: nothing to do
    for algo in (2, 3, 5, 6, 7, 8, 9, 10, 11, 13):
        assert call(wd.ptr, K, M, xd.ptr, N, yd.ptr, M, algo, None) == inv
        assert call(wd.ptr, K, M, xd.ptr, 0, yd.ptr, M, algo, None) == inv          # refused first, an empty call too
    assert call(None, K, M, xd.ptr, N, yd.ptr, M, GEMV, None) == inv
    # a K whose single column does not fit the GEMV's LDS: algo 1 says so
    big = 32768 + 32
    wb, xb = DB(big * 4), DB(big * 4)
    assert call(wb.ptr, big, 1, xb.ptr, 1, yd.ptr, 1, GEMV, None) == uns
    assert b"GEMV" in L.ggml_hip_last_error()
    ggml_hip.check(L.ggml_hip_device_synchronize(), "sync")
    for b in (wd, xd, yd, wb, xb):
        b.free()
