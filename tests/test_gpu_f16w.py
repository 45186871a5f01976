"""F16 WEIGHTS x F32 mul_mat on the device through ggml_hip_mul_mat_f16 (csrc/f16_w.hip and the ROW_F16 row): the GEMV
(algo 1) bit for bit its numpy restatement (tests/f16w_ref.py) on one ragged step, 512 + 32, two steps and a ragged
480 and the 21.5 steps of K = 11008, in column tiles and with a row pitch; a column's bits independent of its place;
exact mode (algo 4) bit for bit ggml_vec_dot_f16 (tests/ggml_ops_ref.py), the MFMA GEMM (algo 9) within the
fp32-accumulation bound; the auto rule on the device; guard bytes; status codes."""
import numpy as np
import pytest

import f16w_ref as R
import ggml_ops_ref as G
from hip_env import ggml_hip, gpu_available

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason="needs a HIP device and libggml_hip.so")]

DB = ggml_hip.DeviceBuffer
GEMV, EXACT, GEMM = 1, 4, 9
IDS = ["K%d_M%d_N%d%s%s" % (c[0], c[1], c[2], "_ldy" if c[3] else "", "_special" if c[4] else "") for c in R.CASES]


def assert_bitwise(got, ref):
    diff = np.flatnonzero(G.bits(got).ravel() != G.bits(ref).ravel())
    assert diff.size == 0, f"{diff.size} of {got.size} differ; first at {diff[:4]}: {np.ravel(got)[diff[:4]]} vs " \
                           f"{np.ravel(ref)[diff[:4]]}"


def gpu_mul_mat(w16, x, algo, ldy=None, fill=0.0):
    M, K = w16.shape
    N = x.shape[0]
    ld = M if ldy is None else ldy
    wd, xd = DB.from_array(w16), DB.from_array(x)
    yd = DB.from_array(np.full((N, ld), np.float32(fill), np.float32))
    ggml_hip.mul_mat_f16(wd, K, M, xd, N, yd, algo=algo, ldy=ld)
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


@pytest.mark.parametrize("i", range(len(R.CASES)), ids=IDS)
def test_gemv_bitwise_the_restatement(exact_off, i):
    K, M, N, pad, _ = R.CASES[i]
    w16, x, ref = R.case(i)
    y = gpu_mul_mat(w16, x, GEMV, ldy=M + pad, fill=2.5)
    assert_bitwise(y[:, :M], ref)
    assert (y[:, M:] == 2.5).all()                           # y beyond column M of each row is not written


def test_column_bits_do_not_depend_on_its_place(exact_off):
    """column j of an N = 17 call (tiles of 8, 8 and a ragged 1) = the N = 1 call on that column, and = its place in
    another tiling (the first 9 columns: 8 + 1)"""
    i = 6                                                    # K = 1504, M = 65, N = 17
    w16, x, ref = R.case(i)
    y17 = gpu_mul_mat(w16, x, GEMV)
    for j in (0, 7, 8, 15, 16):
        assert_bitwise(gpu_mul_mat(w16, x[j:j + 1], GEMV), y17[j:j + 1])
    assert_bitwise(gpu_mul_mat(w16, x[:9], GEMV), y17[:9])
    assert_bitwise(gpu_mul_mat(w16[20:23], x, GEMV), y17[:, 20:23])     # nor on M or the row's place


@pytest.mark.parametrize("i", [2, 6, 8, 10], ids=[IDS[i] for i in (2, 6, 8, 10)])
def test_exact_bitwise_vec_dot_f16_and_gemm_within_bound(exact_off, i):
    w16, x, _ = R.case(i)
    assert_bitwise(gpu_mul_mat(w16, x, EXACT), G.mul_mat_f16_f32(w16, x))
    y = gpu_mul_mat(w16, x, GEMM)
    ref, sab = R.exact_terms(w16, x)
    err = np.abs(y.astype(np.float64) - ref)
    assert np.isfinite(y).all()
    assert (err <= 1e-5 * sab + 1e-30).all(), float((err / (sab + 1e-30)).max())


def test_auto_on_the_device(exact_off):
    L = exact_off
    w16, x, ref = R.case(6)                                  # N = 17: below the GEMM threshold
    assert L.ggml_hip_debug_f16w_auto_algo(1504, 65, 17) == GEMV
    assert_bitwise(gpu_mul_mat(w16, x, 0), ref)
    assert_bitwise(gpu_mul_mat(w16, x[:1], 0), ref[:1])      # N = 1
    w40, x40, _ = R.case(1)                                  # N = 40: the GEMM
    assert L.ggml_hip_debug_f16w_auto_algo(32, 130, 40) == GEMM
    assert_bitwise(gpu_mul_mat(w40, x40, 0), gpu_mul_mat(w40, x40, GEMM))
    L.ggml_hip_set_exact(1)
    assert_bitwise(gpu_mul_mat(w16, x, 0), gpu_mul_mat(w16, x, EXACT))
    assert_bitwise(gpu_mul_mat(w16, x[:1], 0), G.mul_mat_f16_f32(w16, x[:1]))


@pytest.mark.parametrize("algo", [GEMV, EXACT, GEMM])
def test_guard_bytes(exact_off, algo):
    """w, x and y inside one buffer each with 4 KiB of a fixed pattern on both sides: the patterns stay, y's pitch
    columns stay (GEMV), and poisoned guards (NaN halves around w, NaN floats around x) do not reach y"""
    K, M, N = 1504, 65, 9
    w16, x = R.random_case(np.random.default_rng([0xF16, 99]), M, K, N)
    G4 = 4096
    ld = M + 3 if algo == GEMV else M
    wb = np.full(G4 // 2 + M * K + G4 // 2, 0x7E00, np.uint16)          # fp16 NaN
    wb[G4 // 2:G4 // 2 + M * K] = w16.ravel()
    xb = np.full(G4 // 4 + N * K + G4 // 4, np.nan, np.float32)
    xb[G4 // 4:G4 // 4 + N * K] = x.ravel()
    yb = np.full(G4 // 4 + N * ld + G4 // 4, -7.25, np.float32)
    wd, xd, yd = DB.from_array(wb), DB.from_array(xb), DB.from_array(yb)
    ggml_hip.mul_mat_f16(wd, K, M, xd, N, yd, algo=algo, ldy=ld, w_off=G4, x_off=G4, y_off=G4)
    assert np.array_equal(wd.download(wb.shape, np.uint16), wb)
    assert np.array_equal(G.bits(xd.download(xb.shape, np.float32)), G.bits(xb))
    got = yd.download(yb.shape, np.float32)
    assert (got[:G4 // 4] == -7.25).all() and (got[-G4 // 4:] == -7.25).all()
    y = got[G4 // 4:-G4 // 4].reshape(N, ld)
    assert (y[:, M:] == -7.25).all()
    assert np.isfinite(y[:, :M]).all()
    if algo == GEMV:
        assert_bitwise(y[:, :M], R.gemv_schedule(w16, x))
    elif algo == EXACT:
        assert_bitwise(y, G.mul_mat_f16_f32(w16, x))
    for b in (wd, xd, yd):
        b.free()


def test_status_codes(exact_off):
    L = exact_off
    K, M, N = 64, 4, 2
    wd, xd, yd = DB(M * K * 2 + 64), DB(N * K * 4), DB(N * (M + 1) * 4)
    call = lambda *a: L.ggml_hip_mul_mat_f16(*a)
    ok, inv, uns = ggml_hip.OK, ggml_hip.ERR_INVALID, ggml_hip.ERR_UNSUPPORTED
    assert call(wd.ptr, K, M, xd.ptr, N, yd.ptr, M, GEMV, None) == ok
    assert call(wd.ptr, 48, M, xd.ptr, N, yd.ptr, M, GEMV, None) == inv             # K % 32
    assert call(wd.ptr + 2, K, M, xd.ptr, N, yd.ptr, M, GEMV, None) == inv          # w off its 16-byte alignment
    assert call(wd.ptr + 8, K, M, xd.ptr, N, yd.ptr, M, 0, None) == inv
    for algo in (2, 3, 5, 6, 7, 8, 10):
        assert call(wd.ptr, K, M, xd.ptr, N, yd.ptr, M, algo, None) == inv
        assert call(wd.ptr, K, M, xd.ptr, 0, yd.ptr, M, algo, None) == inv          # refused first, an empty call too
    assert call(wd.ptr, K, M, xd.ptr, 0, yd.ptr, M, GEMV, None) == ok                # N == 0: nothing to do
    assert call(wd.ptr, K, M, xd.ptr, N, yd.ptr, M - 1, GEMV, None) == inv           # ldy < M
    assert call(None, K, M, xd.ptr, N, yd.ptr, M, GEMV, None) == inv
    # a K whose single column does not fit the GEMV's LDS image: algo 1 says so, auto runs the exact kernels
    big = 65568
    assert L.ggml_hip_debug_f16w_auto_algo(big, 1, 1) == EXACT
    wb, xb = DB(big * 2), DB(big * 4)
    assert call(wb.ptr, big, 1, xb.ptr, 1, yd.ptr, 1, GEMV, None) == uns
    assert b"GEMV" in L.ggml_hip_last_error()
    # the exact and MFMA launchers have no row pitch
    assert call(wd.ptr, K, M, xd.ptr, N, yd.ptr, M + 1, EXACT, None) == uns
    assert call(wd.ptr, K, M, xd.ptr, N, yd.ptr, M + 1, GEMM, None) == uns
    assert call(wd.ptr, K, M, xd.ptr, N, yd.ptr, M + 1, GEMV, None) == ok
    ggml_hip.check(L.ggml_hip_device_synchronize(), "sync")
    for b in (wd, xd, yd, wb, xb):
        b.free()
