"""Test helper: the decode GEMV with an x prologue / epilogue on device pointers (ggml_hip_debug_gemv_norm; csrc/
q4_0_gemv.hip, ghip::gemv_q4_0_multi_norm), the inputs its tests feed it and their numpy references
(tests/ggml_ops_ref.py), sentinel-padded device buffers and the oracle bound on y.  Shared by
tests/test_gpu_gemv_prologue.py, tests/test_gpu_gemv_epi.py and the CPU-side input checks
(tests/test_gemv_norm_inputs.py); nothing here needs a device until a buffer is made."""
import ctypes

import numpy as np

import ggml_ops_ref as R
from hip_env import ggml_hip

P = ctypes.c_void_p
SENT = np.uint32(0x7FA5C3E1)              # a NaN pattern no kernel here produces
PAD = 64                                  # sentinel floats past the end of every output buffer

# the widths gemv_norm_supported (csrc/q4_0_gemv.hip) accepts lie on both sides of every bound that selects code
# (pairs per lane 1 / 2 / 3 at K <= 4096 / 8192 / 12288; x-waves = ceil(K / 512) for kind 1, ceil(K / 1024) for kind
# 2, at most 16): kind 1 up to 8192, kind 2 up to 12288
KS_KIND1 = (64, 128, 512, 4096, 4160, 8192)
KS_KIND2 = (64, 128, 512, 4096, 4160, 8192, 8256, 12288)
ROW_SETS = ([1], [17], [64, 2, 130], [16, 16, 16, 34])
# the hook-level widths: held for the prologue, and wider than it (their chain runs as its own launch)
HOOK_KS = {1: (64, 4160, 8192), 2: (64, 8256, 12288)}
HOOK_KS_WIDE = {1: (8256, 16384), 2: (12352, 13824, 16384)}
# tests/test_gpu_gemv_epi.py: (K, head size, heads, F16 V cache) of the rope / cache epilogue, (K, M) of the glu one
EPI_ROPE_CASES = [(4096, 128, 32, True), (4096, 64, 64, False), (5120, 128, 40, True),
                  (64, 2, 1, True), (64, 64, 1, False), (4160, 80, 1, True), (8192, 64, 2, False)]
EPI_GLU_CASES = [(4096, 11008), (5120, 13824), (4096, 1000), (64, 2), (64, 34), (4160, 130)]


class GemvEpi(ctypes.Structure):          # csrc/q4_0_kernels.h
    _fields_ = [("glu", ctypes.c_int), ("table", P), ("d", P * 4), ("cs", P * 4), ("c", P * 4),
                ("kind", ctypes.c_int * 4), ("f16", ctypes.c_int * 4), ("ne0", ctypes.c_int * 4),
                ("ne10", ctypes.c_int * 4), ("ne11", ctypes.c_int * 4), ("nb10", ctypes.c_int * 4),
                ("nb11", ctypes.c_int * 4), ("nb12", ctypes.c_int * 4)]


def rand_q4(M, K, rng):
    """M rows of valid q4_0 blocks: random nibbles, fp16 scales ~1e-2."""
    nb = K // 32
    blk = np.zeros((M, nb, 18), np.uint8)
    d = (rng.standard_normal((M, nb)) * 0.01).astype(np.float16)
    blk[:, :, 0:2] = d.view(np.uint8).reshape(M, nb, 2)
    blk[:, :, 2:] = rng.integers(0, 256, (M, nb, 16), dtype=np.uint8)
    return blk.reshape(M, nb * 18)


def _ptr(x):
    return None if x is None else (x if isinstance(x, int) else x.ptr)


def gemv_norm_rc(L, W, Ms, K, kind, a, b, w, ys, epi=None, reps=0, extra=None):
    """the raw call: (return code, mean us of the timed repeats).  kind 0: the plain GEMV on x = b"""
    L.ggml_hip_debug_gemv_norm.argtypes = [ctypes.c_int, P, P, ctypes.c_int64, ctypes.c_int, P, P, P, P, P, P, P, P,
                                           ctypes.c_int, P]
    n = len(W)
    wp = (P * 4)(*[_ptr(x) for x in W])
    mp = (ctypes.c_int64 * 4)(*Ms)
    yp = (P * 4)(*[_ptr(y) for y in ys])
    sc = extra or {}
    us = ctypes.c_float(0.0)
    rc = L.ggml_hip_debug_gemv_norm(n, wp, mp, K, kind, _ptr(a), _ptr(b), _ptr(w), _ptr(sc.get("sum")),
                                    _ptr(sc.get("norm")), _ptr(sc.get("out")), yp,
                                    ctypes.byref(epi) if epi is not None else None, reps, ctypes.byref(us))
    return rc, us.value


def gemv_norm(L, W, Ms, K, kind, a, b, w, ys, epi=None, reps=0, extra=None):
    rc, us = gemv_norm_rc(L, W, Ms, K, kind, a, b, w, ys, epi, reps, extra)
    ggml_hip.check(rc, "gemv_norm")
    return us


# ---------------------------------------------------------------------------------------------- inputs, references
def chain_case(kind, K, with_add, tabs):
    """the prologue's inputs at width K and the numpy restatement of its chain, float32 [K] each:
    kind 1: a (None without the add), b, w; sum = a + b (or b), norm = rms_norm(sum), out = norm * w.  The row is
            rms_rows' (rms_order_free: no correct double summation order changes the float mean);
    kind 2: a (the silu input: the whole fp16 range, clipped to finite fp16, with +-0, the largest fp16 and the
            smallest negative fp16 subnormal in front), b; norm = silu(a), out = norm * b; no sum"""
    if kind == 1:
        a, b, _ = R.rms_rows(K, 1, R.rms_seed(K, 1), with_add)
        w = (1.0 + 0.1 * np.random.default_rng(K).standard_normal(K)).astype(np.float32)
        x = R.add(a, b) if with_add else b
        nrm = R.rms_norm(x)
        out = R.mul(nrm, w[None, :])
        return {"kind": 1, "K": K, "a": a[0] if with_add else None, "b": b[0], "w": w, "sum": x[0], "norm": nrm[0],
                "out": out[0]}
    rng = np.random.default_rng(2 * K + 1)
    a = np.clip(R.silu_spread(rng, K), -65504.0, 65504.0).astype(np.float32)
    a[:4] = np.array([0.0, -0.0, 65504.0, -5.9604645e-8], np.float32)
    b = rng.standard_normal(K).astype(np.float32)
    u = R.silu(a, tabs[0])
    return {"kind": 2, "K": K, "a": a, "b": b, "w": None, "sum": None, "norm": u, "out": R.mul(u, b)}


def assert_case_inputs(c):
    """what the device tests rely on, checkable without a device"""
    assert np.isfinite(c["out"]).all() and c["out"].any()
    if c["kind"] == 1:
        assert R.rms_order_free(c["sum"])
    else:
        assert np.isfinite(R.fp16_to_f32(R.fp16_bits(c["a"]))).all()
        assert R.bits(c["a"][:4]).tolist() == [0, 0x80000000, 0x477FE000, 0xB3800000]


# ---------------------------------------------------------------------------------------------- device buffers
def sentinel_buf(n):
    """n float32 plus PAD more, every word the sentinel"""
    return ggml_hip.DeviceBuffer.from_array(np.full(n + PAD, SENT, np.uint32))


def read_checked(buf, n):
    """the first n words as float32; the PAD words behind them must still be the sentinel"""
    v = buf.download((n + PAD,), np.uint32)
    assert (v[n:] == SENT).all(), np.flatnonzero(v[n:] != SENT)[:8]
    return v[:n].view(np.float32)


def untouched(buf, n):
    return bool((buf.download((n + PAD,), np.uint32) == SENT).all())


def assert_oracle(wq, K, x, y):
    """y [M] within the project's bound (tests/test_gpu_ggml_hook.py: rtol 1e-3 on y, 1e-6 of the sum of the
    absolute block terms) of the oracle's mul_mat of wq and the float32 row x; block terms in slices of rows"""
    import oracle as O
    from parity import block_terms, check_y
    xq = O.quantize_q8_0(x[None, :])
    y_ref = O.mul_mat(wq, K, x[None, :])
    s_abs = np.concatenate([block_terms(wq[i:i + 2048], xq, K)[1] for i in range(0, wq.shape[0], 2048)], axis=1)
    rel, _ = check_y(np.asarray(y)[None, :], y_ref, s_abs, rtol=1e-3, atol_blocks=1e-6)
    assert rel < 1e-3
