"""numpy restatement of the reference's Q6_K x q8_K CPU path (k_quants.c, QK_K = 256), bit for bit:
block decoding, quantize_row_q8_K_reference, dequantize_row_q6_K, the integer superblock terms (y_exact,
S_abs in the form parity.block_terms returns) and the AVX2-order dot of ggml_vec_dot_q6_K_q8_K.

Checked against fixtures generated from the compiled reference (tests/golden/gen_golden_q6k.c) by
tests/test_q6k_ref.py; the GPU tests use it as their reference on fresh data.

Layouts: block_q6_K = ql[128] | qh[64] | int8 scales[16] | fp16 d (210 bytes); block_q8_K = f32 d |
int8 qs[256] | int16 bsums[16] (292 bytes).
"""
import ctypes
import ctypes.util

import numpy as np

QK_K = 256
Q6KB = 210
Q8KB = 292

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.fmaf.argtypes = [ctypes.c_float, ctypes.c_float, ctypes.c_float]
_libm.fmaf.restype = ctypes.c_float


def split_q6_K(wq, K):
    """uint8 [M, K/256*210] -> (d f32 [M, nb], sc int8 [M, nb, 16], q int8 [M, nb, 256]): q = 6-bit value - 32 in
    dequantized element order (k_quants.c:1078-1094); element e is scaled by sc[e // 16]."""
    nb = K // QK_K
    b = np.ascontiguousarray(wq, dtype=np.uint8).reshape(-1, nb, Q6KB)
    M = b.shape[0]
    ql = b[:, :, 0:128].reshape(M, nb, 2, 2, 32)          # [h][j & 1][l]
    qh = b[:, :, 128:192].reshape(M, nb, 2, 32)           # [h][l]
    sc = b[:, :, 192:208].copy().view(np.int8)
    d = b[:, :, 208:210].copy().view(np.float16)[:, :, 0].astype(np.float32)
    q = np.empty((M, nb, 2, 4, 32), np.int8)
    for j in range(4):
        nib = (ql[:, :, :, j & 1, :] >> 4) if (j >> 1) else (ql[:, :, :, j & 1, :] & 0x0F)
        hi = (qh >> (2 * j)) & 3
        q[:, :, :, j, :] = (nib | (hi << 4)).astype(np.int16) - 32
    return d, sc, q.reshape(M, nb, QK_K)


def random_q6_K(rng, M, K, special_d=True, d_scale=1.0):
    """Fresh valid block_q6_K rows: random ql / qh / scales bytes and finite fp16 d (any such bytes form a valid
    block), with zero, negative and fp16-subnormal d mixed in.  d_scale multiplies the spread of d (1.0: the bytes
    every caller without it has always got)."""
    nb = K // QK_K
    b = rng.integers(0, 256, size=(M, nb, Q6KB), dtype=np.uint8)
    d = (rng.standard_normal((M, nb)) * (0.01 * d_scale)).astype(np.float16)
    if special_d:
        flat = d.reshape(-1)
        n = flat.size
        flat[rng.integers(0, n, size=max(1, n // 16))] = np.float16(0.0)
        idx = rng.integers(0, n, size=max(1, n // 16))
        flat[idx] = (rng.integers(1, 1024, size=idx.size).astype(np.uint16)
                     | (rng.integers(0, 2, size=idx.size).astype(np.uint16) << 15)).view(np.float16)   # subnormals
    assert np.isfinite(d.astype(np.float32)).all()
    b[:, :, 208:210] = d.view(np.uint16).reshape(M, nb, 1).view(np.uint8).reshape(M, nb, 2)
    return b.reshape(M, nb * Q6KB)


def quantize_q8_K(x):
    """f32 [N, K] -> uint8 [N, K/256*292], quantize_row_q8_K_reference (k_quants.c:1133-1168); bsums of an
    all-zero block are written as zeros."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    N, K = x.shape
    nb = K // QK_K
    xb = x.reshape(N * nb, QK_K)
    out = np.zeros((N * nb, Q8KB), np.uint8)
    ax = np.abs(xb)
    j = ax.argmax(axis=1)                                  # the first element of largest |x| (strict >)
    rows = np.arange(N * nb)
    amax = ax[rows, j]
    mx = xb[rows, j]
    nz = amax != 0
    with np.errstate(divide="ignore", over="ignore", under="ignore", invalid="ignore"):
        iscale = np.where(nz, np.float32(-128.0) / np.where(nz, mx, np.float32(1)), np.float32(0)).astype(np.float32)
        val = (iscale[:, None] * xb).astype(np.float32) + np.float32(12582912.0)     # nearest_int
        v = (val.astype(np.float32).view(np.int32) & 0x007FFFFF) - 0x00400000
        q = np.minimum(127, v).astype(np.int8)
        q[~nz] = 0
        d = np.where(nz, np.float32(1.0) / np.where(nz, iscale, np.float32(1)), np.float32(0)).astype(np.float32)
    bsums = q.reshape(-1, 16, 16).astype(np.int32).sum(axis=2).astype(np.int16)
    out[:, 0:4] = d.view(np.uint8).reshape(-1, 4)
    out[:, 4:260] = q.view(np.uint8)
    out[:, 260:292] = bsums.view(np.uint8).reshape(-1, 32)
    return out.reshape(N, nb * Q8KB)


def split_q8_K(xq, K):
    """uint8 [N, K/256*292] -> (d f32 [N, nb], q int8 [N, nb, 256], bsums int16 [N, nb, 16])."""
    nb = K // QK_K
    b = np.ascontiguousarray(xq, dtype=np.uint8).reshape(-1, nb, Q8KB)
    d = b[:, :, 0:4].copy().view(np.float32)[:, :, 0]
    q = b[:, :, 4:260].copy().view(np.int8)
    bs = b[:, :, 260:292].copy().view(np.int16)
    return d, q, bs


def dequantize_q6_K(wq, K):
    """dequantize_row_q6_K: (d * (float)sc) * (float)q, two float32 multiplies -> f32 [M, K]."""
    d, sc, q = split_q6_K(wq, K)
    M, nb = d.shape
    ds = (d[:, :, None] * sc.astype(np.float32)).astype(np.float32)            # [M, nb, 16]
    y = (np.repeat(ds, 16, axis=2) * q.astype(np.float32)).astype(np.float32)
    return y.reshape(M, K)


def _lane_sums(wq, xq, K):
    """int64 [N, M, nb, 8]: the AVX2 branch's eight int32 lanes per superblock: lane m sums elements
    32g + 4m .. 32g + 4m + 3 of every 32-element group g, each group scaled by sc[2g + (m >= 4)]."""
    dw, sc, q = split_q6_K(wq, K)
    dx, q8, _ = split_q8_K(xq, K)
    M, nb = dw.shape
    N = dx.shape[0]
    qg = q.reshape(M, nb, 8, 8, 4).astype(np.int64)
    xg = q8.reshape(N, nb, 8, 8, 4).astype(np.int64)
    scl = sc.reshape(M, nb, 8, 2).astype(np.int64)[:, :, :, [0, 0, 0, 0, 1, 1, 1, 1]]     # [M, nb, g, lane]
    p = np.einsum("mbglk,nbglk->nmbgl", qg, xg)
    lanes = (p * scl[None]).sum(axis=3)
    assert np.abs(lanes).max(initial=0) < 2 ** 31
    return dw, dx, lanes


def block_terms(wq, xq, K):
    """(y_exact f64 [N, M], S_abs f64 [N, M]) from the exact integer superblock sums isum_b:
    y = sum_b d_x d_w isum_b, S_abs = sum_b |d_x d_w isum_b| (the form of parity.block_terms)."""
    dw, dx, lanes = _lane_sums(wq, xq, K)
    isum = lanes.sum(axis=3)
    assert np.abs(isum).max(initial=0) <= 2 ** 27
    t = dx.astype(np.float64)[:, None, :] * dw.astype(np.float64)[None, :, :] * isum
    return t.sum(axis=2), np.abs(t).sum(axis=2)


def vec_dot_avx2(wq, xq, K):
    """f32 [N, M]: ggml_vec_dot_q6_K_q8_K's AVX2 branch (k_quants.c:3484-3561), bit for bit:
    acc[m] = fmaf(d, (float)sumi[m], acc[m]) with d = d_x * fp32(d_w), superblocks in order, then hsum_float_8.
    The fused multiply-add is libm's fmaf (a float64 emulation would round twice)."""
    dw, dx, lanes = _lane_sums(wq, xq, K)
    N, M, nb, _ = lanes.shape
    d = (dx[:, None, :] * dw[None, :, :]).astype(np.float32)               # one float32 multiply
    lf = lanes.astype(np.float32)                                          # cvtepi32_ps (round to nearest even)
    fmaf = _libm.fmaf
    y = np.empty((N, M), np.float32)
    f32 = np.float32
    for n in range(N):
        for m in range(M):
            acc = [0.0] * 8
            dn, ln = d[n, m].tolist(), lf[n, m].tolist()
            for b in range(nb):
                db, lb = dn[b], ln[b]
                for k in range(8):
                    acc[k] = fmaf(db, lb[k], acc[k])
            a = [f32(v) for v in acc]
            r = [f32(a[k] + a[k + 4]) for k in range(4)]
            y[n, m] = f32(f32(r[0] + r[2]) + f32(r[1] + r[3]))
    return y
