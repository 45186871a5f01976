"""numpy restatement of the reference's Q5_K / Q4_K x q8_K CPU path (k_quants.c, QK_K = 256), bit for bit:
block decoding, dequantize_row_q5_K / _q4_K, the integer superblock terms (y_exact, S_abs in the form
parity.block_terms returns), the AVX2-order dots of ggml_vec_dot_q5_K_q8_K / _q4_K_q8_K, and the fp32 order of
the device GEMV k_gemv_q45_K (csrc/q45_k.hip).  qh = True is Q5_K, qh = False is Q4_K.

Checked against fixtures generated from the compiled reference (tests/golden/gen_golden_q45k.c) by
tests/test_q45k_ref.py; the GPU tests use it as their reference on fresh data.  The q8_K side is q6k_ref's.

Layouts: block_q5_K = fp16 d | fp16 dmin | scales[12] | qh[32] | qs[128] (176 bytes); block_q4_K is the same
without qh (144 bytes).  Element 64j + 32h + l (j = 0..3, h = 0..1, l = 0..31) is nibble h of qs[32j + l], plus
16 where bit 2j + h of qh[l] is set; sub-block s = 2j + h has the 6-bit scale sc[s] and min m[s]
(get_scale_min_k4, k_quants.c:264-273): w = d sc[s] q - dmin m[s].
"""
import numpy as np

from q6k_ref import QK_K, Q8KB, _libm, quantize_q8_K, split_q8_K   # noqa: F401  (re-exported for the tests)

Q5KB = 176
Q4KB = 144


def block_bytes(qh):
    return Q5KB if qh else Q4KB


def split_q45_K(wq, K, qh):
    """uint8 [M, K/256*bs] -> (d f32 [M, nb], dmin f32 [M, nb], sc int64 [M, nb, 8], m int64 [M, nb, 8],
    q int64 [M, nb, 8, 32]): q = the 4- or 5-bit value (0..15 / 0..31) of sub-block s, element l."""
    nb = K // QK_K
    bs = block_bytes(qh)
    b = np.ascontiguousarray(wq, dtype=np.uint8).reshape(-1, nb, bs)
    M = b.shape[0]
    d = b[:, :, 0:2].copy().view(np.float16)[:, :, 0].astype(np.float32)
    dmin = b[:, :, 2:4].copy().view(np.float16)[:, :, 0].astype(np.float32)
    s = b[:, :, 4:16].astype(np.int64)
    sc = np.empty((M, nb, 8), np.int64)
    m = np.empty((M, nb, 8), np.int64)
    sc[:, :, 0:4] = s[:, :, 0:4] & 63
    m[:, :, 0:4] = s[:, :, 4:8] & 63
    sc[:, :, 4:8] = (s[:, :, 8:12] & 0xF) | ((s[:, :, 0:4] >> 6) << 4)
    m[:, :, 4:8] = (s[:, :, 8:12] >> 4) | ((s[:, :, 4:8] >> 6) << 4)
    qs = b[:, :, bs - 128:bs].reshape(M, nb, 4, 32).astype(np.int64)
    q = np.empty((M, nb, 4, 2, 32), np.int64)
    q[:, :, :, 0, :] = qs & 0xF
    q[:, :, :, 1, :] = qs >> 4
    if qh:
        hb = b[:, :, 16:48].astype(np.int64)                # [M, nb, 32]
        for j in range(4):
            for h in range(2):
                q[:, :, j, h, :] += ((hb >> (2 * j + h)) & 1) << 4
    return d, dmin, sc, m, q.reshape(M, nb, 8, 32)


def random_q45_K(rng, M, K, qh, special=True, d_scale=1.0):
    """Fresh valid rows: random scales / qh / qs bytes and finite fp16 d, dmin (any such bytes form a valid block),
    with zero, negative and fp16-subnormal d / dmin and blocks of all-0 and all-63 scales and mins mixed in.
    d_scale multiplies the spread of d and dmin (1.0: the bytes every caller without it has always got)."""
    nb = K // QK_K
    bs = block_bytes(qh)
    b = rng.integers(0, 256, size=(M, nb, bs), dtype=np.uint8)
    n = M * nb
    for off, scale in ((0, 0.01), (2, 0.005)):
        d = (rng.standard_normal(n) * (scale * d_scale)).astype(np.float16)        # both signs
        if special:
            d[rng.integers(0, n, size=max(1, n // 16))] = np.float16(0.0)
            idx = rng.integers(0, n, size=max(1, n // 16))
            d[idx] = (rng.integers(1, 1024, size=idx.size).astype(np.uint16)
                      | (rng.integers(0, 2, size=idx.size).astype(np.uint16) << 15)).view(np.float16)   # subnormals
        assert np.isfinite(d.astype(np.float32)).all()
        b[:, :, off:off + 2] = d.view(np.uint8).reshape(M, nb, 2)
    if special:
        flat = b.reshape(n, bs)
        flat[rng.integers(0, n, size=max(1, n // 8)), 4:16] = 0x00     # every scale and min 0
        flat[rng.integers(0, n, size=max(1, n // 8)), 4:16] = 0xFF     # every scale and min 63
    return b.reshape(M, nb * bs)


def dequantize_q45_K(wq, K, qh):
    """dequantize_row_q5_K / _q4_K: (d * (float)sc) * (float)q - (dmin * (float)m), rounded multiplies and a
    rounded subtraction, no contraction -> f32 [M, K]."""
    d, dmin, sc, m, q = split_q45_K(wq, K, qh)
    M, nb = d.shape
    d1 = (d[:, :, None] * sc.astype(np.float32)).astype(np.float32)             # [M, nb, 8]
    m1 = (dmin[:, :, None] * m.astype(np.float32)).astype(np.float32)
    y = ((d1[:, :, :, None] * q.astype(np.float32)).astype(np.float32) - m1[:, :, :, None]).astype(np.float32)
    return y.reshape(M, K)


def _int_terms(wq, xq, K, qh):
    """(dw, dminw, dx, lanes int64 [N, M, nb, 8], prod int64 [N, M, nb, 4]): the AVX2 branches' eight int32 lanes per
    superblock (lane L sums sc[s] * q * q8 over elements 32s + 4L .. 32s + 4L + 3 of every sub-block s) and the four
    madd_epi16 products prod_i = m[2i] s[2i] + m[2i+1] s[2i+1] of the mins with the per-32 sums s of q8 (hadd_epi16
    of bsums)."""
    dw, dminw, sc, m, q = split_q45_K(wq, K, qh)
    dx, q8, bsums = split_q8_K(xq, K)
    M, nb = dw.shape
    N = dx.shape[0]
    qg = q.reshape(M, nb, 8, 8, 4)
    xg = q8.reshape(N, nb, 8, 8, 4).astype(np.int64)
    p = np.einsum("mbslk,nbslk->nmbsl", qg, xg)
    lanes = (p * sc[None, :, :, :, None]).sum(axis=3)
    assert np.abs(lanes).max(initial=0) < 2 ** 31
    s32 = bsums.astype(np.int64).reshape(N, nb, 8, 2).sum(axis=3)               # [N, nb, 8]
    ms = m[None] * s32[:, None]                                                 # [N, M, nb, 8]
    prod = ms.reshape(N, M, nb, 4, 2).sum(axis=4)
    return dw, dminw, dx, lanes, prod


def block_terms(wq, xq, K, qh):
    """(y_exact f64 [N, M], S_abs f64 [N, M]) from the exact integer superblock sums isum_b, msum_b:
    y = sum_b d_x d isum_b - d_x dmin msum_b, S_abs = sum_b |d_x d isum_b| + |d_x dmin msum_b|."""
    dw, dminw, dx, lanes, prod = _int_terms(wq, xq, K, qh)
    isum, msum = lanes.sum(axis=3), prod.sum(axis=3)
    assert np.abs(isum).max(initial=0) <= 2 ** 26 and np.abs(msum).max(initial=0) <= 2 ** 21
    a = dx.astype(np.float64)[:, None, :] * dw.astype(np.float64)[None, :, :] * isum
    c = dx.astype(np.float64)[:, None, :] * dminw.astype(np.float64)[None, :, :] * msum
    return (a - c).sum(axis=2), (np.abs(a) + np.abs(c)).sum(axis=2)


def gemv_schedule(wq, x, K, qh):
    """f32 [N, M]: k_gemv_q45_K's own fp32 order on the q8_K of x.  Per superblock b, in order:
    t_b = fmaf(d_x * d, (float)isum_b, -((d_x * dmin) * (float)msum_b)); acc = acc + t_b."""
    xq = quantize_q8_K(x)
    dw, dminw, dx, lanes, prod = _int_terms(wq, xq, K, qh)
    N, M, nb, _ = lanes.shape
    isum = lanes.sum(axis=3).astype(np.float32)                                 # v_cvt_f32_i32: nearest even
    msum = prod.sum(axis=3).astype(np.float32)                                  # exact (< 2^24)
    dd = (dx[:, None, :] * dw[None, :, :]).astype(np.float32)
    dm = (dx[:, None, :] * dminw[None, :, :]).astype(np.float32)
    negp = (-(dm * msum).astype(np.float32)).astype(np.float32)
    fmaf = _libm.fmaf
    f32 = np.float32
    y = np.empty((N, M), np.float32)
    for n in range(N):
        for m in range(M):
            acc = f32(0.0)
            a, i, c = dd[n, m].tolist(), isum[n, m].tolist(), negp[n, m].tolist()
            for b in range(nb):
                acc = f32(acc + f32(fmaf(a[b], i[b], c[b])))
            y[n, m] = acc
    return y


def vec_dot_avx2(wq, xq, K, qh):
    """f32 [N, M]: the AVX2 branch of ggml_vec_dot_q5_K_q8_K (k_quants.c:2927-3010) / ggml_vec_dot_q4_K_q8_K
    (2450-2513), bit for bit.  Both: acc[L] = fmaf(d, (float)lane L, acc[L]) with d = d_x * fp32(d_w), superblocks in
    order, then hsum_float_8; dmin = -d_x * fp32(dmin_w).  Q4_K: acc_m[i] = fmaf(dmin, (float)prod_i, acc_m[i]),
    folded (a0 + a2) + (a1 + a3) and added to the hsum.  Q5_K: summs += dmin * (float)(prod_0 + .. + prod_3), a rounded
    multiply and a rounded add, added to the hsum.  The fused multiply-add is libm's fmaf."""
    dw, dminw, dx, lanes, prod = _int_terms(wq, xq, K, qh)
    N, M, nb, _ = lanes.shape
    d = (dx[:, None, :] * dw[None, :, :]).astype(np.float32)
    dmin = ((-dx)[:, None, :] * dminw[None, :, :]).astype(np.float32)
    lf = lanes.astype(np.float32)                                               # cvtepi32_ps
    pf = prod.astype(np.float32)
    tot = prod.sum(axis=3).astype(np.float32)
    fmaf = _libm.fmaf
    f32 = np.float32
    y = np.empty((N, M), np.float32)
    for n in range(N):
        for m in range(M):
            acc = [0.0] * 8
            accm = [0.0] * 4
            summs = f32(0.0)
            dn, ln, mn = d[n, m].tolist(), lf[n, m].tolist(), dmin[n, m].tolist()
            pn, tn = pf[n, m].tolist(), tot[n, m]
            for b in range(nb):
                if qh:
                    summs = f32(summs + f32(f32(mn[b]) * tn[b]))
                else:
                    for i in range(4):
                        accm[i] = fmaf(mn[b], pn[b][i], accm[i])
                for k in range(8):
                    acc[k] = fmaf(dn[b], ln[b][k], acc[k])
            a = [f32(v) for v in acc]
            r = [f32(a[k] + a[k + 4]) for k in range(4)]
            h = f32(f32(r[0] + r[2]) + f32(r[1] + r[3]))
            if qh:
                y[n, m] = f32(h + summs)
            else:
                am = [f32(v) for v in accm]
                y[n, m] = f32(h + f32(f32(am[0] + am[2]) + f32(am[1] + am[3])))
    return y
