"""numpy restatement of the reference's Q3_K / Q2_K x q8_K CPU path (k_quants.c, QK_K = 256), bit for bit:
block decoding, dequantize_row_q3_K / _q2_K, the integer superblock terms (y_exact, S_abs in the form
parity.block_terms returns), the AVX2-order dots of ggml_vec_dot_q3_K_q8_K / _q2_K_q8_K, and the fp32 order of
the device GEMV k_gemv_q23_K (csrc/q23_k.hip).  q3 = True is Q3_K, q3 = False is Q2_K.

Checked against fixtures generated from the compiled reference (tests/golden/gen_golden_q23k.c) by
tests/test_q23k_ref.py; the GPU tests use it as their reference on fresh data.  The q8_K side is q6k_ref's.

Layouts: block_q3_K = hmask[32] | qs[64] | scales[12] | fp16 d (110 bytes); block_q2_K = scales[16] | qs[64] |
fp16 d | fp16 dmin (84 bytes).  Element 128n + 32k + l (n = 0..1, k = 0..3, l = 0..31) has the low bits
(qs[32n + l] >> 2k) & 3 and the sub-block s = 8n + 2k + l // 16.  Q3_K: q = low2 + 4 * bit (4n + k) of hmask[l] - 4,
sc[s] = the six-bit scale (k_quants.c:1854-1860) - 32, w = d sc[s] q.  Q2_K: q = low2, sc[s] = scales[s] & 15,
m[s] = scales[s] >> 4, w = d sc[s] q - dmin m[s].
"""
import numpy as np

from q6k_ref import QK_K, Q8KB, _libm, quantize_q8_K, split_q8_K   # noqa: F401  (re-exported for the tests)

Q3KB = 110
Q2KB = 84


def block_bytes(q3):
    return Q3KB if q3 else Q2KB


def _low2(qs):
    """qs uint8 [M, nb, 64] -> int64 [M, nb, 2, 4, 32]: element (n, k, l) = (qs[32n + l] >> 2k) & 3"""
    M, nb, _ = qs.shape
    v = qs.reshape(M, nb, 2, 1, 32).astype(np.int64)
    return (v >> (2 * np.arange(4)).reshape(1, 1, 1, 4, 1)) & 3


def split_q3_K(wq, K):
    """uint8 [M, K/256*110] -> (d f32 [M, nb], sc int64 [M, nb, 16] in -32..31, q int64 [M, nb, 16, 16] in -4..3):
    q[.., s, j] is element 16s + j of the superblock."""
    nb = K // QK_K
    b = np.ascontiguousarray(wq, dtype=np.uint8).reshape(-1, nb, Q3KB)
    M = b.shape[0]
    d = b[:, :, 108:110].copy().view(np.float16)[:, :, 0].astype(np.float32)
    s = b[:, :, 96:108].astype(np.int64)
    sc = np.empty((M, nb, 16), np.int64)
    for g in range(4):                                     # scales 4g .. 4g + 3: aux[g] of the reference
        low = (s[:, :, 4 * (g & 1):4 * (g & 1) + 4] >> (4 * (g >> 1))) & 0xF
        high = (s[:, :, 8:12] >> (2 * g)) & 3
        sc[:, :, 4 * g:4 * g + 4] = (low | (high << 4)) - 32
    q = _low2(b[:, :, 32:96])
    hm = b[:, :, 0:32].astype(np.int64)                    # [M, nb, 32]
    for n in range(2):
        for k in range(4):
            q[:, :, n, k, :] += 4 * ((hm >> (4 * n + k)) & 1) - 4
    return d, sc, q.reshape(M, nb, 16, 16)


def split_q2_K(wq, K):
    """uint8 [M, K/256*84] -> (d, dmin f32 [M, nb], sc, m int64 [M, nb, 16] in 0..15, q int64 [M, nb, 16, 16] in 0..3)"""
    nb = K // QK_K
    b = np.ascontiguousarray(wq, dtype=np.uint8).reshape(-1, nb, Q2KB)
    M = b.shape[0]
    d = b[:, :, 80:82].copy().view(np.float16)[:, :, 0].astype(np.float32)
    dmin = b[:, :, 82:84].copy().view(np.float16)[:, :, 0].astype(np.float32)
    s = b[:, :, 0:16].astype(np.int64)
    return d, dmin, s & 0xF, s >> 4, _low2(b[:, :, 16:80]).reshape(M, nb, 16, 16)


def _split(wq, K, q3):
    """(d, dmin, sc, m, q) for either type; Q3_K has dmin = 0 and m = 0"""
    if q3:
        d, sc, q = split_q3_K(wq, K)
        return d, np.zeros_like(d), sc, np.zeros_like(sc), q
    return split_q2_K(wq, K)


def random_q23_K(rng, M, K, q3, special=True, d_scale=1.0):
    """Fresh valid rows: random scale / hmask / qs bytes and finite fp16 d (dmin) (any such bytes form a valid block),
    with zero, negative and fp16-subnormal d / dmin mixed in, and blocks whose scales are all -32 and all 31 (Q3_K),
    whose scales and mins are all 0 and all 15 (Q2_K), and, Q3_K, whose hmask is all set and all clear.
    d_scale multiplies the spread of d and dmin (1.0: the bytes every caller without it has always got)."""
    nb = K // QK_K
    bs = block_bytes(q3)
    b = rng.integers(0, 256, size=(M, nb, bs), dtype=np.uint8)
    n = M * nb
    for off, scale in ((108, 0.01),) if q3 else ((80, 0.01), (82, 0.005)):
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
        s0, s1 = (96, 108) if q3 else (0, 16)
        flat[rng.integers(0, n, size=max(1, n // 8)), s0:s1] = 0x00     # Q3_K: every scale -32; Q2_K: scales, mins 0
        flat[rng.integers(0, n, size=max(1, n // 8)), s0:s1] = 0xFF     # Q3_K: every scale 31; Q2_K: scales, mins 15
        if q3:
            flat[rng.integers(0, n, size=max(1, n // 8)), 0:32] = 0x00  # every high bit clear: q in -4..-1
            flat[rng.integers(0, n, size=max(1, n // 8)), 0:32] = 0xFF  # every high bit set: q in 0..3
    return b.reshape(M, nb * bs)


def dequantize(wq, K, q3):
    """dequantize_row_q3_K: (d * (float)sc) * (float)q; dequantize_row_q2_K: (d * (float)sc) * (float)q - dmin *
    (float)m; rounded multiplies and a rounded subtraction, no contraction -> f32 [M, K]."""
    d, dmin, sc, m, q = _split(wq, K, q3)
    M, nb = d.shape
    dl = (d[:, :, None] * sc.astype(np.float32)).astype(np.float32)             # [M, nb, 16]
    y = (dl[:, :, :, None] * q.astype(np.float32)).astype(np.float32)
    if not q3:
        ml = (dmin[:, :, None] * m.astype(np.float32)).astype(np.float32)
        y = (y - ml[:, :, :, None]).astype(np.float32)
    return y.reshape(M, K)


def _int_terms(wq, xq, K, q3):
    """(dw, dminw, dx, lanes int64 [N, M, nb, 8], prod int64 [N, M, nb, 8]): the AVX2 branches' eight int32 lanes per
    superblock, lane L = sum_n sum_k sc[8n + 2k + (L >= 4)] * sum of q q8 over elements 128n + 32k + 4L .. + 3, and
    the eight madd_epi16 products of the mins with bsums, prod_L = m[2L] bsums[2L] + m[2L + 1] bsums[2L + 1]
    (zero for Q3_K)."""
    dw, dminw, sc, m, q = _split(wq, K, q3)
    dx, q8, bsums = split_q8_K(xq, K)
    M, nb = dw.shape
    N = dx.shape[0]
    # element 128n + 32k + 16h + 4j + e: sub-block (n, k, h), lane L = 4h + j
    qg = q.reshape(M, nb, 2, 4, 2, 4, 4)
    xg = q8.reshape(N, nb, 2, 4, 2, 4, 4).astype(np.int64)
    p = np.einsum("mbnkhje,cbnkhje->cmbnkhj", qg, xg)                            # [N, M, nb, 2, 4, 2, 4]
    scg = sc.reshape(M, nb, 2, 4, 2)
    lanes = (p * scg[None, :, :, :, :, :, None]).sum(axis=(3, 4)).reshape(N, M, nb, 8)
    assert np.abs(lanes).max(initial=0) < 2 ** 31
    ms = m[None] * bsums.astype(np.int64)[:, None]                              # [N, M, nb, 16]
    prod = ms.reshape(N, M, nb, 8, 2).sum(axis=4)
    return dw, dminw, dx, lanes, prod


def block_terms(wq, xq, K, q3):
    """(y_exact f64 [N, M], S_abs f64 [N, M]) from the exact integer superblock sums isum_b, msum_b:
    y = sum_b d_x d isum_b - d_x dmin msum_b, S_abs = sum_b |d_x d isum_b| + |d_x dmin msum_b|."""
    dw, dminw, dx, lanes, prod = _int_terms(wq, xq, K, q3)
    isum, msum = lanes.sum(axis=3), prod.sum(axis=3)
    assert np.abs(isum).max(initial=0) <= 2 ** 22 and np.abs(msum).max(initial=0) <= 2 ** 19
    a = dx.astype(np.float64)[:, None, :] * dw.astype(np.float64)[None, :, :] * isum
    c = dx.astype(np.float64)[:, None, :] * dminw.astype(np.float64)[None, :, :] * msum
    return (a - c).sum(axis=2), (np.abs(a) + np.abs(c)).sum(axis=2)


def gemv_schedule(wq, x, K, q3):
    """f32 [N, M]: k_gemv_q23_K's own fp32 order on the q8_K of x.  Per superblock b, in order:
    Q3_K t_b = (d_x * d) * (float)isum_b; Q2_K t_b = fmaf(d_x * d, (float)isum_b, -((d_x * dmin) * (float)msum_b));
    acc = acc + t_b."""
    xq = quantize_q8_K(x)
    dw, dminw, dx, lanes, prod = _int_terms(wq, xq, K, q3)
    N, M, nb, _ = lanes.shape
    isum = lanes.sum(axis=3).astype(np.float32)                                 # exact (<= 2^22)
    msum = prod.sum(axis=3).astype(np.float32)
    dd = (dx[:, None, :] * dw[None, :, :]).astype(np.float32)
    dm = (dx[:, None, :] * dminw[None, :, :]).astype(np.float32)
    negp = (-(dm * msum).astype(np.float32)).astype(np.float32)
    tq3 = (dd * isum).astype(np.float32)
    fmaf = _libm.fmaf
    f32 = np.float32
    y = np.empty((N, M), np.float32)
    for n in range(N):
        for m in range(M):
            acc = f32(0.0)
            a, i, c, t3 = dd[n, m].tolist(), isum[n, m].tolist(), negp[n, m].tolist(), tq3[n, m]
            for b in range(nb):
                acc = f32(acc + (t3[b] if q3 else f32(fmaf(a[b], i[b], c[b]))))
            y[n, m] = acc
    return y


def vec_dot_avx2(wq, xq, K, q3):
    """f32 [N, M]: the AVX2 branch of ggml_vec_dot_q3_K_q8_K (k_quants.c:1836-1938) / ggml_vec_dot_q2_K_q8_K
    (1330-1394), bit for bit.  Per superblock, in order: Q2_K first acc[L] = fmaf(dmin, (float)prod_L, acc[L]) with
    dmin = -d_x * fp32(dmin_w); then both acc[L] = fmaf(d, (float)lane L, acc[L]) with d = d_x * fp32(d_w); at the
    end hsum_float_8.  The fused multiply-add is libm's fmaf."""
    dw, dminw, dx, lanes, prod = _int_terms(wq, xq, K, q3)
    N, M, nb, _ = lanes.shape
    d = (dx[:, None, :] * dw[None, :, :]).astype(np.float32)
    dmin = ((-dx)[:, None, :] * dminw[None, :, :]).astype(np.float32)
    lf = lanes.astype(np.float32)                                               # cvtepi32_ps
    pf = prod.astype(np.float32)
    fmaf = _libm.fmaf
    f32 = np.float32
    y = np.empty((N, M), np.float32)
    for n in range(N):
        for m in range(M):
            acc = [0.0] * 8
            dn, ln, mn, pn = d[n, m].tolist(), lf[n, m].tolist(), dmin[n, m].tolist(), pf[n, m].tolist()
            for b in range(nb):
                if not q3:
                    for k in range(8):
                        acc[k] = fmaf(mn[b], pn[b][k], acc[k])
                for k in range(8):
                    acc[k] = fmaf(dn[b], ln[b][k], acc[k])
            a = [f32(v) for v in acc]
            r = [f32(a[k] + a[k + 4]) for k in range(4)]
            y[n, m] = f32(f32(r[0] + r[2]) + f32(r[1] + r[3]))
    return y
