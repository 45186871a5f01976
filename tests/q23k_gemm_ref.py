"""numpy restatement of the integer arithmetic of the Q3_K / Q2_K int8-MFMA GEMM (csrc/q23_k_gemm.hip), built on
q23k_ref.py.  The GEMM shares the GEMV's schedule (q23k_ref.gemv_schedule); what is its own is how the exact
superblock sums come off the matrix cores, with the sub-block scale folded into the int8 weight:

    Q3_K  isum_b = sum_s sc[s] sum_l q q8    sc in [-32, 31], q in [-4, 3]: sc q reaches 128, so the plane holds the
                                             negated product w" = (-sc) q in [-128, 124] and isum_b = -(w" . q8)
    Q2_K  isum_b = sum_s sc[s] sum_l q q8    sc in [0, 15], q in [0, 3]: the plane holds w' = sc q in [0, 45]
          msum_b = sum_s m[s] bsum16[s]      bsum16 = 128 bh + bl, bl = bsum16 & 127, bh = bsum16 >> 7 (arithmetic)
                                             msum_b = 128 (m . bh) + (m . bl), sixteen sub-blocks = the MFMA's K = 16

The kernel forms a byte of the plane as the low byte of the product of the two factors' low bytes; that is the right
int8 whatever the signs because the true value fits in one (scaled_weights asserts it).  q3 = True is Q3_K, q3 =
False is Q2_K.
"""
import numpy as np

import q23k_ref as R


def scaled_weights(wq, K, q3):
    """int64 [M, nb, 16, 16]: what the weight plane holds, element j of sub-block s: (-sc[s]) q for Q3_K, sc[s] q for
    Q2_K; always an int8, and equal to the byte product mod 256 read as a signed byte."""
    _, _, sc, _, q = R._split(wq, K, q3)
    w = (-sc if q3 else sc)[:, :, :, None] * q
    assert w.min(initial=0) >= -128 and w.max(initial=0) <= 127
    f = (-sc if q3 else sc)[:, :, :, None] & 0xFF
    low = ((q & 0xFF) * f) & 0xFF
    assert np.array_equal(low.astype(np.uint8).view(np.int8).astype(np.int64), w)
    return w


def isum_sign(q3):
    """isum_b = isum_sign * (plane . q8)"""
    return -1 if q3 else 1


def bsum16(xq, K):
    """int64 [N, nb, 16]: the sums of the 16 q8 of each sub-block (the reference's bsums, recomputed from qs)."""
    _, q8, bsums = R.split_q8_K(xq, K)
    s = q8.astype(np.int64).reshape(q8.shape[0], K // R.QK_K, 16, 16).sum(axis=3)
    assert np.array_equal(s, bsums.astype(np.int64).reshape(s.shape))
    return s


def bsum_digits(xq, K):
    """(bh, bl) int64 [N, nb, 16] with bsum16 = 128 bh + bl, bl in [0, 127], bh in [-16, 15]."""
    s = bsum16(xq, K)
    return s >> 7, s & 127


def sums_from_planes(wq, xq, K, q3):
    """(isum, msum) int64 [N, M, nb], rebuilt from what the kernel feeds the matrix cores: the int8 weight plane
    against the q8 values (one chain per superblock) and, Q2_K, the m bytes against the two digits of bsum16 (msum =
    0 for Q3_K).  The ranges stated in the kernel's header are asserted."""
    w = scaled_weights(wq, K, q3)
    _, _, _, m, _ = R._split(wq, K, q3)
    _, q8, _ = R.split_q8_K(xq, K)
    M, nb = w.shape[:2]
    plane = w.reshape(M, nb, 256).astype(np.int8)
    x = q8.reshape(-1, nb, 256).astype(np.int8)
    S = np.einsum("mbk,nbk->nmb", plane.astype(np.int64), x.astype(np.int64))
    assert np.abs(S).max(initial=0) <= (2 ** 22 if q3 else 45 * 128 * 256)
    bh, bl = bsum_digits(xq, K)
    assert bl.min(initial=0) >= 0 and bl.max(initial=0) <= 127 and bh.min(initial=0) >= -16 and bh.max(initial=0) <= 15
    assert m.min(initial=0) >= 0 and m.max(initial=0) <= 15
    Mh = np.einsum("mbs,nbs->nmb", m, bh)
    Ml = np.einsum("mbs,nbs->nmb", m, bl)
    assert np.abs(Ml).max(initial=0) <= 16 * 15 * 127 and np.abs(Mh).max(initial=0) <= 16 * 15 * 16
    msum = 128 * Mh + Ml
    assert np.abs(msum).max(initial=0) <= 16 * 15 * 2048
    return isum_sign(q3) * S, msum


def pack_q23_K(q, sc, m, d, dmin, q3):
    """block_q3_K / block_q2_K rows from values q [M, nb, 16, 16] (-4..3 / 0..3), scales sc [M, nb, 16] (-32..31 /
    0..15), Q2_K mins m [M, nb, 16] (0..15) and fp16 d, dmin [M, nb] (Q3_K ignores m and dmin): the inverse of
    q23k_ref._split."""
    q = np.asarray(q, np.int64)
    sc = np.asarray(sc, np.int64)
    M, nb = q.shape[:2]
    bs = R.block_bytes(q3)
    b = np.zeros((M, nb, bs), np.uint8)
    u = (q + 4 if q3 else q).reshape(M, nb, 2, 4, 32)          # element 128n + 32k + l
    assert u.min() >= 0 and u.max() <= (7 if q3 else 3)
    qs = np.zeros((M, nb, 2, 32), np.int64)
    for k in range(4):
        qs |= (u[:, :, :, k, :] & 3) << (2 * k)
    d16 = np.ascontiguousarray(d, np.float16).reshape(M, nb, 1).view(np.uint8).reshape(M, nb, 2)
    if q3:
        hm = np.zeros((M, nb, 32), np.int64)
        for n in range(2):
            for k in range(4):
                hm |= (u[:, :, n, k, :] >> 2) << (4 * n + k)
        v = sc + 32
        assert v.min() >= 0 and v.max() <= 63
        s = np.zeros((M, nb, 12), np.int64)
        for g in range(4):                                     # scales 4g .. 4g + 3
            s[:, :, 4 * (g & 1):4 * (g & 1) + 4] |= (v[:, :, 4 * g:4 * g + 4] & 0xF) << (4 * (g >> 1))
            s[:, :, 8:12] |= (v[:, :, 4 * g:4 * g + 4] >> 4) << (2 * g)
        b[:, :, 0:32] = hm
        b[:, :, 32:96] = qs.reshape(M, nb, 64)
        b[:, :, 96:108] = s
        b[:, :, 108:110] = d16
    else:
        m = np.asarray(m, np.int64)
        assert sc.min() >= 0 and sc.max() <= 15 and m.min() >= 0 and m.max() <= 15
        b[:, :, 0:16] = sc | (m << 4)
        b[:, :, 16:80] = qs.reshape(M, nb, 64)
        b[:, :, 80:82] = d16
        b[:, :, 82:84] = np.ascontiguousarray(dmin, np.float16).reshape(M, nb, 1).view(np.uint8).reshape(M, nb, 2)
    return b.reshape(M, nb * bs)
