"""numpy restatement of the integer arithmetic of the Q5_K / Q4_K int8-MFMA GEMM (csrc/q45_k_gemm.hip), built on
q45k_ref.py.  The GEMM shares the GEMV's schedule (q45k_ref.gemv_schedule); what is its own is how the two exact
superblock sums come off the matrix cores:

    isum_b = sum_s sc[s] sum_l q q8      the scaled weight w' = sc[s] q = 128 hi + lo, lo = w' & 127, hi = w' >> 7
                                         isum_b = 128 (hi . q8) + (lo . q8)
    msum_b = sum_s m[s] bsum32[s]        bsum32 = 128 bh + bl, bl = bsum32 & 127, bh = bsum32 >> 7 (arithmetic)
                                         msum_b = 128 (m . bh) + (m . bl)

qh = True is Q5_K, qh = False is Q4_K.
"""
import numpy as np

import q45k_ref as R

Q_MAX = {True: 31, False: 15}


def scaled_weights(wq, K, qh):
    """int64 [M, nb, 8, 32]: w' = sc[s] q of sub-block s, element l."""
    _, _, sc, _, q = R.split_q45_K(wq, K, qh)
    return sc[:, :, :, None] * q


def digits(wq, K, qh):
    """(hi, lo) int64 [M, nb, 8, 32] with w' = 128 hi + lo, lo in [0, 127], hi in [0, 15]."""
    w = scaled_weights(wq, K, qh)
    return w >> 7, w & 127


def bsum32(xq, K):
    """int64 [N, nb, 8]: the sums of the 32 q8 of each sub-block (the reference's bsums pairs added)."""
    _, q8, _ = R.split_q8_K(xq, K)
    return q8.astype(np.int64).reshape(q8.shape[0], K // R.QK_K, 8, 32).sum(axis=3)


def bsum_digits(xq, K):
    """(bh, bl) int64 [N, nb, 8] with bsum32 = 128 bh + bl, bl in [0, 127], bh in [-32, 31]."""
    s = bsum32(xq, K)
    return s >> 7, s & 127


def sums_from_digits(wq, xq, K, qh):
    """(isum, msum) int64 [N, M, nb], recomposed from the four digit products the matrix cores accumulate."""
    hi, lo = digits(wq, K, qh)
    bh, bl = bsum_digits(xq, K)
    _, _, _, m, _ = R.split_q45_K(wq, K, qh)
    _, q8, _ = R.split_q8_K(xq, K)
    M, nb = hi.shape[:2]
    x = q8.astype(np.int64).reshape(-1, nb, 256)
    H = np.einsum("mbk,nbk->nmb", hi.reshape(M, nb, 256), x)
    L = np.einsum("mbk,nbk->nmb", lo.reshape(M, nb, 256), x)
    Mh = np.einsum("mbs,nbs->nmb", m, bh)
    Ml = np.einsum("mbs,nbs->nmb", m, bl)
    assert np.abs(H).max(initial=0) < 2 ** 19 and np.abs(L).max(initial=0) < 2 ** 22
    assert np.abs(Mh).max(initial=0) < 2 ** 14 and np.abs(Ml).max(initial=0) < 2 ** 16
    return 128 * H + L, 128 * Mh + Ml


def pack_q45_K(q, sc, m, d, dmin, qh):
    """block_q5_K / block_q4_K rows from values q [M, nb, 8, 32] (0..31 / 0..15), 6-bit scales and mins
    [M, nb, 8] and fp16 d, dmin [M, nb]: the inverse of q45k_ref.split_q45_K."""
    q = np.asarray(q, np.int64)
    sc, m = np.asarray(sc, np.int64), np.asarray(m, np.int64)
    M, nb = q.shape[:2]
    bs = R.block_bytes(qh)
    b = np.zeros((M, nb, bs), np.uint8)
    b[:, :, 0:2] = np.ascontiguousarray(d, np.float16).reshape(M, nb, 1).view(np.uint8).reshape(M, nb, 2)
    b[:, :, 2:4] = np.ascontiguousarray(dmin, np.float16).reshape(M, nb, 1).view(np.uint8).reshape(M, nb, 2)
    b[:, :, 4:8] = (sc[:, :, 0:4] & 63) | ((sc[:, :, 4:8] >> 4) << 6)
    b[:, :, 8:12] = (m[:, :, 0:4] & 63) | ((m[:, :, 4:8] >> 4) << 6)
    b[:, :, 12:16] = (sc[:, :, 4:8] & 0xF) | ((m[:, :, 4:8] & 0xF) << 4)
    e = q.reshape(M, nb, 4, 2, 32)
    b[:, :, bs - 128:bs] = ((e[:, :, :, 0, :] & 0xF) | ((e[:, :, :, 1, :] & 0xF) << 4)).reshape(M, nb, 128)
    if qh:
        hb = np.zeros((M, nb, 32), np.int64)
        for j in range(4):
            for h in range(2):
                hb |= (e[:, :, j, h, :] >> 4) << (2 * j + h)
        b[:, :, 16:48] = hb
    return b.reshape(M, nb * bs)
