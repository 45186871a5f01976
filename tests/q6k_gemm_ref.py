"""numpy restatement of the schedule the Q6_K GEMV and the int8-MFMA GEMM share (csrc/q6_k.hip,
csrc/q6_k_gemm.hip), bit for bit, built on q6k_ref.py:

    per output and superblock b:  isum_b = sum_g sc[g] sum_(e in g) (q_e - 32) q8_e          (exact int32)
                                  acc = fmaf((float32)(d_x[n][b] * d_w[m][b]), (float32)isum_b, acc)
    superblocks in order b = 0 .. nb - 1, acc starting from +0,

and the GEMM's digit split of the scaled weight w' = sc (q - 32) = 128 hi + lo.
"""
import numpy as np

import q6k_ref as R


def gemv_order(wq, xq, K):
    """f32 [N, M] from Q6_K rows wq and block_q8_K rows xq, in the device schedule (libm fmaf, as vec_dot_avx2)."""
    dw, dx, lanes = R._lane_sums(wq, xq, K)
    isum = lanes.sum(-1)
    assert np.abs(isum).max(initial=0) <= 2 ** 27
    N, M, nb = isum.shape
    isf = isum.astype(np.float32)                                          # v_cvt_f32_i32, round to nearest even
    d = (dx[:, None, :] * dw[None, :, :]).astype(np.float32)               # one float32 multiply
    fmaf = R._libm.fmaf
    y = np.empty((N, M), np.float32)
    for n in range(N):
        for m in range(M):
            acc = 0.0
            dn, sn = d[n, m].tolist(), isf[n, m].tolist()
            for b in range(nb):
                acc = fmaf(dn[b], sn[b], acc)
            y[n, m] = acc
    return y


def scaled_weights(wq, K):
    """int32 [M, nb, 256]: w' = sc (q - 32) in element order."""
    _, sc, q = R.split_q6_K(wq, K)
    return np.repeat(sc.astype(np.int32), 16, axis=2) * q.astype(np.int32)


def digits(wq, K):
    """(hi, lo) int32 [M, nb, 256] with w' = 128 hi + lo, lo in [-64, 63]: lo = ((w' + 64) & 127) - 64."""
    w = scaled_weights(wq, K)
    lo = ((w + 64) & 127) - 64
    hi = (w - lo) >> 7
    return hi, lo


def pack_q6_K(q6, sc, d):
    """block_q6_K rows from 6-bit values q6 [M, nb, 256] (0..63, element order), int8 scales [M, nb, 16] and
    fp16 d [M, nb]: the inverse of q6k_ref.split_q6_K."""
    q6 = np.asarray(q6, np.uint8)
    M, nb, _ = q6.shape
    e = q6.reshape(M, nb, 2, 4, 32)                                        # [h][j][l]
    b = np.zeros((M, nb, R.Q6KB), np.uint8)
    ql = np.zeros((M, nb, 2, 2, 32), np.uint8)
    qh = np.zeros((M, nb, 2, 32), np.uint8)
    for j in range(4):
        ql[:, :, :, j & 1, :] |= (e[:, :, :, j, :] & 0x0F) << (4 * (j >> 1))
        qh |= (e[:, :, :, j, :] >> 4) << (2 * j)
    b[:, :, 0:128] = ql.reshape(M, nb, 128)
    b[:, :, 128:192] = qh.reshape(M, nb, 64)
    b[:, :, 192:208] = np.asarray(sc, np.int8).reshape(M, nb, 16).view(np.uint8)
    b[:, :, 208:210] = np.ascontiguousarray(d, np.float16).reshape(M, nb, 1).view(np.uint8).reshape(M, nb, 2)
    return b.reshape(M, nb * R.Q6KB)
