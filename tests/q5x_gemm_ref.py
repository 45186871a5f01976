"""numpy restatement of the Q4_1 / Q5_1 prefill GEMM's schedule (csrc/q5x_gemm.hip, algo 7 of ggml_hip_mul_mat_q4_1 /
_q5_1), independent of the device.  Per output y[n][m], from acc = +0, the blocks b = 0 .. K / 32 - 1 in order:

    acc = fmaf((float)isum_b, d_w[m][b] * d_x[n][b], acc)      the product one rounded float32 multiply
    acc = fmaf(m_w[m][b], s_x[n][b], acc)

isum_b is the exact integer sum of the block's 32 products of the stored weight value (0..15 / 0..31) and the q8_1
byte, at most 32 * 31 * 127 < 2^17.  Both fma products are exact in float64 (17 x 24 and 11 x 24 bits), so
blk32_ref.fmaf32 is a correctly rounded fma for them."""
import numpy as np

import q5x_ref as R
from blk32_ref import fmaf32


def chain(t, wq, xq, K):
    """f32 [N, M] of the weight rows wq (uint8 [M, B K / 32]) against the q8_1 rows xq (uint8 [N, 40 K / 32])."""
    assert R.has_min(t)
    dw, mw, dx, sx, lanes = R._lane_sums(t, wq, xq, K)
    isum = lanes.sum(axis=3)
    assert np.abs(isum).max(initial=0) < 1 << 17
    isum = isum.astype(np.float32)
    N, M, nb = isum.shape
    acc = np.zeros((N, M), np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for b in range(nb):
            d = (dw[None, :, b] * dx[:, None, b]).astype(np.float32)
            acc = fmaf32(isum[:, :, b], d, acc)
            acc = fmaf32(np.broadcast_to(mw[None, :, b], acc.shape), np.broadcast_to(sx[:, None, b], acc.shape), acc)
    return acc
