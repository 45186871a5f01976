"""What the restatements of the 32-weight block types (Q8_0, Q4_1, Q5_0, Q5_1: tests/q8_0w_ref.py, tests/q5x_ref.py,
tests/q5x_gemm_ref.py) share: a correctly rounded float32 fma on numpy arrays, and the fp32 order of the fused GEMV
(k_gemv_blk32, csrc/blk32_w.hip), which is the same for the four types: 64 lane chains per row and the wave's DPP
tree."""
import numpy as np


def fmaf32(a, b, c):
    """float32 fma(a, b, c), correctly rounded, for float32 arrays whose product a * b is exact in float64 (here: a
    24-bit scale times an integer below 2^20, or an fp16 minimum times a float32).  p + c is formed in float64
    rounded to ODD (TwoSum gives the rounding error; an inexact even result moves to its odd neighbour), so that the
    final rounding to float32 is the single rounding of the exact sum (53 >= 2 * 24 + 2 bits)."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    other = np.nextafter(s, np.where(err > 0, np.inf, -np.inf))
    even = (s.view(np.int64) & 1) == 0
    s = np.where((err != 0) & even, other, s)
    return s.astype(np.float32)


def wave_sum_lane63(v):
    """f32 [..., 64] -> f32 [...]: wave_sum_lane63 (q4_0_device.h) as lane 63 sees it.  Float addition is commutative,
    so the DPP steps (quad xor 1, quad xor 2, half mirror, row mirror) are the balanced pairwise tree over lanes in
    natural order up to the four 16-lane rows, and the two broadcasts leave (row3 + row2) + (row1 + row0)."""
    f = np.float32
    while v.shape[-1] > 4:
        v = (v[..., 0::2] + v[..., 1::2]).astype(f)
    return ((v[..., 3] + v[..., 2]).astype(f) + (v[..., 1] + v[..., 0]).astype(f)).astype(f)


def gemv_lane_chains(isum, dd, mw=None, sx=None):
    """f32 [N, M]: the fused GEMV's fp32 order.  isum f32 [N, M, nb] = (float) of the exact integer block sums, dd f32
    [N, M, nb] = d_w * d_x rounded to float32, and for the types with a minimum mw f32 [M, nb], sx f32 [N, nb].  Pair
    p of a row (blocks 2p, 2p + 1) belongs to lane p % 64; a lane walks its pairs in increasing p from acc = +0, per
    pair block A then block B: acc = fmaf(isum, dd, acc), with a minimum acc = fmaf(m_w, s_x, acc) right after it;
    lanes without a pair stay at +0; then wave_sum_lane63."""
    N, M, nb = isum.shape
    npairs = nb // 2
    acc = np.zeros((N, M, 64), np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for p0 in range(0, npairs, 64):
            n = min(64, npairs - p0)
            for k in (0, 1):
                b = 2 * (p0 + np.arange(n)) + k
                acc[:, :, :n] = fmaf32(isum[:, :, b], dd[:, :, b], acc[:, :, :n])
                if mw is not None:
                    shape = (N, M, n)
                    acc[:, :, :n] = fmaf32(np.broadcast_to(mw[None, :, b], shape), np.broadcast_to(sx[:, None, b], shape),
                                           acc[:, :, :n])
        return wave_sum_lane63(acc)
