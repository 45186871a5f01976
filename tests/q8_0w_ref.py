"""numpy restatement of the reference's CPU path for Q8_0 WEIGHTS (ggml.c of Fcucgvhhhvjv/llama.cpp-q_4_0):
dequantize_row_q8_0 (ggml.c:1594-1610) and the AVX2 branch of ggml_vec_dot_q8_0_q8_0 (ggml.c:3231-3320), bit for
bit; tests/test_q8_0w_ref.py checks both against the fixtures the compiled reference wrote
(tests/golden/gen_golden_q8_0w.c).  The activation side is the reference's quantize_row_q8_0, which the oracle
restates (oracle.quantize_q8_0, bit-exact)."""
import numpy as np

from blk32_ref import fmaf32, gemv_lane_chains
from parity import split_q8_0

QK = 32
Q8B = 34


def random_q8_0(rng, M, K, special=True):
    """uint8 [M, 34 K / 32]: random qs over the whole int8 range (-128 included) and finite fp16 d of both signs
    over a wide exponent range; with special, a few blocks of d = 0 / -0 / subnormal and of all -128 / +127."""
    nb = K // QK
    b = np.empty((M, nb, Q8B), np.uint8)
    b[:, :, 2:] = rng.integers(0, 256, (M, nb, 32), dtype=np.uint8)
    d = (rng.standard_normal((M, nb)) * np.exp2(rng.integers(-10, 1, (M, nb)))).astype(np.float16)
    b[:, :, 0:2] = d.view(np.uint8).reshape(M, nb, 2)
    if special:
        k = min(M * nb, 8)
        flat = b.reshape(M * nb, Q8B)
        idx = rng.choice(M * nb, k, replace=False)
        pats = [(0x0000, None), (0x8000, None), (0x0001, None), (0x83FF, None), (None, 0x80), (None, 0x7F)]
        for i, (dbits, q) in zip(idx, pats):
            if dbits is not None:
                flat[i, 0:2] = np.array([dbits], np.uint16).view(np.uint8)
            if q is not None:
                flat[i, 2:] = q
    return b.reshape(M, nb * Q8B)


def dequantize_q8_0(wq, K):
    """dequantize_row_q8_0: (float)q * fp32(d), one float32 multiply -> f32 [M, K]."""
    d, q = split_q8_0(wq, K)
    return (q.astype(np.float32) * d[:, :, None]).astype(np.float32).reshape(d.shape[0], K)


def _lane_sums(wq, xq, K):
    """int64 [N, M, nb, 8]: lane j of block b = sum of w_e q_e over e = 4j .. 4j + 3 (mul_sum_i8_pairs_float: exact
    for every int8 weight, -128 included, against activations in [-127, 127])."""
    dw, w = split_q8_0(wq, K)
    dx, q = split_q8_0(xq, K)
    M, nb = dw.shape
    N = dx.shape[0]
    wg = w.reshape(M, nb, 8, 4).astype(np.int64)
    xg = q.reshape(N, nb, 8, 4).astype(np.int64)
    return dw, dx, np.einsum("mbjk,nbjk->nmbj", wg, xg)


def block_terms(wq, xq, K):
    """(y_exact f64 [N, M], S_abs f64 [N, M]) from the exact integer block sums: y = sum_b d_x d_w isum_b,
    S_abs = sum_b |d_x d_w isum_b| (the form of parity.block_terms, on Q8_0 weights)."""
    dw, dx, lanes = _lane_sums(wq, xq, K)
    isum = lanes.sum(axis=3)
    assert np.abs(isum).max(initial=0) <= 32 * 128 * 127
    t = dx.astype(np.float64)[:, None, :] * dw.astype(np.float64)[None, :, :] * isum
    return t.sum(axis=2), np.abs(t).sum(axis=2)


def vec_dot_avx2(wq, xq, K):
    """f32 [N, M]: the AVX2 branch of ggml_vec_dot_q8_0_q8_0, bit for bit: per block, d = fp32(d_w) * fp32(d_x)
    rounded to float32, acc_j = fmaf(d, (float)lane_j, acc_j) for the eight lanes, blocks in order, then
    hsum_float_8: (a_k + a_{k+4}), then k with k + 2, then the last pair."""
    dw, dx, lanes = _lane_sums(wq, xq, K)
    N, M, nb, _ = lanes.shape
    d = (dx[:, None, :] * dw[None, :, :]).astype(np.float32)
    lf = lanes.astype(np.float32)                       # exact: |lane| <= 4 * 128 * 127
    acc = np.zeros((N, M, 8), np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for b in range(nb):
            acc = fmaf32(np.broadcast_to(d[:, :, b, None], acc.shape), lf[:, :, b, :], acc)
        r = (acc[:, :, 0:4] + acc[:, :, 4:8]).astype(np.float32)
        r = (r[:, :, 0:2] + r[:, :, 2:4]).astype(np.float32)
        return (r[:, :, 0] + r[:, :, 1]).astype(np.float32)


def gemv_schedule(wq, x, K):
    """f32 [N, M]: k_gemv_blk32's own fp32 order on Q8_0 weights against f32 x [N, K].  x per block is q8_block_lane's:
    the q8_0 bytes and d_x = fp32(fp16(amax / 127.f)); the lane chains and the tree are blk32_ref.gemv_lane_chains."""
    import oracle as O
    dw, dx, lanes = _lane_sums(wq, O.quantize_q8_0(np.ascontiguousarray(x, np.float32), "avx2"), K)
    isum = lanes.sum(axis=3).astype(np.float32)         # exact: |isum| <= 32 * 128 * 127 < 2^24
    dd = (dw[None, :, :] * dx[:, None, :]).astype(np.float32)
    return gemv_lane_chains(isum, dd)


def q4_0_as_q8_0(w4q, K):
    """A q4_0 matrix as Q8_0 rows with the same values: qs = nibble - 8 in dequantize_row_q4_0's element order
    (element j = low nibble of qs[j], j + 16 = high nibble), the same fp16 d."""
    nb = K // QK
    b4 = np.ascontiguousarray(w4q).reshape(-1, nb, 18)
    out = np.empty((b4.shape[0], nb, Q8B), np.uint8)
    out[:, :, 0:2] = b4[:, :, 0:2]
    qs = b4[:, :, 2:18]
    out[:, :, 2:18] = ((qs & 0x0F).astype(np.int8) - 8).view(np.uint8)
    out[:, :, 18:34] = ((qs >> 4).astype(np.int8) - 8).view(np.uint8)
    return out.reshape(b4.shape[0], nb * Q8B)
