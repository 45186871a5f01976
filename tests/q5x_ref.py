"""numpy restatement of the reference's CPU path for Q4_1, Q5_0 and Q5_1 WEIGHTS (ggml.c of
Fcucgvhhhvjv/llama.cpp-q_4_0): the block layouts (ggml.c:877-915), quantize_row_q{4_1,5_0,5_1}_reference
(ggml.c:959-1092), the dequantizers (ggml.c:1520-1592), the AVX2 branch of quantize_row_q8_1 (ggml.c:1402-1463) and
the AVX2 branches of ggml_vec_dot_q4_1_q8_1, ggml_vec_dot_q5_0_q8_0 and ggml_vec_dot_q5_1_q8_1 (ggml.c:2680-2713,
2894-2916, 3144-3169), bit for bit; tests/test_q5x_ref.py checks all of it against the fixtures the compiled
reference wrote (tests/golden/gen_golden_q5x.c).

A type is named by its fixture variant: "q41", "q50", "q51".  Q5_0 multiplies against q8_0 activations
(oracle.quantize_q8_0), the two types with a minimum against q8_1: f32 d, f32 s, qs[32] (40 bytes)."""
import numpy as np

from blk32_ref import fmaf32, gemv_lane_chains
from parity import split_q8_0

QK = 32
Q81B = 40
# variant -> (ggml type, has qh, has min, block bytes)
TYPES = {"q41": (3, False, True, 20), "q50": (6, True, False, 22), "q51": (7, True, True, 24)}
VARIANTS = tuple(TYPES)


def has_qh(t):
    return TYPES[t][1]


def has_min(t):
    return TYPES[t][2]


def block_bytes(t):
    return TYPES[t][3]


def split(t, wq, K):
    """uint8 [M, B K / 32] -> (d f32 [M, nb], m f32 [M, nb] (zeros without a minimum), q int64 [M, nb, 32]): q is the
    stored value 0..15 / 0..31, element j < 16 the low nibble of qs[j], j + 16 the high one, bit e of qh the fifth
    bit of element e."""
    _, qh, mn, B = TYPES[t]
    nb = K // QK
    b = np.ascontiguousarray(wq).reshape(-1, nb, B)
    d = b[:, :, 0:2].copy().view(np.float16)[:, :, 0].astype(np.float32)
    o = 2
    m = np.zeros_like(d)
    if mn:
        m = b[:, :, 2:4].copy().view(np.float16)[:, :, 0].astype(np.float32)
        o = 4
    hi5 = np.zeros(b.shape[:2] + (32,), np.int64)
    if qh:
        h = b[:, :, o:o + 4].copy().view("<u4")[:, :, 0].astype(np.int64)
        hi5 = (h[:, :, None] >> np.arange(32)) & 1
        o += 4
    qs = b[:, :, o:o + 16].astype(np.int64)
    q = np.concatenate([qs & 15, qs >> 4], axis=2) | (hi5 << 4)
    return d, m, q


def split_q8_1(xq, K):
    """uint8 [N, 40 K / 32] -> (d f32 [N, nb], s f32 [N, nb], q int8 [N, nb, 32])."""
    nb = K // QK
    b = np.ascontiguousarray(xq).reshape(-1, nb, Q81B)
    d = b[:, :, 0:4].copy().view(np.float32)[:, :, 0]
    s = b[:, :, 4:8].copy().view(np.float32)[:, :, 0]
    return d, s, b[:, :, 8:40].copy().view(np.int8)


def split_x(t, xq, K):
    """(d, s, q) of the activation rows of type t: q8_1 with a minimum, else q8_0 with s = 0."""
    if has_min(t):
        return split_q8_1(xq, K)
    d, q = split_q8_0(xq, K)
    return d, np.zeros_like(d), q


SPECIAL_BITS = (0x0000, 0x8000, 0x0001, 0x83FF)
SPECIAL_QH = (0x00000000, 0xFFFFFFFF, 0xAAAAAAAA, 0x0000FFFF, 0xFFFF0000)


def random_blocks(rng, M, K, qh, has_min, special=True):
    """uint8 [M, B K / 32]: random nibble bytes and qh over their whole range, finite fp16 d and m of both signs over
    a wide exponent range; with special, a few blocks of d / m = 0, -0 and subnormal, of qh = 0 / all ones / 0xAAAAAAAA
    / the two half masks, and of all-0x00, all-0xFF and 0xF0 nibble bytes."""
    nb = K // QK
    B = 18 + 2 * has_min + 4 * qh
    b = rng.integers(0, 256, (M, nb, B), dtype=np.uint8)
    d = (rng.standard_normal((M, nb)) * np.exp2(rng.integers(-10, 1, (M, nb)))).astype(np.float16)
    b[:, :, 0:2] = d.view(np.uint8).reshape(M, nb, 2)
    if has_min:
        m = (rng.standard_normal((M, nb)) * np.exp2(rng.integers(-8, 3, (M, nb)))).astype(np.float16)
        b[:, :, 2:4] = m.view(np.uint8).reshape(M, nb, 2)
    if special:
        flat = b.reshape(M * nb, B)
        oh = 2 + 2 * has_min
        oq = oh + 4 * qh
        idx = rng.permutation(M * nb)[:12]
        for k, i in enumerate(idx):
            if k < 4:
                flat[i, 0:2] = np.array([SPECIAL_BITS[k]], "<u2").view(np.uint8)
                if has_min:
                    flat[i, 2:4] = np.array([SPECIAL_BITS[(k + 1) % 4]], "<u2").view(np.uint8)
            elif k < 9:
                if qh:
                    flat[i, oh:oh + 4] = np.array([SPECIAL_QH[k - 4]], "<u4").view(np.uint8)
            else:
                flat[i, oq:] = (0x00, 0xFF, 0xF0)[k - 9]
    return b.reshape(M, nb * B)


def dequantize(t, wq, K):
    """dequantize_row_q4_1 / q5_0 / q5_1: q * d + m resp. (q - 16) * d in float32, one multiply and (with a minimum)
    one add -> f32 [M, K]."""
    d, m, q = split(t, wq, K)
    if not has_min(t):
        return ((q - 16).astype(np.float32) * d[:, :, None]).astype(np.float32).reshape(d.shape[0], K)
    p = (q.astype(np.float32) * d[:, :, None]).astype(np.float32)
    return (p + m[:, :, None]).astype(np.float32).reshape(d.shape[0], K)


def quantize_q8_1(x):
    """The AVX2 branch of quantize_row_q8_1: the qs bytes of quantize_row_q8_0 (the oracle's restatement), d =
    amax / 127.f kept as float32, s = d * (float)sum(qs), one float32 multiply -> uint8 [N, 40 K / 32]."""
    import oracle as O
    x = np.ascontiguousarray(x, np.float32)
    N, K = x.shape
    nb = K // QK
    _, q = split_q8_0(O.quantize_q8_0(x, "avx2"), K)
    amax = np.abs(x.reshape(N, nb, QK)).max(axis=2)
    d = (amax / np.float32(127.0)).astype(np.float32)
    s = (d * q.astype(np.int32).sum(axis=2).astype(np.float32)).astype(np.float32)
    out = np.empty((N, nb, Q81B), np.uint8)
    out[:, :, 0:4] = d.view(np.uint8).reshape(N, nb, 4)
    out[:, :, 4:8] = s.view(np.uint8).reshape(N, nb, 4)
    out[:, :, 8:] = q.view(np.uint8)
    return out.reshape(N, nb * Q81B)


def quantize_x(t, x):
    """The activation rows type t multiplies against (quantize_row_q_dot)."""
    import oracle as O
    return quantize_q8_1(x) if has_min(t) else O.quantize_q8_0(np.ascontiguousarray(x, np.float32), "avx2")


def _lane_sums(t, wq, xq, K):
    """(dw, mw, dx, sx, lanes int64 [N, M, nb, 8]): lane j of block b = the sum over elements 4j .. 4j + 3 of the weight
    byte (q, or q - 16 for Q5_0) times the activation byte; maddubs cannot saturate (2 * 31 * 127 < 32767)."""
    dw, mw, w = split(t, wq, K)
    dx, sx, q = split_x(t, xq, K)
    if not has_min(t):
        w = w - 16
    M, nb = dw.shape
    N = dx.shape[0]
    lanes = np.einsum("mbjk,nbjk->nmbj", w.reshape(M, nb, 8, 4), q.reshape(N, nb, 8, 4).astype(np.int64))
    return dw, mw, dx, sx, lanes


def block_terms(t, wq, xq, K):
    """(y_exact f64 [N, M], S_abs f64 [N, M]): y = sum_b (d_w d_x isum_b + m_w s_b), S_abs = sum_b (|d_w d_x isum_b| +
    |m_w s_b|) from the exact integer block sums."""
    dw, mw, dx, sx, lanes = _lane_sums(t, wq, xq, K)
    isum = lanes.sum(axis=3)
    a = dx.astype(np.float64)[:, None, :] * dw.astype(np.float64)[None, :, :] * isum
    b = sx.astype(np.float64)[:, None, :] * mw.astype(np.float64)[None, :, :]
    return (a + b).sum(axis=2), (np.abs(a) + np.abs(b)).sum(axis=2)


def vec_dot_avx2(t, wq, xq, K, summs_fma=False):
    """f32 [N, M]: the AVX2 branch of the type's ggml_vec_dot, bit for bit.  Per block, d = fp32(d_w) * d_x rounded to
    float32 and acc_j = fmaf(d, (float)lane_j, acc_j) for the eight lanes, blocks in order; then hsum_float_8: (a_k +
    a_{k+4}), k with k + 2, the last pair.  With a minimum, summs += fp32(m) * s runs as its own serial chain and is
    added last.  What the fixtures settled: the compiled reference (gcc -O2 -std=c11: no contraction) forms that
    step as a float32 MULTIPLY rounded to float32 and then a float32 ADD, not as one fma (summs_fma=True computes the
    fma form, which the K = 2304 and 4160 fixtures of both types reject)."""
    dw, mw, dx, sx, lanes = _lane_sums(t, wq, xq, K)
    N, M, nb, _ = lanes.shape
    d = (dx[:, None, :] * dw[None, :, :]).astype(np.float32)
    lf = lanes.astype(np.float32)                       # exact: |lane| <= 4 * 31 * 127
    acc = np.zeros((N, M, 8), np.float32)
    summs = np.zeros((N, M), np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for b in range(nb):
            acc = fmaf32(np.broadcast_to(d[:, :, b, None], acc.shape), lf[:, :, b, :], acc)
            if has_min(t) and summs_fma:
                summs = fmaf32(np.broadcast_to(mw[None, :, b], summs.shape), np.broadcast_to(sx[:, None, b], summs.shape),
                               summs)
            elif has_min(t):
                summs = (summs + (mw[None, :, b] * sx[:, None, b]).astype(np.float32)).astype(np.float32)
        r = (acc[:, :, 0:4] + acc[:, :, 4:8]).astype(np.float32)
        r = (r[:, :, 0:2] + r[:, :, 2:4]).astype(np.float32)
        r = (r[:, :, 0] + r[:, :, 1]).astype(np.float32)
        return (r + summs).astype(np.float32) if has_min(t) else r


def gemv_schedule(t, wq, x, K):
    """f32 [N, M]: k_gemv_blk32's own fp32 order on weights of type t against f32 x [N, K].  x per block: Q5_0 takes
    q8_block_lane's bytes with d_x = fp32(fp16(amax / 127.f)), and its block sum has the integer 16 * sum q taken off
    (here: the weights as q - 16, the same integer); the types with a minimum take the unrounded d_x = amax / 127.f
    and s_x = d_x * (float)sum q, one rounded multiply (quantize_q8_1).  The lane chains and the tree are
    blk32_ref.gemv_lane_chains."""
    dw, mw, dx, sx, lanes = _lane_sums(t, wq, quantize_x(t, x), K)
    isum = lanes.sum(axis=3).astype(np.float32)         # exact: |isum| <= 32 * 31 * 127 < 2^24
    dd = (dw[None, :, :] * dx[:, None, :]).astype(np.float32)
    return gemv_lane_chains(isum, dd, mw, sx) if has_min(t) else gemv_lane_chains(isum, dd)


def _pack(t, d, m, q):
    """blocks from float32 d, m [M, nb] and the quantized values q uint8 [M, nb, 32]."""
    _, qh, mn, B = TYPES[t]
    M, nb = d.shape
    out = np.empty((M, nb, B), np.uint8)
    out[:, :, 0:2] = d.astype(np.float16).view(np.uint8).reshape(M, nb, 2)
    o = 2
    if mn:
        out[:, :, 2:4] = m.astype(np.float16).view(np.uint8).reshape(M, nb, 2)
        o = 4
    if qh:
        bits = ((q.astype(np.uint64) >> 4) & 1) << np.arange(32, dtype=np.uint64)
        out[:, :, o:o + 4] = bits.sum(axis=2).astype("<u4").view(np.uint8).reshape(M, nb, 4)
        o += 4
    out[:, :, o:] = (q[:, :, :16] & 15) | ((q[:, :, 16:] & 15) << 4)
    return out.reshape(M, nb * B)


def quantize_w(t, w):
    """quantize_row_q4_1_reference / q5_0 / q5_1 (ggml.c:959-1092) of f32 [M, K], every step in float32 (the values
    before the truncating cast are non-negative, so truncation is floor)."""
    w = np.ascontiguousarray(w, np.float32)
    M, K = w.shape
    x = w.reshape(M, K // QK, QK)
    f = np.float32
    with np.errstate(divide="ignore", invalid="ignore"):
        if t == "q50":
            i = np.abs(x).argmax(axis=2)                # the first element of the largest magnitude
            mx = np.take_along_axis(x, i[:, :, None], axis=2)[:, :, 0]
            d = (mx / f(-16)).astype(f)
            inv = np.where(d != 0, (f(1) / d).astype(f), f(0)).astype(f)
            v = ((x * inv[:, :, None]).astype(f) + f(16.5)).astype(f)
            q = np.minimum(31, v.astype(np.int32).astype(np.int8)).astype(np.uint8)
            return _pack(t, d, None, q)
        lo, hi = x.min(axis=2), x.max(axis=2)
        levels = 15 if t == "q41" else 31
        d = ((hi - lo).astype(f) / f(levels)).astype(f)
        inv = np.where(d != 0, (f(1) / d).astype(f), f(0)).astype(f)
        v = (((x - lo[:, :, None]).astype(f) * inv[:, :, None]).astype(f) + f(0.5)).astype(f)
        q = v.astype(np.int32)
        q = np.minimum(15, q.astype(np.int8)).astype(np.uint8) if t == "q41" else q.astype(np.uint8)
        return _pack(t, d, lo, q)
