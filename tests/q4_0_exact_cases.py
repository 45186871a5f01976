"""Order-free exact cases for the q4_0 x q8_0 fast path (numpy), and the shapes the GPU module runs.

An order-free case is a q4_0 weight matrix and an f32 activation matrix on which every legal order of the
fp32 arithmetic of a correct kernel gives the same bits, so y must equal float32(y64) with no tolerance:

  weights      written as q4_0 blocks directly: d_w = +-2^e (fp16 bits), e in a window of span_w + 1 adjacent
               exponents, nibbles uniform over 0..15;
  activations  x[n, 32b + j] = q[n, b, j] * 2^f[n, b] with integer |q| <= qmax and exactly one element per block
               forced to +-127, f in a window of span_x + 1 exponents inside fp16's normal range.

Then amax = 127 * 2^f, d = amax / 127 = 2^f exactly, id = 2^-f exactly and x * id = q exactly: any correct q8_0
quantizer (AVX2 ties included: there are no ties) returns exactly d and q.  Every term d_w d_x sumi is an integer
multiple of unit = 2^(min e + min f), and build() asserts for every (n, m)

    sum_b |d_w d_x| * (sum_j nib |q| + 8 sum_j |q|) < 2^23 * unit,

which bounds every partial sum of every order (with or without fma, across split-K slabs, and for a kernel that
keeps the unsigned-nibble dot and the -8 sum(q) correction apart) below 2^23 units: all of them are exact in fp32.
"""
import functools

import numpy as np

from parity import QK, split_q4_0, split_q8_0

E_W0 = -9            # lowest d_w exponent of a window (2^-9 .. 2^-5: the scale of 0.02-sigma weights)
F_X0 = -6            # lowest d_x exponent of a window (fp16 normal range is 2^-14 .. 2^15)

# (largest K, span_w, span_x, qmax): the windows whose headroom was checked per K; a K between two rows takes
# the next larger row's (narrower) windows
WINDOWS = [(64, 4, 3, 127), (256, 3, 2, 127), (1024, 2, 1, 127), (4096, 1, 0, 127), (4544, 1, 0, 127),
           (11008, 0, 0, 15), (13824, 0, 0, 15)]


def windows_for(K):
    for kmax, sw, sx, qmax in WINDOWS:
        if K <= kmax:
            return sw, sx, qmax
    raise ValueError(f"no exponent windows for K = {K}")


def exact_terms(wq, xq, K):
    """block_terms (y64 and S_abs [N, M], float64) one block at a time: the integer block sums through float32 BLAS
    (every partial sum is an integer below 2^24, so exact), the scale product and the sums in float64: parity.block_terms
    without its [N, M, nb] intermediates (the same values exactly on an order-free case, to float64 rounding otherwise)."""
    dw, w = split_q4_0(wq, K)
    dx, q = split_q8_0(xq, K)
    wf, qf = w.astype(np.float32), q.astype(np.float32)
    dw, dx = dw.astype(np.float64), dx.astype(np.float64)
    y = np.zeros((q.shape[0], w.shape[0]))
    s = np.zeros_like(y)
    for b in range(K // QK):
        t = (qf[:, b, :] @ wf[:, b, :].T).astype(np.float64) * (dx[:, b, None] * dw[None, :, b])
        y += t
        s += np.abs(t)
    return y, s


def build(e, sign, nib, q, f):
    """e, sign [M, nb] (d_w = sign * 2^e), nib [M, nb, 32] in 0..15, q [N, nb, 32] int with max |q| = 127 per
    block, f [N, nb] -> dict(wq, x, xq, y64, s_abs, mag_log2); asserts the headroom condition."""
    M, nb = e.shape
    N = q.shape[0]
    assert np.all(np.abs(q).max(axis=2) == 127), "every block needs one element at +-127"
    assert nib.min() >= 0 and nib.max() <= 15
    assert e.min() >= -14 and e.max() <= 15 and f.min() >= -14 and f.max() <= 15
    dw = (sign * np.exp2(e.astype(np.float64))).astype(np.float16)
    wq = np.empty((M, nb, 18), np.uint8)
    wq[:, :, 0:2] = dw[:, :, None].view(np.uint8)
    wq[:, :, 2:18] = (nib[:, :, :16] | (nib[:, :, 16:] << 4)).astype(np.uint8)
    dx = np.exp2(f.astype(np.float64))
    x = (q * dx[:, :, None]).astype(np.float32).reshape(N, nb * QK)
    xq = np.empty((N, nb, 34), np.uint8)
    xq[:, :, 0:2] = dx.astype(np.float16)[:, :, None].view(np.uint8)
    xq[:, :, 2:34] = q.astype(np.int8).view(np.uint8)
    wq, xq = wq.reshape(M, nb * 18), xq.reshape(N, nb * 34)
    # headroom, in units of 2^(min e + min f): float64 sums of integers far below 2^53 are exact
    aq, nf = np.abs(q).astype(np.float32), nib.astype(np.float32)
    sw, sx = np.exp2((e - e.min()).astype(np.float64)), np.exp2((f - f.min()).astype(np.float64))
    mag = np.zeros((N, M))
    for b in range(nb):                                   # float32 BLAS on integers below 2^24: exact
        inner = (aq[:, b, :] @ nf[:, b, :].T).astype(np.float64) + 8.0 * aq[:, b, :].sum(axis=1, dtype=np.float64)[:, None]
        mag += inner * (sx[:, b, None] * sw[None, :, b])
    assert mag.max() < 2.0 ** 23, f"no headroom: 2^{np.log2(mag.max()):.2f} units"
    y64, s_abs = exact_terms(wq, xq, nb * QK)
    for a in (wq, x, xq, y64, s_abs):
        a.setflags(write=False)
    return dict(wq=wq, x=x, xq=xq, y64=y64, s_abs=s_abs, mag_log2=float(np.log2(mag.max())),
                unit_log2=int(e.min() + f.min()))


def draw(K, M, N, seed, span_w, span_x, qmax=127):
    """The random parts of an order-free case: (e, sign, nib, q, f)."""
    assert K % 64 == 0
    nb = K // QK
    rng = np.random.default_rng(seed)
    e = rng.integers(E_W0, E_W0 + span_w + 1, (M, nb))
    sign = rng.choice(np.array([-1.0, 1.0]), (M, nb))
    nib = rng.integers(0, 16, (M, nb, QK))
    q = rng.integers(-qmax, qmax + 1, (N, nb, QK))
    j = rng.integers(0, QK, (N, nb))
    np.put_along_axis(q, j[:, :, None], rng.choice(np.array([-127, 127]), (N, nb))[:, :, None], axis=2)
    f = rng.integers(F_X0, F_X0 + span_x + 1, (N, nb))
    return e, sign, nib, q, f


def order_free_case(K, M, N, seed, span_w, span_x, qmax=127):
    """q4_0 bytes wq [M, K/32*18], x f32 [N, K], the q8_0 bytes xq [N, K/32*34] x must quantize to, y64 and S_abs
    [N, M] (a dict, arrays read-only)."""
    return build(*draw(K, M, N, seed, span_w, span_x, qmax))


@functools.lru_cache(maxsize=None)
def order_free(K, M, N, seed=0):
    """order_free_case at the windows of K (cached: the arrays are read-only and shared among tests)."""
    return order_free_case(K, M, N, 0x0F00 + seed, *windows_for(K))


@functools.lru_cache(maxsize=None)
def extreme_order_free(K=256, M=64, N=160):
    """The order-free twin of the fp6 extreme-blocks case: rows of all-0 (w = -8) and all-15 (w = 7) nibbles,
    tokens whose q are all +127, all -127, and 0 except the forced element: the largest block sums
    (|sumi| = 32 * 8 * 127) and every e2m3 code at its extremes.  Windows span_w = 2, span_x = 1: the worst block
    is 23 * 127 * 32 units, times 2^3 over 8 blocks = 2^22.5."""
    e, sign, nib, q, f = draw(K, M, N, 0x0E00, 2, 1)
    nib[:8] = 0
    nib[8:16] = 15
    nib[16:24, ::2] = 0
    nib[16:24, 1::2] = 15
    q[:8] = 127
    q[8:16] = -127
    forced = np.abs(q[16:24]) == 127
    q[16:24] = np.where(forced & (np.cumsum(forced, axis=2) == 1), q[16:24], 0)    # one +-127, 31 zeros
    q[24:32, :, ::2] = 127
    q[24:32, :, 1::2] = -127
    return build(e, sign, nib, q, f)


# ------------------------------------------------------------------------------------------- gaussian cases
def gaussian_case(O, K, M, N, seed, spread=False):
    """make_case of tests/test_gpu_parity.py (spread: x with a per-block scale spread, as in
    test_q8_0_bitexact_random_scales), the oracle's q8_0 bytes of x, and block_terms on them."""
    wq, _ = O.quantize_q4_0(O.gaussian(M * K, 0x5EED0000 + seed, 0.0, 0.02).reshape(M, K))
    if spread:
        rng = np.random.default_rng(seed)
        x = (rng.standard_normal((N, K)) * np.exp(rng.uniform(-12, 10, (N, K // QK))).repeat(QK, 1)).astype(np.float32)
    else:
        x = O.gaussian(N * K, 0x5EED1000 + seed, 0.0, 1.0).reshape(N, K)
    xq = O.quantize_q8_0(x, "avx2")
    y64, s_abs = exact_terms(wq, xq, K)
    for a in (wq, x, xq, y64, s_abs):
        a.setflags(write=False)
    return dict(wq=wq, x=x, xq=xq, y64=y64, s_abs=s_abs)


_gauss_cache = {}


def gaussian(O, K, M, N, spread=False):
    key = (K, M, N, spread)
    if key not in _gauss_cache:
        _gauss_cache[key] = gaussian_case(O, K, M, N, seed=K * 11 + M * 3 + N, spread=spread)
    return _gauss_cache[key]


# ------------------------------------------------------------------------------------------- the GPU module's shapes
GEMV_KM = [(64, 1), (64, 37), (256, 129), (1024, 333), (4544, 73)]      # (4544, 73): rows only 4-byte aligned
GEMV_N = [1, 3, 8]
GEMV_SHAPES = [(K, M, N) for K, M in GEMV_KM for N in GEMV_N] + [(11008, 33, 1)] + \
    [(256, 129, N) for N in (2, 4, 5, 6, 7)]        # 172 pairs: 3 per lane; the other token-count instantiations
BAL_SHAPES = [(12352, 17, 1), (13824, 65, 1)]                           # K > 12288: chunk items, balance on / off
SPLITK_SHAPES = [(64, 130, 9),           # fewer blocks than K splits
                 (256, 129, 31), (1024, 64, 33), (4544, 200, 65), (1024, 65, 128),
                 (1088, 4100, 128)]      # 516 tiles, two rounds of 256 CUs: the 8-wave form (17 pairs: 3, 3, 3, 3, 3, 2)
GEMM_SHAPES = [(64, 130, 9),             # one half stage
               (128, 1, 200), (256, 129, 65),
               (1024, 200, 130),         # ragged in both tile sizes
               (4544, 73, 33)]           # partial last stage
IMAGE_SHAPES = [(1024, 200, 130), (4544, 73, 65)]
CHAIN_SPEC = [(1024, [320]), (320, [200, 64])]      # (K, [M...]): task 1 reads task 0's y as x
EXTREME_SHAPE = (256, 64, 160)


def all_shapes():
    """Every (K, M, N) the GPU module builds a case at."""
    chain = [(CHAIN_SPEC[0][0], CHAIN_SPEC[0][1][0], 1)]
    return sorted(set(GEMV_SHAPES + BAL_SHAPES + SPLITK_SHAPES + GEMM_SHAPES + IMAGE_SHAPES + chain))
