"""numpy restatement of the F16-weight GEMV's order of additions (csrc/f16_w.hip, k_gemv_f16w): y[n][m] = sum_e
W[m][e] * fp16(x[n][e]) with the semantics of ggml_compute_forward_mul_mat_f16_f32 (ggml.c:11026: x rounded to fp16,
round to nearest even) in the kernel's own fixed fp32 order.  A product of two fp16 values is exact in float32 (22
significant bits, exponents far inside the range), so each fma of the kernel is ONE float32 addition of an exact
product and plain float32 numpy reproduces it.

The order, which depends on K alone: steps of 512 elements; lane l of 64 owns elements 512 s + 8 l .. + 7 of step s
and keeps two chains from +0, chain 0 over the even elements (+0, +2, +4, +6) and chain 1 over the odd ones, in that
order, steps in increasing s; in the last step of a K that is no multiple of 512 the lanes at or past K add nothing.
Then t_l = c0_l + c1_l and the 64 t_l as the balanced binary tree over the lanes in order."""
import numpy as np

from ggml_ops_ref import fp16_bits, fp16_to_f32

STEP, LANES = 512, 64


def random_case(rng, M, K, N, special=False):
    """(w uint16 [M, K] F16 bit patterns of 0.5 N(0, 1), x f32 [N, K] of N(0, 1)); special: fp16 subnormals and +-0 in
    w and |x| up to 6e4 as well"""
    w = (rng.standard_normal((M, K)) * 0.5).astype(np.float16)
    x = rng.standard_normal((N, K)).astype(np.float32)
    if special:
        flat = w.reshape(-1).view(np.uint16)
        idx = rng.choice(flat.size, min(flat.size // 2, 64), replace=False)
        pats = np.array([0x0000, 0x8000, 0x0001, 0x8001, 0x03FF, 0x83FF, 0x0200, 0x0400], np.uint16)
        flat[idx] = pats[np.arange(idx.size) % pats.size]
        xf = x.reshape(-1)
        jdx = rng.choice(xf.size, min(xf.size // 2, 64), replace=False)
        big = np.array([6e4, -6e4, 65000.0, -1234.5, 3e4, 5.9604645e-8, -0.0, 1e-9], np.float32)
        xf[jdx] = big[np.arange(jdx.size) % big.size]
    return np.ascontiguousarray(w.view(np.uint16)), x


def operands(w16, x32):
    """(w f32 [M, K], fp16(x) as f32 [N, K]): the exact values the products are formed of"""
    w16 = np.asarray(w16)
    w = (w16.view(np.float16) if w16.dtype == np.uint16 else w16.astype(np.float16)).astype(np.float32)
    xh = fp16_to_f32(fp16_bits(x32)).reshape(np.shape(x32))
    return w, xh


def gemv_schedule(w16, x32):
    """f32 [N, M]: k_gemv_f16w's result, bit for bit"""
    w, xh = operands(w16, x32)
    M, K = w.shape
    N = xh.shape[0]
    assert K % 32 == 0 and xh.shape[1] == K
    nsteps = (K + STEP - 1) // STEP
    pad = nsteps * STEP - K                                   # the lanes past K: products of +0, skipped below
    wp = np.pad(w, ((0, 0), (0, pad))).reshape(M, nsteps, LANES, 4, 2)
    xp = np.pad(xh, ((0, 0), (0, pad))).reshape(N, nsteps, LANES, 4, 2)
    live = (np.arange(nsteps)[:, None] * STEP + np.arange(LANES)[None, :] * 8) < K      # [step, lane]
    c = np.zeros((N, M, LANES, 2), np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for s in range(nsteps):
            for j in range(4):
                p = (wp[None, :, s, :, j, :] * xp[:, None, s, :, j, :]).astype(np.float32)    # exact
                c = np.where(live[s][None, None, :, None], (c + p).astype(np.float32), c)
        t = (c[..., 0] + c[..., 1]).astype(np.float32)
        while t.shape[-1] > 1:
            t = (t[..., 0::2] + t[..., 1::2]).astype(np.float32)
    return t[..., 0]


def exact_terms(w16, x32):
    """(y f64 [N, M], S_abs f64 [N, M]): the float64 sum of the fp16 products and the sum of their magnitudes"""
    w, xh = operands(w16, x32)
    w64, x64 = w.astype(np.float64), xh.astype(np.float64)
    return x64 @ w64.T, np.abs(x64) @ np.abs(w64).T


# The shapes of tests/test_gpu_f16w.py, shared with tests/test_f16w_ref.py (which shows on the CPU that the restated
# order differs from ggml_vec_dot_f16's on these very inputs).  K: one ragged step (32), 512 + 32 (544), two steps and
# a ragged 480 (1504), the 21.5 steps of the LLaMA-7B w2 (11008, where a launch takes 5 columns: N = 8, 9 and 17 are
# tiled there, N = 9, 17 and 40 everywhere).  (K, M, N, ldy - M, special)
CASES = [(32, 1, 1, 0, False), (32, 130, 40, 0, False), (544, 3, 7, 0, False), (544, 65, 2, 0, False),
         (544, 130, 9, 0, False), (1504, 3, 8, 0, False), (1504, 65, 17, 0, False), (1504, 130, 1, 5, False),
         (1504, 65, 7, 0, True), (11008, 3, 1, 0, False), (11008, 65, 8, 0, False), (11008, 1, 9, 0, False),
         (11008, 130, 2, 3, False), (11008, 3, 17, 0, False)]
_cache = {}


def case(i):
    """(w16, x, the restated y) of CASES[i], computed once per process"""
    if i not in _cache:
        K, M, N, _, special = CASES[i]
        w16, x = random_case(np.random.default_rng([0xF16, i]), M, K, N, special)
        y = gemv_schedule(w16, x)
        for a in (w16, x, y):
            a.setflags(write=False)
        _cache[i] = (w16, x, y)
    return _cache[i]
