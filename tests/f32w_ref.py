"""numpy restatements of the F32-weight mul_mats (csrc/f32_w.hip, csrc/f32_w_gemm.hip): y[n][m] = sum_e W[m][e] * x[n][e]
with the semantics of ggml_compute_forward_mul_mat_f32 (ggml.c:10855): no operand is rounded, every product enters by
an fma with one rounding (ggml_ops_ref.fma32), fp32 subnormals are kept.  Three orders of the same sum:

  vec_dot_f32 / mul_mat_f32   ggml_vec_dot_f32 (ggml.c:2266) in its AVX2 + FMA schedule (GGML_F32_STEP 32, GGML_F32_EPR
      8): 32 chains, chain e % 32 takes element e in order from +0; GGML_F32x8_REDUCE: (v0 + v2) + (v1 + v3), the low
      half + the high half, (t0 + t1) + (t2 + t3).  K % 32 == 0 (the scalar leftover loop is the compiler's to contract).
      The exact kernel (algo 4) gives these bits; tests/golden/f32w_*.bin pin them to ggml's own CPU op.
  gemv_schedule               k_gemv_f32w (algo 1): steps of 256 elements; lane l of 64 owns elements 256 s + 4 l .. + 3 of
      step s and keeps two chains from +0, chain 0 over elements +0, +2 and chain 1 over +1, +3, in that order, steps in
      increasing s; in the last step of a K that is no multiple of 256 the lanes at or past K add nothing.  Then
      t_l = c0_l + c1_l and the 64 t_l as the balanced binary tree over the lanes in order.
  gemm_schedule(w, x, S)      k_gemm_f32w (algo 12): S equal slices of K; per slice one chain acc = fma(w[e], x[e], acc)
      over the slice's elements in natural order from +0; S = 1 is the chain's value, S > 1 is ((a_0 + a_1) + a_2) + a_3.
      A requested S for which K / S is no multiple of 32 runs as the next smaller one (gemm_ksplit)."""
import numpy as np

from ggml_ops_ref import fma32

STEP, LANES = 256, 64


def random_case(rng, M, K, N, special=False):
    """(w f32 [M, K] of 0.5 N(0, 1), x f32 [N, K] of N(0, 1)); special: +-0, subnormal weights and products, a weight of
    magnitude 2^-130 against large x, and magnitudes spread over 2^+-20 as well"""
    w = (rng.standard_normal((M, K)) * 0.5).astype(np.float32)
    x = rng.standard_normal((N, K)).astype(np.float32)
    if special:
        w *= np.exp2(rng.integers(-20, 21, (M, K))).astype(np.float32)
        wf = w.reshape(-1)
        idx = rng.choice(wf.size, min(wf.size // 2, 96), replace=False)
        pats = np.array([0.0, -0.0, 2.0 ** -130, -2.0 ** -130, 2.0 ** -149, 1e-30, -3e-39, 2.0 ** -126], np.float32)
        wf[idx] = pats[np.arange(idx.size) % pats.size]
        xf = x.reshape(-1)
        jdx = rng.choice(xf.size, min(xf.size // 2, 96), replace=False)
        big = np.array([2.0 ** 20, -2.0 ** 22, 1e-12, -0.0, 3e4, 2.0 ** -100, 0.0, -1e-20], np.float32)
        xf[jdx] = big[np.arange(jdx.size) % big.size]
        w[0, :] = 0.0                                         # a row whose only survivor is a subnormal weight: 2^-130 *
        w[0, 5] = np.float32(2.0 ** -130)                     # 2^20 = 2^-110, which a flush of the operand would lose
        x[:, 5] = np.float32(2.0 ** 20)
    return np.ascontiguousarray(w), np.ascontiguousarray(x)


def _tree(t):
    while t.shape[-1] > 1:
        t = (t[..., 0::2] + t[..., 1::2]).astype(np.float32)
    return t[..., 0]


def vec_dot_f32(w, x):
    """ggml_vec_dot_f32 of rows w [..., K] and x [..., K] in the AVX2 + FMA schedule; the leading axes broadcast"""
    w, x = np.asarray(w, np.float32), np.asarray(x, np.float32)
    K = w.shape[-1]
    assert x.shape[-1] == K and K % 32 == 0
    lead = np.broadcast(w[..., 0], x[..., 0]).shape
    acc = np.zeros(lead + (32,), np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(0, K, 32):
            acc = fma32(w[..., i:i + 32], x[..., i:i + 32], acc)
        v = acc.reshape(lead + (4, 8))
        v0 = (v[..., 0, :] + v[..., 2, :]).astype(np.float32)
        v1 = (v[..., 1, :] + v[..., 3, :]).astype(np.float32)
        v0 = (v0 + v1).astype(np.float32)
        t0 = (v0[..., 0:4] + v0[..., 4:8]).astype(np.float32)
        t1a = (t0[..., 0] + t0[..., 1]).astype(np.float32)
        t1b = (t0[..., 2] + t0[..., 3]).astype(np.float32)
        return (t1a + t1b).astype(np.float32)


def mul_mat_f32(w, x):
    """ggml_compute_forward_mul_mat_f32: w [M, K], x [N, K] -> [N, M], dst[n][m] = vec_dot_f32(w[m], x[n])"""
    w, x = np.asarray(w, np.float32), np.asarray(x, np.float32)
    return vec_dot_f32(w[None, :, :], x[:, None, :])


def gemv_schedule(w, x):
    """f32 [N, M]: k_gemv_f32w's result, bit for bit"""
    w, x = np.asarray(w, np.float32), np.asarray(x, np.float32)
    M, K = w.shape
    N = x.shape[0]
    assert K % 32 == 0 and x.shape[1] == K
    nsteps = (K + STEP - 1) // STEP
    pad = nsteps * STEP - K                                   # the lanes past K: skipped below
    wp = np.pad(w, ((0, 0), (0, pad))).reshape(M, nsteps, LANES, 2, 2)
    xp = np.pad(x, ((0, 0), (0, pad))).reshape(N, nsteps, LANES, 2, 2)
    live = (np.arange(nsteps)[:, None] * STEP + np.arange(LANES)[None, :] * 4) < K      # [step, lane]
    c = np.zeros((N, M, LANES, 2), np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for s in range(nsteps):
            for j in range(2):
                f = fma32(wp[None, :, s, :, j, :], xp[:, None, s, :, j, :], c)
                c = np.where(live[s][None, None, :, None], f, c)
        t = (c[..., 0] + c[..., 1]).astype(np.float32)
        return _tree(t)


def gemm_ksplit(K, S):
    """the split a request of S runs as: the largest S' <= S of 4, 2, 1 with whole 32-element chunks per slice"""
    assert S in (1, 2, 4)
    while S > 1 and K % (32 * S):
        S //= 2
    return S


def gemm_schedule(w, x, S):
    """f32 [N, M]: k_gemm_f32w's result at K split S (as gemm_ksplit(K, S) runs it), bit for bit"""
    w, x = np.asarray(w, np.float32), np.asarray(x, np.float32)
    M, K = w.shape
    N = x.shape[0]
    assert K % 32 == 0 and x.shape[1] == K
    S = gemm_ksplit(K, S)
    ks = K // S
    acc = np.zeros((S, N, M), np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for e in range(ks):                                   # the S slices side by side, element e of each
            cols = np.arange(S) * ks + e
            acc = fma32(w[:, cols].T[:, None, :], x[:, cols].T[:, :, None], acc)
        y = acc[0]
        for s in range(1, S):
            y = (y + acc[s]).astype(np.float32)
    return y


def exact_terms(w, x):
    """(S64 f64 [N, M], S_abs f64 [N, M]): the float64 sum of the exact products and the sum of their magnitudes"""
    w64, x64 = np.asarray(w, np.float64), np.asarray(x, np.float64)
    return x64 @ w64.T, np.abs(x64) @ np.abs(w64).T


def bound(K, s_abs):
    """|y - S64| <= 1.01 K 2^-24 sum|w x|: the worst case of any order of K fp32 fmas (each of the at most K roundings
    is at most 2^-24 of a partial sum, itself at most (1 + K 2^-24) sum|w x|)"""
    return 1.01 * K * 2.0 ** -24 * s_abs


# The shapes of tests/test_gpu_f32w.py (GEMV_CASES) and tests/test_gpu_f32w_gemm.py (GEMM_CASES), shared with
# tests/test_f32w_ref.py.  GEMV: one ragged step (32), 256 + 32, two steps (512), five and a ragged 224 (1504, tiles
# 8 + 8 + 1 at N = 17), the 43 steps of the LLaMA-7B w2 (11008, where a launch takes 2 columns).
# (K, M, N, ldy - M, special)
GEMV_CASES = [(32, 130, 1, 0, False), (288, 17, 3, 0, False), (512, 64, 8, 3, False), (1504, 65, 17, 0, False),
              (11008, 65, 8, 0, False), (288, 33, 5, 0, True)]
# GEMM: one chunk and ragged M; a small one; ragged both ways over more than one tile each way; K = 4544 = 142 chunks
# (S = 4 has no whole chunks per slice: runs as 2); the 128 x 64 tile.  (K, M, N, ldy - M, special)
GEMM_CASES = [(32, 130, 40, 0, False), (128, 33, 9, 2, False), (1024, 200, 130, 0, False), (4544, 73, 33, 0, False),
              (2048, 96, 48, 0, False), (128, 33, 9, 0, True)]
CASES = GEMV_CASES + GEMM_CASES
_cache = {}


def case(i):
    """(w, x) of CASES[i], made once per process and read-only"""
    if i not in _cache:
        K, M, N, _, special = CASES[i]
        w, x = random_case(np.random.default_rng([0xF32, i]), M, K, N, special)
        for a in (w, x):
            a.setflags(write=False)
        _cache[i] = (w, x)
    return _cache[i]


_refs = {}


def ref(i, kind, S=1):
    """the restated y of CASES[i], computed once per process: kind 'gemv', 'exact' or 'gemm' (with S)"""
    key = (i, kind, S if kind == "gemm" else 0)
    if key not in _refs:
        w, x = case(i)
        y = gemv_schedule(w, x) if kind == "gemv" else mul_mat_f32(w, x) if kind == "exact" else gemm_schedule(w, x, S)
        y.setflags(write=False)
        _refs[key] = y
    return _refs[key]
