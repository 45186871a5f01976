"""The shapes of the F16-weight prefill GEMM's tests (csrc/f16_w_gemm.hip, algo 11 of ggml_hip_mul_mat_f16), shared by
tests/test_f16w_gemm_inputs.py (CPU: what the bound asks of these inputs) and tests/test_gpu_f16w_gemm.py.  Weights and
x come from f16w_ref.random_case with seeds of their own; the float64 sum of the exact products and the sum of their
magnitudes are computed once per process and shared read-only.

The bound: |y - S| <= 1e-5 * sum |W * fp16(x)| per output (tests/test_gpu_f16w.py's for algo 9).  special = True (fp16
subnormals, +-0, |x| to 6e4) only at K <= 1504: on those inputs at K = 11008 one sequential fp32 chain is at 8.7e-6 of
the sum of magnitudes, too close to the bound to tell a wrong kernel from a right one."""
import numpy as np

import f16w_ref as R

BOUND = 1e-5

# (K, M, N, special): smallest call; one ragged chunk; K no multiple of 64 and N = 9; subnormals; ragged rows and more
# than 128 columns; long K; the long-K layer shape
CASES = [(32, 1, 1, False), (32, 130, 40, False), (544, 130, 9, False), (1504, 65, 17, True),
         (4160, 70, 130, False), (11008, 65, 8, False), (11008, 33, 70, False)]
IDS = ["K%d_M%d_N%d%s" % (c[0], c[1], c[2], "_special" if c[3] else "") for c in CASES]
WIDE = 4                                                     # the N = 130 case of the slice tests

# One more shape per plan of the launcher, each named with the plan auto takes for it at 256 CUs (the MI355X, and what
# the rule assumes where no device is known; gemm_f16w_auto_plan: N <= 64 with fewer than 512 row tiles of 32: plan 1;
# else plan 3 where its 128 x 128 tiles are at least 192, else plan 2 where its 64 x 128 tiles x 2 slices are at least
# 256, else plan 1).  (K, M, N, plan)
BIG = (64, 16390, 300, 3)                                    # 129 x 3 = 387 tiles of 128 x 128, ragged both ways: a grid
                                                             # larger than the device
PLAN_CASES = [(96, 200, 64, 1),                              # N <= 64
              (96, 200, 65, 1),                              # 2 tiles of plan 3, 4 x 1 x 2 workgroups of plan 2: too few;
                                                             # two column tiles of plan 1
              (96, 8200, 129, 2),                            # 65 x 2 = 130 tiles of plan 3, 129 x 2 x 2 = 516 workgroups of plan 2
              (32, 16390, 9, 2),                             # N <= 64 but 513 row tiles of 32: 129 tiles of plan 3, 514 of plan 2
              (64, 8321, 300, 3),                            # 66 x 3 = 198 tiles of 128 x 128
              BIG]

_cache = {}


def rng_for(*key):
    return np.random.default_rng([0xF16B, *key])


def inputs(K, M, N, special=False, key=0):
    """(w16, x) of a shape, computed once per process, read-only"""
    k = ("in", K, M, N, special, key)
    if k not in _cache:
        w16, x = R.random_case(rng_for(K, M, N, key), M, K, N, special)
        w16.setflags(write=False)
        x.setflags(write=False)
        _cache[k] = (w16, x)
    return _cache[k]


def terms(K, M, N, special=False, key=0):
    """(S f64 [N, M], sum of magnitudes f64 [N, M]) of inputs(...), computed once per process, read-only"""
    k = ("ref", K, M, N, special, key)
    if k not in _cache:
        ref, sab = R.exact_terms(*inputs(K, M, N, special, key))
        ref.setflags(write=False)
        sab.setflags(write=False)
        _cache[k] = (ref, sab)
    return _cache[k]


# The special inputs put one sequential fp32 chain at 2.4e-6 .. 3.8e-6 of the sum of magnitudes depending on where the
# seed places the large |x| (eight seeds tried on the CPU); the seed used is one where the chain stays within a quarter
# of the bound, the condition tests/test_f16w_gemm_inputs.py pins for every case.
SPECIAL_KEY = 4


def case(i):
    """(w16, x, S, sum of magnitudes) of CASES[i]"""
    K, M, N, special = CASES[i]
    key = SPECIAL_KEY if special else 0
    return inputs(K, M, N, special, key) + terms(K, M, N, special, key)


def within_bound(y, ref, sab):
    """(ok, the largest error as a share of the sum of magnitudes)"""
    err = np.abs(np.asarray(y, np.float64) - ref)
    return bool((err <= BOUND * sab + 1e-30).all()), float((err / (sab + 1e-30)).max())
