"""The q4_0 fast path pinned to its exact block sums, with no relative slack.

Every path gets two checks (tests/q4_0_exact_cases.py, tests/parity.py):
 (a) order-free inputs, on which every legal order of the fp32 arithmetic gives the same bits: y must EQUAL
     float32(y64) (as values; -0.0 == +0.0).  This also pins the q8_0 bytes of the quantizer fused into the path
     (the GEMV prologue, quantize_q8_0_soa, gemm8_prep_x, gemm9_prep_x), which are otherwise seen only through y:
     a wrong d or a q off by one LSB changes an exact y;
 (b) gaussian make_case inputs, and the same with a per-block scale spread (as test_q8_0_bitexact_random_scales),
     within check_y_terms of y64 = block_terms on the oracle's q8_0 bytes: |y - y64| <= 1.01 (nb + 2) 2^-24 S_abs.

roundings = 2 everywhere, read from the kernels: each one forms the block sum as an integer (k_gemv_q4_0 and
k_engine_q4_0: v_dot4 on the unsigned nibbles, then `- 8 * sum(q)` still in int32, q4_0_gemv.hip `sA = dot_q4_q8(..)
- sx.x`; k_gemm7 / k_gemm8 / split-K: the i8 MFMA on nibble - 8; k_gemm9 / k_gemm9w: the fp6 MFMA, whose f32 result is
that integer), forms d_x * d_w exactly (fp16 x fp16 in fp32, or the rank-1 fp16 MFMA), and accumulates with ONE fmaf
per block (`acc = fmaf(S, P, acc)`): one rounding per term and addition.  After the chain the partial sums meet in a
6-step wave reduction (GEMV, engine), in chunk order (BAL), in SK steps (split-K) or in one step (the workgroup
halves of k_gemm8 / k_gemm9): never more than nb - 1 additions on a term's path that can round (an addition of 0.0 is
exact).  No kernel keeps the nibble dot and the -8 sum(q) correction as separate floats, so S_abs stands as it is.

The q4_0 fast-mode kernels of csrc/q4_0_{gemv,gemm,engine}.hip, and where each is pinned:

  k_gemv_q4_0<NT 1, PPL 1..3> (row items, N = 1)  TestGemv (K = 64, 256, 1024: one pair per lane, VAR 15; K = 4544: two;
                                                  K = 11008: three, VAR 3)
  k_gemv_q4_0<NT 3 / 8, PPL 0> (chunk items)      TestGemv at N = 3, 8 (K = 4544: two chunks per row, ring depth 2)
  k_gemv_q4_0<PPL 0, BAL 0 / 1> (K > 12288)       TestGemvBalance, both settings (different summation orders)
  k_gemv_q4_0, the other launch policies (VAR,    bitwise the automatic policy's: test_gpu_parity.py::test_gemv_launch_
    ring depth, row maps, workgroups per CU,      policies_bitwise_identical (incl. (64, 37, 3), which is TestGemv's)
    row items off)
  k_gemv_q4_0<NT 2, 4..7>                         TestGemv (256, 129, N): no test links the token-count instantiations
                                                  to one another, so each is run here once
  k_gemv_q4_0 sibling launches (GemvMats n > 1)   test_gpu_parity.py::test_multi_matrix_siblings_match_single_calls,
                                                  test_gemv_balanced_chunks (siblings == single calls, bitwise)
  k_gemv_q4_0<PRO 1 / 2> (norm / silu prologue)   test_gpu_gemv_prologue.py::test_prologue (y bitwise the plain GEMV's
                                                  on the chain's output)
  k_gemv_q4_0<EPI 1 / 2> (rope / copy / glu)      test_gpu_gemv_epi.py::test_rope_cache_epilogue_bitwise,
                                                  test_glu_epilogue_bitwise (the mul_mat's y bitwise the plain GEMV's)
  k_gemm_sk_q4_0<16> + quantize_q8_0_soa          TestSplitK, the shapes below two rounds of 32 x 32 tiles
  k_gemm_sk_q4_0<8>                               TestSplitK (1088, 4100, 128): 516 tiles; no test links it bitwise to
                                                  the 16-wave form (their slices differ), so it is run here
  k_gemm7_q4_0 + quantize_q8_0_soa (fp16 d copy)  TestGemm[gemm7]
  k_prep8_x / k_prep8_w / k_gemm8_q4_0            TestGemm[gemm8] (per-call image), TestRegisteredImages[int8]
  k_prep9_x / k_prep9_w / k_gemm9_q4_0<true>      TestGemm[gemm9] (launches of at most half the CUs' tiles run as half
                                                  tiles), TestRegisteredImages[fp6], the fp6 extreme twin in
                                                  test_gpu_parity.py
  k_gemm9_q4_0<false> (whole 128 x 64 tiles)      bitwise k_gemm9_q4_0<true>: test_gpu_parity.py::test_gemm9_sibling_
                                                  group_one_launch_bitwise[tile128x64] (a 152-tile sibling launch of
                                                  whole tiles == the single calls, which run as half tiles); and
                                                  == k_gemm8: test_gemm9_fp6_bitwise_equals_gemm8_int8
  k_gemm9w_q4_0 (128 x 128 tile)                  TestGemm[gemm9w]
  x-image producers (ops / epilogues that write   test_gpu_x9.py, test_gpu_prefill_chain.py (image bitwise
    k_gemm9's x image), g9_ximage_out             gemm9_prep_x's of the same floats; chain y bitwise per-launch)
  k_engine_q4_0                                   TestChain[engine]; == per-launch: test_gpu_chain.py::test_engine_
                                                  ragged_linear_chain_bitwise and the other test_engine_* there
  decode chains per launch (k_gemv_q4_0)          TestChain[per-launch]

The worst multiple of 2^-24 S_abs each path needed is printed by the module's last test (a record, not a threshold).
"""
import ctypes

import numpy as np
import pytest

import oracle as O
import q4_0_exact_cases as C
from hip_env import ggml_hip, gpu_available
from parity import QK, assert_equal_values, block_terms, check_y_terms

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason="needs a HIP device and libggml_hip.so")]

DB = ggml_hip.DeviceBuffer
NEEDS = {}          # path -> worst multiple of 2^-24 * S_abs over the gaussian cases


def _set(name, v):
    L = ggml_hip.load()
    fn = getattr(L, name)
    fn.argtypes = [ctypes.c_int]
    ggml_hip.check(fn(v), name)


def mul_mat(wq, K, x, algo):
    """y [N, M] of one ggml_hip_mul_mat_q4_0_ex call; y is pre-filled with a NaN pattern."""
    x = np.ascontiguousarray(x, np.float32)
    N, M = x.shape[0], wq.shape[0]
    wd, xd = DB.from_array(np.ascontiguousarray(wq)), DB.from_array(x)
    yd = DB(N * M * 4)
    ggml_hip.load().ggml_hip_memset(yd.ptr, 0xFF, yd.nbytes, None)
    ggml_hip.mul_mat(wd, K, M, xd, N, yd, algo=algo)
    return yd.download((N, M), np.float32)


class Path:
    """One way through the fast path: the algo and the debug switches around the call (restored in a finally)."""

    def __init__(self, name, algo, switches=()):
        self.name, self.algo, self.switches = name, algo, switches

    def run(self, wq, K, x):
        done = []
        try:
            for sw, v in self.switches:
                done.append(sw)
                _set(sw, v)
            return mul_mat(wq, K, x, self.algo)
        finally:
            for sw in reversed(done):
                _set(sw, -1)

    def __repr__(self):
        return self.name


def check_order_free(path, K, M, N):
    c = C.order_free(K, M, N)
    assert_equal_values(path.run(c["wq"], K, c["x"]), c["y64"])


def check_gaussian(path, K, M, N, spread):
    c = C.gaussian(O, K, M, N, spread=spread)
    need = check_y_terms(path.run(c["wq"], K, c["x"]), c["y64"], c["s_abs"], K // QK)
    NEEDS[path.name] = max(NEEDS.get(path.name, 0.0), need)
    print(f"{path.name} K={K} M={M} N={N} {'spread' if spread else 'gauss'}: needs {need:.2f} * 2^-24 S_abs "
          f"(bound {1.01 * (K // QK + 2):.1f})")


KINDS = pytest.mark.parametrize("spread", [False, True], ids=["gauss", "spread"])
GEMV = Path("gemv", 1)
BAL = [Path("gemv-chunks-balanced", 1, (("ggml_hip_debug_set_gemv_bal", 1),)),
       Path("gemv-chunks-by-row", 1, (("ggml_hip_debug_set_gemv_bal", 0),))]
SPLITK = Path("split-k", 3)
GEMMS = [Path("gemm7-bytes-in-place", 2, (("ggml_hip_debug_set_gemm_version", 7),)),
         Path("gemm8-per-call-image", 2, (("ggml_hip_debug_set_gemm_version", 9),)),
         Path("gemm9-per-call-image", 2, (("ggml_hip_debug_set_gemm_version", 11), ("ggml_hip_debug_set_gemm9_wide", 0))),
         Path("gemm9w-per-call-image", 2, (("ggml_hip_debug_set_gemm_version", 11), ("ggml_hip_debug_set_gemm9_wide", 1)))]


def _ids(v):
    return repr(v) if isinstance(v, Path) else None


class TestGemv:
    """algo 1, the quantizer fused into the prologue: K = 64 (one pair per row, 63 idle lanes), ragged M, more
    than one workgroup (M = 333), rows only 4-byte aligned (K = 4544, 2,556-byte rows), N = 1 (row items), 3, 8."""

    @pytest.mark.parametrize("K,M,N", C.GEMV_SHAPES)
    def test_order_free_equal(self, K, M, N):
        check_order_free(GEMV, K, M, N)

    @KINDS
    @pytest.mark.parametrize("K,M,N", C.GEMV_SHAPES)
    def test_gaussian_within_terms(self, K, M, N, spread):
        check_gaussian(GEMV, K, M, N, spread)


class TestGemvBalance:
    """K > 12288: chunk items, with the chunk balance forced on (per-chunk sums combined in chunk order) and off
    (a wave's chunks of a row in one chain): two summation orders, one exact answer."""

    @pytest.mark.parametrize("path", BAL, ids=_ids)
    @pytest.mark.parametrize("K,M,N", C.BAL_SHAPES)
    def test_order_free_equal(self, K, M, N, path):
        check_order_free(path, K, M, N)

    @KINDS
    @pytest.mark.parametrize("path", BAL, ids=_ids)
    @pytest.mark.parametrize("K,M,N", C.BAL_SHAPES)
    def test_gaussian_within_terms(self, K, M, N, path, spread):
        check_gaussian(path, K, M, N, spread)


class TestSplitK:
    """algo 3 (quantize_q8_0_soa + k_gemm_sk_q4_0): fewer blocks than K splits (K = 64: 14 of 16 waves idle),
    ragged 32 x 32 tiles in M and N, K = 4544 (71 pairs over 16 waves: a short last slice), N = 128."""

    @pytest.mark.parametrize("K,M,N", C.SPLITK_SHAPES)
    def test_order_free_equal(self, K, M, N):
        check_order_free(SPLITK, K, M, N)

    @KINDS
    @pytest.mark.parametrize("K,M,N", C.SPLITK_SHAPES)
    def test_gaussian_within_terms(self, K, M, N, spread):
        check_gaussian(SPLITK, K, M, N, spread)


class TestGemm:
    """algo 2 forced to k_gemm7 on the bytes in place (version 7), k_gemm8 and k_gemm9 on per-call images (9, 11;
    k_gemm9 in both tiles): K = 64 (one half stage), M = 1, ragged in both tile sizes, K = 4544 (a partial last
    stage: 142 blocks = 17 stages of 8 + 6, 35 of 4 + 2)."""

    @pytest.mark.parametrize("path", GEMMS, ids=_ids)
    @pytest.mark.parametrize("K,M,N", C.GEMM_SHAPES)
    def test_order_free_equal(self, K, M, N, path):
        check_order_free(path, K, M, N)

    @KINDS
    @pytest.mark.parametrize("path", GEMMS, ids=_ids)
    @pytest.mark.parametrize("K,M,N", C.GEMM_SHAPES)
    def test_gaussian_within_terms(self, K, M, N, path, spread):
        check_gaussian(path, K, M, N, spread)


class TestRegisteredImages:
    """ggml_hip_weight_image_create under version 8 (int8 image, k_gemm8) and 10 (fp6 image, k_gemm9): the image is
    built once by the same k_prep8_w / k_prep9_w, found by the weight's address and used by algo 2."""

    @staticmethod
    def run(v, wq, K, x):
        L = ggml_hip.load()
        x = np.ascontiguousarray(x, np.float32)
        N, M = x.shape[0], wq.shape[0]
        wd, xd = DB.from_array(np.ascontiguousarray(wq)), DB.from_array(x)
        yd = DB(N * M * 4)
        L.ggml_hip_memset(yd.ptr, 0xFF, yd.nbytes, None)
        before = L.ggml_hip_weight_image_bytes()
        made = False
        try:
            _set("ggml_hip_debug_set_gemm_version", v)
            ggml_hip.check(L.ggml_hip_weight_image_create(wd.ptr, K, M, None), "image")
            made = True
            assert L.ggml_hip_weight_image_bytes() > before
            ggml_hip.mul_mat(wd, K, M, xd, N, yd, algo=2)
            return yd.download((N, M), np.float32)
        finally:
            _set("ggml_hip_debug_set_gemm_version", -1)
            if made:
                assert L.ggml_hip_weight_image_free(wd.ptr) == 1

    @pytest.mark.parametrize("v", [8, 10], ids=["int8-image", "fp6-image"])
    @pytest.mark.parametrize("K,M,N", C.IMAGE_SHAPES)
    def test_order_free_equal(self, K, M, N, v):
        c = C.order_free(K, M, N)
        assert_equal_values(self.run(v, c["wq"], K, c["x"]), c["y64"])

    @KINDS
    @pytest.mark.parametrize("v", [8, 10], ids=["int8-image", "fp6-image"])
    @pytest.mark.parametrize("K,M,N", C.IMAGE_SHAPES)
    def test_gaussian_within_terms(self, K, M, N, v, spread):
        c = C.gaussian(O, K, M, N, spread=spread)
        name = f"registered-image-v{v}"
        need = check_y_terms(self.run(v, c["wq"], K, c["x"]), c["y64"], c["s_abs"], K // QK)
        NEEDS[name] = max(NEEDS.get(name, 0.0), need)
        print(f"{name} K={K} M={M} N={N} {'spread' if spread else 'gauss'}: needs {need:.2f} * 2^-24 S_abs")


class TestChain:
    """A two-task decode chain, per launch and through the persistent engine (k_engine_q4_0): task 0 gets order-free
    inputs and must be exact; task 1 reads task 0's y (its first K values, whatever they are) as x and is checked
    against block_terms on the oracle's q8_0 bytes of that y, siblings included."""

    @pytest.mark.parametrize("engine", [0, 1], ids=["per-launch", "engine"])
    def test_chain_exact_then_within_terms(self, engine):
        (K0, (M0,)), (K1, Ms1) = C.CHAIN_SPEC
        c = C.order_free(K0, M0, 1)
        w1 = [O.quantize_q4_0(O.gaussian(M * K1, 0xC4A1 + i, 0.0, 0.05).reshape(M, K1))[0] for i, M in enumerate(Ms1)]
        wd0 = DB.from_array(np.ascontiguousarray(c["wq"]))
        wd1 = [DB.from_array(w) for w in w1]
        xd0 = DB.from_array(np.ascontiguousarray(c["x"]))
        y0 = DB(M0 * 4)
        ys1 = [DB(M * 4) for M in Ms1]
        for b in [y0] + ys1:
            ggml_hip.load().ggml_hip_memset(b.ptr, 0xFF, b.nbytes, None)
        ch = ggml_hip.Chain([([wd0], [M0], K0, xd0, [y0]), (wd1, Ms1, K1, y0, ys1)], engine=engine)
        assert ch.engine_info()["on"] == engine, ggml_hip.load().ggml_hip_last_error()
        ch.launch()
        assert ch.status() == 0, ggml_hip.load().ggml_hip_last_error()
        got0 = y0.download((1, M0), np.float32)
        assert_equal_values(got0, c["y64"])
        xin = np.ascontiguousarray(got0[:, :K1])
        xq = O.quantize_q8_0(xin, "avx2")
        name = "chain-engine" if engine else "chain-per-launch"
        for w, M, yd in zip(w1, Ms1, ys1):
            y64, s_abs = block_terms(w, xq, K1)
            need = check_y_terms(yd.download((1, M), np.float32), y64, s_abs, K1 // QK)
            NEEDS[name] = max(NEEDS.get(name, 0.0), need)
            print(f"{name} task 1 M={M}: needs {need:.2f} * 2^-24 S_abs")


def test_worst_needs_report(capsys):
    """The last test of the module: prints the worst need per path recorded by the tests above (past the output
    capture, so a plain -q run shows it).  A record of what was measured against y64, not a threshold: every figure
    has already passed its bound in check_y_terms."""
    with capsys.disabled():
        print("\nq4_0 fast path, worst |y - y64| / (2^-24 S_abs) per path (bound: 1.01 (nb + 2)):")
        for path, need in sorted(NEEDS.items()):
            print(f"  {path:<28s} {need:6.2f}")
    assert all(np.isfinite(v) for v in NEEDS.values())
