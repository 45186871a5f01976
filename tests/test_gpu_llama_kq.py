"""The reference's unmodified llama.cpp with k-quants on (-DGGML_USE_K_QUANTS -DGGML_USE_CUBLAS, linked against
libggml_hip_cuda.so: oracle/_ref/libllama_ref_kq_hip.so) loads the tiny k-quants GGJT v3 LLaMAs of
tests/ggjt_kq_model.py with its own loader: the ten file types its quantizer writes at QK_K = 256, two to three weight
types inside one layer, a Q6_K output.weight behind every one of them (the q4_0 file included).  The golden logits are
those of the reference's CPU build with k-quants (tests/golden/gen_llama_kq_golden.py).

 a. full offload, exact mode, the Q4_K switch on: prompt and decode logits bitwise the golden, every weight mul_mat on
    the device;
 b. the Q4_K switch in its default position (off), the four files that hold Q4_K, n_gpu_layers 0, 1 and 99: bitwise
    the golden.  In an offloaded layer a Q4_K matrix stays on the backend's host copy while its src1 and dst are device
    tensors: the node is served from the host copy (hook_weight_type), since ggml.c's CPU mul_mat asserts host operands;
 c. host weights (n_gpu_layers 0), exact mode, the other files: bitwise the golden through the residency cache;
 d. the fast kernels at full offload: finite, on the device, within 2e-2 of the golden's largest logit;
 e. the k-quant prefill GEMMs forced on against forced off at N = 40, fast mode: prompt logits bitwise equal, and the
    two settings do select different algos for every (type, K, M) of the file;
 f. another batch size (12-token prompt, 8 decode steps) live against the CPU build: bitwise;
 g. launch fusion on / off and the launch modes 1, 2, 3 against eager around k-quant nodes: bitwise."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

import ggjt_kq_model as GK
from conftest import ROOT
from hip_env import ggml_hip, gpu_available

GOLD = os.path.join(ROOT, "tests", "golden")
HIP_LIB = os.path.join(ROOT, "oracle", "_ref", "libllama_ref_kq_hip.so")
CPU_LIB = os.path.join(ROOT, "oracle", "_ref", "libllama_ref_kq_cpu.so")

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason="needs a HIP device and libggml_hip.so"),
              pytest.mark.skipif(not os.path.exists(HIP_LIB), reason="oracle/_ref/libllama_ref_kq_hip.so not built")]

OPS = json.load(open(os.path.join(GOLD, "ggml_op_enum.json")))
MAN = json.load(open(os.path.join(GOLD, "llama_kq_tiny_manifest.json")))
N_EVALS = 2                                      # prompt evals of one run (the second is the one returned)
N_LAYER = GK.HP4["n_layer"]
N_FUSED = 15                                     # ggml-hip.h, ggml_hip_debug_op_stats: fused launches in the last slots
NEVER = 2 ** 31 - 1                              # a GEMM threshold no N reaches (ggml-hip.h: INT_MAX)
N_PROMPT = len(GK.PROMPT)

HAS_Q4_K = ("q2_k", "q3_k_m", "q4_k_s", "q4_k_m")
NO_Q4_K = tuple(v for v in GK.VARIANTS if v not in HAS_Q4_K)


def n_q4_K(v):
    """the weight mul_mats of one eval whose src0 is Q4_K (tok_embeddings is read by get_rows, not by a mul_mat)"""
    return sum(1 for n, t in GK.type_map(v).items() if t == GK.Q4_K and n != "tok_embeddings.weight")


def op_stats(L, fused=False):
    L.ggml_hip_debug_op_stats.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    n = OPS["GGML_OP_COUNT"]
    c = np.zeros(2 * n + 1 + N_FUSED, np.int64)
    ggml_hip.check(L.ggml_hip_debug_op_stats(c.ctypes.data, c.size, 1), "op stats")
    return (c[:n], c[2 * n + 1:]) if fused else c[:n]


def gold_of(v):
    return (np.load(os.path.join(GOLD, f"llama_kq_{v}_tiny_logits.npy")),
            np.load(os.path.join(GOLD, f"llama_kq_{v}_tiny_decode_logits.npy")))


def write_model(tmp_path, v):
    mp = str(tmp_path / f"m-{v}.ggjt")
    assert GK.write(mp, v) == MAN["models"][v]["model_sha256"]
    return mp


def run_llama(tmp_path, v, exact, ngl=99, q4k=1, with_decode=True):
    """(prompt logits, decode logits, op counts) of one run; every switch is put back and the weight cache cleared"""
    sys.path.insert(0, GOLD)
    from gen_llama_golden import ref_logits
    L = ggml_hip.load()
    mp = write_model(tmp_path, v)
    prev = L.ggml_hip_get_exact()
    prev_q4k = L.ggml_hip_debug_set_q4_K(q4k)
    try:
        ggml_hip.check(L.ggml_hip_set_exact(1 if exact else 0), "set_exact")
        ggml_hip.check(L.ggml_hip_weight_cache_clear(), "cache clear")
        op_stats(L)
        r = ref_logits(HIP_LIB, mp, n_evals=N_EVALS, n_gpu_layers=ngl, with_decode=with_decode)
        ran = op_stats(L)
    finally:
        ggml_hip.check(L.ggml_hip_weight_cache_clear(), "cache clear")
        L.ggml_hip_set_exact(prev)
        L.ggml_hip_debug_set_q4_K(prev_q4k)
    got, dec = r if with_decode else (r, None)
    return got, dec, ran


def assert_layer_mul_mats_on_device(ran):
    """7 weight mul_mats per layer plus the lm_head per eval ran on the device; beside them at most the two f16
    attention mul_mats per layer (which launch fusion may fold into other launches)."""
    evals = N_EVALS + len(GK.DECODE)
    mm = int(ran[OPS["GGML_OP_MUL_MAT"]])
    assert (7 * N_LAYER + 1) * evals <= mm <= (9 * N_LAYER + 1) * evals, mm


def bits(a):
    return a.view(np.uint32)


# ---- a ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("v", GK.VARIANTS)
def test_full_offload_exact_mode_bitwise(tmp_path, v):
    got, dec, ran = run_llama(tmp_path, v, exact=True)
    gold, dgold = gold_of(v)
    assert np.array_equal(bits(got), bits(gold))
    assert np.array_equal(bits(dec), bits(dgold))
    assert_layer_mul_mats_on_device(ran)
    for op in ("GGML_OP_RMS_NORM", "GGML_OP_ROPE", "GGML_OP_SOFT_MAX", "GGML_OP_SILU"):
        assert ran[OPS[op]] > 0, op                                          # the nodes between them too


# ---- b ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ngl", [0, 1, 99])
@pytest.mark.parametrize("v", HAS_Q4_K)
def test_q4_K_switch_default_exact_mode_bitwise(tmp_path, v, ngl):
    """The files that hold Q4_K with the switch off, as a process that never touched it runs them.  n_gpu_layers 0:
    the Q4_K mul_mats stay on ggml's CPU op, every other prompt mul_mat reaches the device through the residency
    cache and the decode steps stay on the CPU (matrices below GGML_HIP_DECODE_MIN_WEIGHTS).  n_gpu_layers >= 1: the
    Q4_K matrices of an offloaded layer are CPU tensors between device operands and are served from the host copy."""
    assert n_q4_K(v) == {"q2_k": 6, "q3_k_m": 6, "q4_k_s": 14, "q4_k_m": 12}[v]
    got, dec, ran = run_llama(tmp_path, v, exact=True, ngl=ngl, q4k=0)
    gold, dgold = gold_of(v)
    assert np.array_equal(bits(got), bits(gold))
    assert np.array_equal(bits(dec), bits(dgold))
    if ngl == 0:
        assert ran[OPS["GGML_OP_MUL_MAT"]] == (7 * N_LAYER + 1 - n_q4_K(v)) * N_EVALS
    elif ngl == 99:
        assert_layer_mul_mats_on_device(ran)       # nothing can fall back to the CPU between device operands


# ---- c ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("v", NO_Q4_K)
def test_host_weights_exact_mode_bitwise(tmp_path, v):
    """n_gpu_layers 0: the weights stay host tensors; the prompt's mul_mats (N = 40) reach the device through the
    residency cache, the decode steps stay on ggml's CPU ops (matrices below GGML_HIP_DECODE_MIN_WEIGHTS)."""
    got, dec, ran = run_llama(tmp_path, v, exact=True, ngl=0, q4k=0)
    gold, dgold = gold_of(v)
    assert np.array_equal(bits(got), bits(gold))
    assert np.array_equal(bits(dec), bits(dgold))
    assert ran[OPS["GGML_OP_MUL_MAT"]] == (7 * N_LAYER + 1) * N_EVALS


# ---- d ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("v", GK.VARIANTS)
def test_full_offload_fast_kernels(tmp_path, v):
    """The bound is the one tests/test_gpu_llama_q5x.py uses.  Measured on an MI355X, max |delta| / max |gold|, prompt /
    decode: q4_0_q6k 7.1e-3 / 8.2e-3, q2_k 1.6e-7 / 1.6e-7, q3_k_s 1.8e-7 / 4.5e-8, q3_k_m 2.4e-7 / 8.1e-4, q3_k_l
    5.7e-3 / 1.3e-7, q4_k_s 1.1e-3 / 1.5e-7, q4_k_m 1.9e-7 / 6.5e-8, q5_k_s 1.99e-2 / 4.4e-3, q5_k_m 1.3e-2 / 4.1e-5,
    q6_k 1.4e-2 / 9.4e-3.  Per matrix the fast kernels are within 4e-8 of the exact ones (relative to |W| . |x|); a
    prompt row is either within 2e-7 of the golden or, from the first token at which a q8_K rounding of an activation
    falls the other way, about 5e-3 off, and so is every later row that attends to that token's K and V."""
    got, dec, ran = run_llama(tmp_path, v, exact=False)
    gold, dgold = gold_of(v)
    assert np.isfinite(got).all() and np.isfinite(dec).all()
    assert_layer_mul_mats_on_device(ran)
    scale = np.abs(gold).max()
    ep, ed = np.abs(got - gold).max() / scale, np.abs(dec - dgold).max() / scale
    print(f"fast-mode distance {v}: prompt {ep:.3e} decode {ed:.3e} (max |gold| {scale:.4f})")
    assert ep < 2e-2 and ed < 2e-2


# ---- e ------------------------------------------------------------------------------------------------------------

def auto_algo(L, typ, K, M, N):
    if typ == GK.Q6_K:
        return L.ggml_hip_debug_q6k_auto_algo(K, M, N)
    if typ in (GK.Q4_K, GK.Q5_K):
        return L.ggml_hip_debug_q45k_auto_algo(typ, K, M, N)
    assert typ in (GK.Q2_K, GK.Q3_K), typ
    return L.ggml_hip_debug_q23k_auto_algo(typ, K, M, N)


GEMM_ALGO = {GK.Q6_K: 5, GK.Q5_K: 6, GK.Q4_K: 6, GK.Q3_K: 8, GK.Q2_K: 8}      # ggml-hip.h


@pytest.mark.parametrize("v", ["q3_k_l", "q2_k", "q5_k_m", "q6_k"])
def test_prefill_gemms_change_no_bit(tmp_path, v):
    """Fast mode, full offload, the 40-token prompt: every k-quant GEMM forced off (the GEMVs' column tiles) against
    every one forced on from N = 9.  The logits are bitwise equal, and for every (type, K, M) of the file the two
    settings select different algos at N = 40, so the comparison is of two different kernels."""
    sys.path.insert(0, GOLD)
    L = ggml_hip.load()
    shapes = sorted({(t, ne[0], ne[1]) for n, t, ne, _ in GK.tensors(v) if len(ne) == 2 and n != "tok_embeddings.weight"})
    assert {t for t, _, _ in shapes} == set(GK.type_map(v).values()) and len(shapes) >= 3
    setters = (L.ggml_hip_debug_set_q6k_gemm_min_n, L.ggml_hip_debug_set_q45k_gemm_min_n,
               L.ggml_hip_debug_set_q23k_gemm_min_n)
    out, algos = {}, {}
    prev_exact = L.ggml_hip_get_exact()
    try:
        for name, min_n in (("off", NEVER), ("on", 9)):
            for s in setters:
                s(min_n)
            ggml_hip.check(L.ggml_hip_set_exact(0), "set_exact")
            algos[name] = [auto_algo(L, t, K, M, N_PROMPT) for t, K, M in shapes]
            out[name] = run_llama(tmp_path, v, exact=False, with_decode=False)
    finally:
        for s in setters:
            s(-1)
        L.ggml_hip_set_exact(prev_exact)
    assert algos["off"] == [1] * len(shapes), (shapes, algos)
    assert algos["on"] == [GEMM_ALGO[t] for t, _, _ in shapes], (shapes, algos)
    assert np.isfinite(out["on"][0]).all()
    assert np.array_equal(bits(out["on"][0]), bits(out["off"][0]))
    assert np.array_equal(out["on"][2], out["off"][2])                       # the same nodes counted


# ---- f, g: refllama_bench ---------------------------------------------------------------------------------------

def bench_logits(lib_path, mp, n_prompt, n_decode, ngl):
    lib = ctypes.CDLL(lib_path)
    lib.refllama_bench.restype = ctypes.c_int
    lib.refllama_bench.argtypes = [ctypes.c_char_p] + [ctypes.c_int] * 6 + [ctypes.c_void_p, ctypes.c_void_p]
    nv = GK.HP4["n_vocab"]
    res = np.zeros(3, np.float64)
    lg = np.zeros(nv, np.float32)
    assert lib.refllama_bench(mp.encode(), n_prompt, n_decode, 1, ngl, 1024, 1, res.ctypes.data, lg.ctypes.data) == nv
    return lg


@pytest.mark.skipif(not os.path.exists(CPU_LIB), reason="oracle/_ref/libllama_ref_kq_cpu.so not built")
@pytest.mark.parametrize("v", ["q3_k_m", "q5_k_m"])
def test_batch_of_12_exact_bitwise_vs_cpu_build(tmp_path, v):
    """A 12-token prompt (between 9 and 31: the Q6_K GEMM from N = 9 in fast mode, the exact kernels' and the GEMVs'
    column tiles of 8 + 4 otherwise) and 8 decode steps at full offload in exact mode, against the reference's CPU
    build with k-quants run live: the final logits are bitwise equal."""
    L = ggml_hip.load()
    mp = write_model(tmp_path, v)
    prev = L.ggml_hip_get_exact()
    prev_q4k = L.ggml_hip_debug_set_q4_K(1)
    try:
        ggml_hip.check(L.ggml_hip_set_exact(1), "set_exact")
        ggml_hip.check(L.ggml_hip_weight_cache_clear(), "cache clear")
        op_stats(L)
        got = bench_logits(HIP_LIB, mp, 12, 8, 99)
        ran = op_stats(L)
    finally:
        ggml_hip.check(L.ggml_hip_weight_cache_clear(), "cache clear")
        L.ggml_hip_set_exact(prev)
        L.ggml_hip_debug_set_q4_K(prev_q4k)
    ref = bench_logits(CPU_LIB, mp, 12, 8, 0)
    assert np.isfinite(ref).all()
    assert np.array_equal(bits(got), bits(ref))
    assert ran[OPS["GGML_OP_MUL_MAT"]] >= (7 * N_LAYER + 1) * 9


@pytest.mark.parametrize("exact", [0, 1], ids=["fast", "exact"])
@pytest.mark.parametrize("v", ["q4_0_q6k", "q3_k_l"])
def test_fusion_and_launch_modes_bitwise(tmp_path, v, exact):
    """24-token prompt and 30 decode steps at full offload: the k-quant nodes (the Q6_K lm_head behind q4_0 layers;
    Q3_K and Q5_K matrices with the Q6_K lm_head) between the hook scheduler's held q4_0 sibling groups and fused
    chains, under the launch recorder (1 HIP graphs, 2 launcher thread) and the own-AQL-queue mode (3).  Fusion off
    and every launch mode give the logits of fused eager launches bit for bit; in the q4_0 file the sibling groups
    and the soft_max -> KQV launches still fire with the Q6_K lm_head in the graph."""
    n_prompt, n_decode = 24, 30
    L = ggml_hip.load()
    mp = write_model(tmp_path, v)
    L.ggml_hip_debug_set_fuse.argtypes = [ctypes.c_int]
    L.ggml_hip_debug_set_graph.argtypes = [ctypes.c_int]
    prev = L.ggml_hip_get_exact()
    prev_q4k = L.ggml_hip_debug_set_q4_K(1)
    out = {}
    try:
        ggml_hip.check(L.ggml_hip_set_exact(exact), "set_exact")
        for fuse, mode in ((1, 0), (0, 0), (1, 1), (1, 2), (1, 3)):
            ggml_hip.check(L.ggml_hip_debug_set_fuse(fuse), "set_fuse")
            ggml_hip.check(L.ggml_hip_debug_set_graph(mode), "set_graph")
            ggml_hip.check(L.ggml_hip_weight_cache_clear(), "cache clear")
            op_stats(L)
            lg = bench_logits(HIP_LIB, mp, n_prompt, n_decode, 99)
            out[(fuse, mode)] = (lg,) + op_stats(L, fused=True)
    finally:
        L.ggml_hip_debug_set_graph(0)
        L.ggml_hip_debug_set_fuse(1)
        ggml_hip.check(L.ggml_hip_weight_cache_clear(), "cache clear")
        L.ggml_hip_set_exact(prev)
        L.ggml_hip_debug_set_q4_K(prev_q4k)
    base, ran, fused = out[(1, 0)]
    assert np.isfinite(base).all()
    for key, (lg, _, _) in out.items():
        assert np.array_equal(bits(lg), bits(base)), key
    assert ran[OPS["GGML_OP_MUL_MAT"]] >= (7 * N_LAYER + 1) * (n_decode + 1)
    assert (out[(0, 0)][2] == 0).all(), out[(0, 0)][2]                       # fusion off: nothing fused
    assert fused[8] >= n_decode * N_LAYER, fused                             # soft_max -> KQV, any weight type
    if v == "q4_0_q6k":
        print("fused launches", v, "exact" if exact else "fast", fused.tolist())
        assert fused[6] >= 2 * n_decode * N_LAYER, fused                     # wq|wk|wv and w1|w3 as sibling groups
        evals = n_decode + 1
        assert fused[0] >= evals * N_LAYER, fused                            # [add ->] rms_norm -> mul chains
        # silu -> mul of every layer and eval: its own launch (2), the w2 GEMV's prologue (10) or the w1|w3 GEMV's
        # epilogue (13, the fast kernels at decode)
        assert fused[2] + fused[10] + fused[13] >= evals * N_LAYER, fused
