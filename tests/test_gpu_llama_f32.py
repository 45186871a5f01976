"""The reference's unmodified llama.cpp (built with -DGGML_USE_CUBLAS, linked against libggml_hip_cuda.so) loads
the tiny "all F32" GGJT v3 LLaMA (tests/ggjt_f32_model.py, ftype 0) with its own loader and evaluates the 40-token
prompt and three decode steps.  Fully offloaded, every layer matrix is an F32 device tensor: without the F32 row the
backend declines its mul_mat and ggml.c aborts on the device operand.  In exact mode the logits are bit-identical to
the golden logits of the reference's CPU-only build (tests/golden/gen_llama_f32_golden.py) at prompt and decode; the
fast kernels (the F32 GEMV at decode, the f32-MFMA GEMM at the prompt) differ from them by the order of the additions
alone; and with n_gpu_layers = 0 and the F32 switch on the prompt's mul_mats reach the device through the residency
cache."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

import ggjt_f32_model as GF
from conftest import ROOT
from hip_env import ggml_hip, gpu_available

GOLD = os.path.join(ROOT, "tests", "golden")
HIP_LIB = os.path.join(ROOT, "oracle", "_ref", "libllama_ref_hip.so")

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason="needs a HIP device and libggml_hip.so"),
              pytest.mark.skipif(not os.path.exists(HIP_LIB), reason="oracle/_ref/libllama_ref_hip.so not built")]

OPS = json.load(open(os.path.join(GOLD, "ggml_op_enum.json")))
N_EVALS = 2                                      # prompt evals of one run (the second is the one returned)


def op_stats(L):
    L.ggml_hip_debug_op_stats.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    n = OPS["GGML_OP_COUNT"]
    c = np.zeros(n, np.int64)
    ggml_hip.check(L.ggml_hip_debug_op_stats(c.ctypes.data, c.size, 1), "op stats")
    return c


def run_llama(tmp_path, exact, ngl=99, f32_w=0):
    sys.path.insert(0, GOLD)
    from gen_llama_golden import ref_logits
    L = ggml_hip.load()
    prev = L.ggml_hip_get_exact()
    prev_w = L.ggml_hip_debug_set_f32_w(f32_w)
    ggml_hip.check(L.ggml_hip_set_exact(1 if exact else 0), "set_exact")
    ggml_hip.check(L.ggml_hip_weight_cache_clear(), "cache clear")
    mp = str(tmp_path / "mf.ggjt")
    assert GF.write(mp) == json.load(open(os.path.join(GOLD, "llama_f32_tiny_manifest.json")))["model_sha256"]
    op_stats(L)
    try:
        got, dec = ref_logits(HIP_LIB, mp, n_evals=N_EVALS, n_gpu_layers=ngl, with_decode=True)
        ran = op_stats(L)
    finally:
        ggml_hip.check(L.ggml_hip_weight_cache_clear(), "cache clear")
        L.ggml_hip_set_exact(prev)
        L.ggml_hip_debug_set_f32_w(prev_w)
    return got, dec, ran, (np.load(os.path.join(GOLD, "llama_f32_tiny_logits.npy")),
                           np.load(os.path.join(GOLD, "llama_f32_tiny_decode_logits.npy")))


def assert_layer_mul_mats_on_device(ran):
    """7 F32 weight mul_mats per layer plus the lm_head per eval ran on the device; beside them at most the two f16
    attention mul_mats per layer (which launch fusion may fold into other launches)."""
    nl = GF.HP["n_layer"]
    evals = N_EVALS + len(GF.DECODE)
    mm = int(ran[OPS["GGML_OP_MUL_MAT"]])
    assert (7 * nl + 1) * evals <= mm <= (9 * nl + 1) * evals, mm


def test_f32_llama_full_offload_exact_mode_bitwise(tmp_path):
    got, dec, ran, (gold, dgold) = run_llama(tmp_path, exact=True)
    assert np.array_equal(got.view(np.uint32), gold.view(np.uint32))
    assert np.array_equal(dec.view(np.uint32), dgold.view(np.uint32))
    assert_layer_mul_mats_on_device(ran)
    for op in ("GGML_OP_RMS_NORM", "GGML_OP_ROPE", "GGML_OP_SOFT_MAX", "GGML_OP_SILU"):
        assert ran[OPS[op]] > 0, op                                          # the nodes between them too


def test_f32_llama_full_offload_fast_kernels(tmp_path):
    """the F16 test's own cap; only the order of the additions differs here, so the ratio is far below F16's"""
    got, dec, ran, (gold, dgold) = run_llama(tmp_path, exact=False)
    assert np.isfinite(got).all() and np.isfinite(dec).all()
    assert_layer_mul_mats_on_device(ran)
    scale = np.abs(gold).max()
    print("fast kernels: max |logit - gold| / max |gold|", float(np.abs(got - gold).max() / scale),
          float(np.abs(dec - dgold).max() / scale))
    assert np.abs(got - gold).max() / scale < 2e-2 and np.abs(dec - dgold).max() / scale < 2e-2


def test_f32_llama_host_weights_switch_on_exact_mode_bitwise(tmp_path):
    """n_gpu_layers 0, GGML_HIP_F32_W on: the weights stay host tensors; the prompt's mul_mats (N = 40) reach the device
    through the residency cache, the decode steps stay on ggml's CPU ops (matrices below GGML_HIP_DECODE_MIN_WEIGHTS)."""
    got, dec, ran, (gold, dgold) = run_llama(tmp_path, exact=True, ngl=0, f32_w=1)
    assert np.array_equal(got.view(np.uint32), gold.view(np.uint32))
    assert np.array_equal(dec.view(np.uint32), dgold.view(np.uint32))
    assert ran[OPS["GGML_OP_MUL_MAT"]] == (7 * GF.HP["n_layer"] + 1) * N_EVALS
