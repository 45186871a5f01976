"""The reference's unmodified llama.cpp (built with -DGGML_USE_CUBLAS, linked against libggml_hip_cuda.so) loads
the tiny "mostly F16" GGJT v3 LLaMA (tests/ggjt_f16_model.py) with its own loader and evaluates the 40-token prompt
and three decode steps.  Fully offloaded in exact mode the logits are bit-identical to the golden logits of the
reference's CPU-only build (tests/golden/gen_llama_f16_golden.py) at prompt and decode; the fast kernels (the F16 GEMV
at decode, the MFMA kernel at the prompt) give finite logits close to them; and with n_gpu_layers = 0 the prompt's
F16 weight mul_mats reach the device through the residency cache."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

import ggjt_f16_model as GF
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


def run_llama(tmp_path, exact, ngl=99):
    sys.path.insert(0, GOLD)
    from gen_llama_golden import ref_logits
    L = ggml_hip.load()
    prev = L.ggml_hip_get_exact()
    ggml_hip.check(L.ggml_hip_set_exact(1 if exact else 0), "set_exact")
    ggml_hip.check(L.ggml_hip_weight_cache_clear(), "cache clear")
    mp = str(tmp_path / "mf.ggjt")
    assert GF.write(mp) == json.load(open(os.path.join(GOLD, "llama_f16_tiny_manifest.json")))["model_sha256"]
    op_stats(L)
    try:
        got, dec = ref_logits(HIP_LIB, mp, n_evals=N_EVALS, n_gpu_layers=ngl, with_decode=True)
        ran = op_stats(L)
    finally:
        ggml_hip.check(L.ggml_hip_weight_cache_clear(), "cache clear")
        L.ggml_hip_set_exact(prev)
    return got, dec, ran, (np.load(os.path.join(GOLD, "llama_f16_tiny_logits.npy")),
                           np.load(os.path.join(GOLD, "llama_f16_tiny_decode_logits.npy")))


def assert_layer_mul_mats_on_device(ran):
    """7 F16 weight mul_mats per layer plus the lm_head per eval ran on the device; beside them at most the two f16
    attention mul_mats per layer (which launch fusion may fold into other launches)."""
    nl = GF.HP["n_layer"]
    evals = N_EVALS + len(GF.DECODE)
    mm = int(ran[OPS["GGML_OP_MUL_MAT"]])
    assert (7 * nl + 1) * evals <= mm <= (9 * nl + 1) * evals, mm


def test_f16_llama_full_offload_exact_mode_bitwise(tmp_path):
    got, dec, ran, (gold, dgold) = run_llama(tmp_path, exact=True)
    assert np.array_equal(got.view(np.uint32), gold.view(np.uint32))
    assert np.array_equal(dec.view(np.uint32), dgold.view(np.uint32))
    assert_layer_mul_mats_on_device(ran)
    for op in ("GGML_OP_RMS_NORM", "GGML_OP_ROPE", "GGML_OP_SOFT_MAX", "GGML_OP_SILU"):
        assert ran[OPS[op]] > 0, op                                          # the nodes between them too


def test_f16_llama_full_offload_fast_kernels(tmp_path):
    got, dec, ran, (gold, dgold) = run_llama(tmp_path, exact=False)
    assert np.isfinite(got).all() and np.isfinite(dec).all()
    assert_layer_mul_mats_on_device(ran)
    scale = np.abs(gold).max()
    print("fast kernels: max |logit - gold| / max |gold|", float(np.abs(got - gold).max() / scale),
          float(np.abs(dec - dgold).max() / scale))
    assert np.abs(got - gold).max() / scale < 2e-2 and np.abs(dec - dgold).max() / scale < 2e-2


def test_f16_llama_host_weights_exact_mode_bitwise(tmp_path):
    """n_gpu_layers 0: the weights stay host tensors; the prompt's mul_mats (N = 40) reach the device through the
    residency cache, the decode steps stay on ggml's CPU ops (matrices below GGML_HIP_DECODE_MIN_WEIGHTS)."""
    got, dec, ran, (gold, dgold) = run_llama(tmp_path, exact=True, ngl=0)
    assert np.array_equal(got.view(np.uint32), gold.view(np.uint32))
    assert np.array_equal(dec.view(np.uint32), dgold.view(np.uint32))
    assert ran[OPS["GGML_OP_MUL_MAT"]] == (7 * GF.HP["n_layer"] + 1) * N_EVALS
