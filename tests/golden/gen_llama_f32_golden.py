"""Golden logits of the tiny "all F32" GGJT v3 LLaMA (tests/ggjt_f32_model.py) from the REFERENCE's own
llama.cpp + ggml.c, CPU-only build (oracle/_ref/libllama_ref_cpu.so, oracle/Makefile `ref`): the 40-token prompt and
the three single-token decode steps of tests/ggjt_model.py.
Run here (needs the reference build): python tests/golden/gen_llama_f32_golden.py"""
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [HERE, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
import ggjt_f32_model as GF  # noqa: E402
from gen_llama_golden import ref_logits  # noqa: E402

if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as d:
        mp = os.path.join(d, "tiny-f32.ggjt")
        sha = GF.write(mp)
        logits, dlogits = ref_logits(os.path.join(ROOT, "oracle", "_ref", "libllama_ref_cpu.so"), mp,
                                     with_decode=True)
    assert np.isfinite(logits).all() and np.isfinite(dlogits).all()
    np.save(os.path.join(HERE, "llama_f32_tiny_logits.npy"), logits)
    np.save(os.path.join(HERE, "llama_f32_tiny_decode_logits.npy"), dlogits)
    json.dump({"model_sha256": sha, "prompt": GF.PROMPT, "decode": GF.DECODE, "hparams": GF.HP, "n_ff": GF.n_ff(GF.HP),
               "logits_shape": list(logits.shape), "decode_logits_shape": list(dlogits.shape),
               "generator": "reference llama.cpp + ggml.c (CPU, -march=x86-64-v3), llama_eval logits_all, 4 threads; "
                            "then one llama_eval per decode token at n_past = 40, 41, 42"},
              open(os.path.join(HERE, "llama_f32_tiny_manifest.json"), "w"), indent=1)
    print("model", sha, "logits", logits.shape, float(np.abs(logits).max()))
