"""Golden logits of the tiny "mostly Q4_1", "mostly Q5_0" and "mostly Q5_1" GGJT v3 LLaMAs (tests/ggjt_q5x_model.py)
from the REFERENCE's own llama.cpp + ggml.c, CPU-only build (oracle/_ref/libllama_ref_cpu.so, oracle/Makefile `ref`):
the 40-token prompt and the three single-token decode steps of tests/ggjt_model.py, per type.
Run here (needs the reference build): python tests/golden/gen_llama_q5x_golden.py"""
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [HERE, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
import ggjt_q5x_model as G5  # noqa: E402
from gen_llama_golden import ref_logits  # noqa: E402

if __name__ == "__main__":
    models = {}
    for t in G5.VARIANTS:
        with tempfile.TemporaryDirectory() as d:
            mp = os.path.join(d, f"tiny-{t}.ggjt")
            sha = G5.write(mp, t)
            logits, dlogits = ref_logits(os.path.join(ROOT, "oracle", "_ref", "libllama_ref_cpu.so"), mp,
                                         with_decode=True)
        assert np.isfinite(logits).all() and np.isfinite(dlogits).all()
        np.save(os.path.join(HERE, f"llama_{t}_tiny_logits.npy"), logits)
        np.save(os.path.join(HERE, f"llama_{t}_tiny_decode_logits.npy"), dlogits)
        models[t] = {"model_sha256": sha, "hparams": G5.hparams(t), "logits_shape": list(logits.shape),
                     "decode_logits_shape": list(dlogits.shape)}
        print(t, "model", sha, "logits", logits.shape, float(np.abs(logits).max()))
    json.dump({"models": models, "prompt": G5.PROMPT, "decode": G5.DECODE, "n_ff": G5.n_ff(G5.hparams("q41")),
               "generator": "reference llama.cpp + ggml.c (CPU, -march=x86-64-v3), llama_eval logits_all, 4 threads; "
                            "then one llama_eval per decode token at n_past = 40, 41, 42"},
              open(os.path.join(HERE, "llama_q5x_tiny_manifest.json"), "w"), indent=1)
