"""Golden logits of the tiny k-quants GGJT v3 LLaMAs (tests/ggjt_kq_model.py: one per file type the reference's
quantizer writes at QK_K = 256, plus the q4_0 file with its Q6_K output.weight) from the REFERENCE's own llama.cpp +
ggml.c + k_quants.c, CPU-only build with -DGGML_USE_K_QUANTS (oracle/_ref/libllama_ref_kq_cpu.so, oracle/Makefile
`ref`): the 40-token prompt and the three single-token decode steps of tests/ggjt_model.py, per variant.
Run here (needs the reference build): python tests/golden/gen_llama_kq_golden.py"""
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [HERE, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
import ggjt_kq_model as GK  # noqa: E402
from gen_llama_golden import ref_logits  # noqa: E402

if __name__ == "__main__":
    models = {}
    for v in GK.VARIANTS:
        with tempfile.TemporaryDirectory() as d:
            mp = os.path.join(d, f"tiny-{v}.ggjt")
            sha = GK.write(mp, v)
            size = os.path.getsize(mp)
            logits, dlogits = ref_logits(os.path.join(ROOT, "oracle", "_ref", "libllama_ref_kq_cpu.so"), mp,
                                         with_decode=True)
        assert np.isfinite(logits).all() and np.isfinite(dlogits).all()
        np.save(os.path.join(HERE, f"llama_kq_{v}_tiny_logits.npy"), logits)
        np.save(os.path.join(HERE, f"llama_kq_{v}_tiny_decode_logits.npy"), dlogits)
        models[v] = {"model_sha256": sha, "model_bytes": size, "hparams": GK.hparams(v),
                     "tensor_types": {n: GK.TYPE_NAME[t] for n, t in GK.type_map(v).items()},
                     "logits_shape": list(logits.shape), "decode_logits_shape": list(dlogits.shape)}
        print(v, "model", sha, size, "logits", logits.shape, float(np.abs(logits).max()))
    json.dump({"models": models, "prompt": GK.PROMPT, "decode": GK.DECODE, "n_ff": GK.n_ff(GK.hparams("q6_k")),
               "generator": "reference llama.cpp + ggml.c + k_quants.c (CPU, -march=x86-64-v3, -DGGML_USE_K_QUANTS), "
                            "llama_eval logits_all, 4 threads; then one llama_eval per decode token at n_past = 40, "
                            "41, 42"},
              open(os.path.join(HERE, "llama_kq_tiny_manifest.json"), "w"), indent=1)
