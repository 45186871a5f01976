"""The tiny "mostly F16" LLaMA file (tests/ggjt_f16_model.py) is the one the golden logits were computed from
(tests/golden/gen_llama_f16_golden.py): its sha256 equals the manifest's, every 2-D tensor is F16 and ftype is 1."""
import json
import os

import numpy as np

import ggjt_f16_model as GF
from conftest import ROOT

GOLD = os.path.join(ROOT, "tests", "golden")


def test_model_file_matches_manifest(tmp_path):
    man = json.load(open(os.path.join(GOLD, "llama_f16_tiny_manifest.json")))
    assert GF.write(str(tmp_path / "mf.ggjt")) == man["model_sha256"]
    assert man["hparams"] == GF.HP and GF.HP["ftype"] == 1
    assert man["prompt"] == GF.PROMPT and man["decode"] == GF.DECODE
    logits = np.load(os.path.join(GOLD, "llama_f16_tiny_logits.npy"))
    dlogits = np.load(os.path.join(GOLD, "llama_f16_tiny_decode_logits.npy"))
    assert list(logits.shape) == man["logits_shape"] and list(dlogits.shape) == man["decode_logits_shape"]
    assert np.isfinite(logits).all() and np.isfinite(dlogits).all()


def test_every_matrix_is_f16():
    for name, typ, ne, data in GF.tensors():
        assert typ == (GF.GGML_TYPE_F16 if len(ne) == 2 else GF.GGML_TYPE_F32), name
        assert len(data) == int(np.prod(ne)) * (2 if len(ne) == 2 else 4), name
        if len(ne) == 2:
            assert ne[0] % 32 == 0 and np.isfinite(np.frombuffer(data, np.float16)).all(), name
