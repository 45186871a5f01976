"""The tiny "all F32" LLaMA file (tests/ggjt_f32_model.py) is the one the golden logits were computed from
(tests/golden/gen_llama_f32_golden.py): its sha256 equals the manifest's, every tensor is F32 and ftype is 0."""
import json
import os

import numpy as np

import ggjt_f32_model as GF
from conftest import ROOT

GOLD = os.path.join(ROOT, "tests", "golden")


def test_model_file_matches_manifest(tmp_path):
    man = json.load(open(os.path.join(GOLD, "llama_f32_tiny_manifest.json")))
    assert GF.write(str(tmp_path / "mf.ggjt")) == man["model_sha256"]
    assert man["hparams"] == GF.HP and GF.HP["ftype"] == 0
    assert man["prompt"] == GF.PROMPT and man["decode"] == GF.DECODE
    logits = np.load(os.path.join(GOLD, "llama_f32_tiny_logits.npy"))
    dlogits = np.load(os.path.join(GOLD, "llama_f32_tiny_decode_logits.npy"))
    assert list(logits.shape) == man["logits_shape"] and list(dlogits.shape) == man["decode_logits_shape"]
    assert np.isfinite(logits).all() and np.isfinite(dlogits).all()


def test_every_matrix_is_f32():
    n2 = 0
    for name, typ, ne, data in GF.tensors():
        assert typ == GF.GGML_TYPE_F32, name
        assert len(data) == int(np.prod(ne)) * 4, name
        if len(ne) == 2:
            n2 += 1
            assert ne[0] % 32 == 0 and np.isfinite(np.frombuffer(data, np.float32)).all(), name
    assert n2 == 2 + 7 * GF.HP["n_layer"]
