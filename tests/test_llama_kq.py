"""The tiny k-quants LLaMA files (tests/ggjt_kq_model.py) are the ones the golden logits were computed from
(tests/golden/gen_llama_kq_golden.py): per variant the writer's sha256 equals the manifest's, the tensor types are the
mix the reference's quantizer writes for that file type at n_layer = 2 (llama.cpp:2416-2440), every dequantized matrix
has the spread the model was scaled to, and the reference's CPU build with k-quants reproduces the committed logits
bit for bit at 1 and at 4 threads."""
import json
import os
import sys

import numpy as np
import pytest

import ggjt_kq_model as GK
from conftest import ROOT

GOLD = os.path.join(ROOT, "tests", "golden")
CPU_LIB = os.path.join(ROOT, "oracle", "_ref", "libllama_ref_kq_cpu.so")
MAN = json.load(open(os.path.join(GOLD, "llama_kq_tiny_manifest.json")))

Q40, Q2, Q3, Q4, Q5, Q6 = "Q4_0", "Q2_K", "Q3_K", "Q4_K", "Q5_K", "Q6_K"
# variant: (ftype, every layer's matrices, {matrix: type} in every layer, {matrix: type} in layer 1 only); the
# embeddings take the base type and output.weight is Q6_K throughout.  Written out here, not derived from GK.
TABLE = {
    "q4_0_q6k": (2, Q40, {}, {}),
    "q2_k": (10, Q2, {"wv": Q4, "wo": Q4, "w2": Q4}, {}),
    "q3_k_s": (11, Q3, {}, {}),
    "q3_k_m": (12, Q3, {"wv": Q4, "wo": Q4, "w2": Q4}, {}),
    "q3_k_l": (13, Q3, {"wv": Q5, "wo": Q5, "w2": Q5}, {}),
    "q4_k_s": (14, Q4, {}, {}),
    "q4_k_m": (15, Q4, {}, {"wv": Q6, "w2": Q6}),
    "q5_k_s": (16, Q5, {}, {}),
    "q5_k_m": (17, Q5, {}, {"wv": Q6, "w2": Q6}),
    "q6_k": (18, Q6, {}, {}),
}


def expected_types(v):
    ftype, base, every, last = TABLE[v]
    out = {"tok_embeddings.weight": base, "output.weight": Q6}
    for i in range(2):
        for w in ("wq", "wk", "wv", "wo", "w1", "w2", "w3"):
            part = "attention" if w in ("wq", "wk", "wv", "wo") else "feed_forward"
            t = every.get(w, base)
            if i == 1:
                t = last.get(w, t)
            out[f"layers.{i}.{part}.{w}.weight"] = t
    return out


def test_variants_are_the_table():
    assert set(GK.VARIANTS) == set(TABLE) == set(MAN["models"])
    assert GK.HP4["n_layer"] == 2 and GK.HP4["n_embd"] % 256 == 0 and GK.n_ff(GK.HP4) % 256 == 0


@pytest.mark.parametrize("v", GK.VARIANTS)
def test_model_file_matches_manifest(tmp_path, v):
    man = MAN["models"][v]
    mp = str(tmp_path / "m.ggjt")
    assert GK.write(mp, v) == man["model_sha256"]
    assert os.path.getsize(mp) == man["model_bytes"] <= 1600000
    assert man["hparams"] == GK.hparams(v) == dict(GK.HP4, ftype=TABLE[v][0])
    assert MAN["prompt"] == GK.PROMPT and MAN["decode"] == GK.DECODE and MAN["n_ff"] == 768
    logits = np.load(os.path.join(GOLD, f"llama_kq_{v}_tiny_logits.npy"))
    dlogits = np.load(os.path.join(GOLD, f"llama_kq_{v}_tiny_decode_logits.npy"))
    assert list(logits.shape) == man["logits_shape"] == [40, 320]
    assert list(dlogits.shape) == man["decode_logits_shape"] == [3, 320]
    assert logits.dtype == dlogits.dtype == np.float32
    assert np.isfinite(logits).all() and np.isfinite(dlogits).all()
    assert 1.0 < np.abs(logits).max() < 100.0          # logits of an ordinary size, as the q4_0 model's


@pytest.mark.parametrize("v", GK.VARIANTS)
def test_type_map_and_dequantized_spread(v):
    """Every 2-D tensor has the table's type and the block bytes of that type; dequantized with the numpy
    restatements, the layer matrices and output.weight have a standard deviation within [0.02, 0.1] and the
    embeddings within [0.5, 2], and every value is finite."""
    want = expected_types(v)
    assert {n: GK.TYPE_NAME[t] for n, t in GK.type_map(v).items()} == want == MAN["models"][v]["tensor_types"]
    seen = {}
    for name, typ, ne, data in GK.tensors(v):
        if len(ne) != 2:
            assert typ == GK.GGML_TYPE_F32 and len(data) == 4 * ne[0], name
            continue
        seen[name] = GK.TYPE_NAME[typ]
        K, M = ne
        assert K % 256 == 0, name
        per256 = 18 * 8 if typ == GK.GGML_TYPE_Q4_0 else GK.BLOCK_BYTES[typ]
        assert len(data) == M * (K // 256) * per256, name
        w = GK.dequantize(typ, data, ne)
        assert w.shape == (M, K) and np.isfinite(w).all(), name
        std = float(w.astype(np.float64).std())
        lo, hi = (0.5, 2.0) if name == "tok_embeddings.weight" else (0.02, 0.1)
        assert lo <= std <= hi, (name, std)
    assert seen == want


def test_generators_default_bytes_unchanged():
    """d_scale = 1 (the default) is the byte stream the per-matrix tests have always drawn; another scale changes
    the fp16 d / dmin fields only."""
    import q23k_ref as R23
    import q45k_ref as R45
    import q6k_ref as R6
    rng = lambda: np.random.default_rng(7)      # noqa: E731
    for gen, args, fields in ((R23.random_q23_K, (3, 512, True), [(108, 110)]),
                              (R23.random_q23_K, (3, 512, False), [(80, 84)]),
                              (R45.random_q45_K, (3, 512, True), [(0, 4)]),
                              (R45.random_q45_K, (3, 512, False), [(0, 4)]),
                              (R6.random_q6_K, (3, 512), [(208, 210)])):
        a, b, c = gen(rng(), *args), gen(rng(), *args, d_scale=1.0), gen(rng(), *args, d_scale=0.25)
        assert np.array_equal(a, b)
        bs = a.shape[1] // 2
        keep = np.ones(bs, bool)
        for lo, hi in fields:
            keep[lo:hi] = False
        assert np.array_equal(a.reshape(3, 2, bs)[:, :, keep], c.reshape(3, 2, bs)[:, :, keep])
        assert not np.array_equal(a, c)


@pytest.mark.skipif(not os.path.exists(CPU_LIB), reason="oracle/_ref/libllama_ref_kq_cpu.so not built")
@pytest.mark.parametrize("v", GK.VARIANTS)
def test_reference_kq_cpu_reproduces_golden_logits(tmp_path, v):
    sys.path.insert(0, GOLD)
    from gen_llama_golden import ref_logits
    mp = str(tmp_path / "m.ggjt")
    GK.write(mp, v)
    gold = np.load(os.path.join(GOLD, f"llama_kq_{v}_tiny_logits.npy"))
    dgold = np.load(os.path.join(GOLD, f"llama_kq_{v}_tiny_decode_logits.npy"))
    for n_threads in (1, 4):
        got, dec = ref_logits(CPU_LIB, mp, n_threads=n_threads, with_decode=True)
        assert np.array_equal(got.view(np.uint32), gold.view(np.uint32)), n_threads
        assert np.array_equal(dec.view(np.uint32), dgold.view(np.uint32)), n_threads
