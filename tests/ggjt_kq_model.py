"""The tiny LLaMA of tests/ggjt_model.py as the k-quants GGJT v3 files the reference's quantizer writes at QK_K = 256:
the same container, hparams, vocab, tensor order, f32 norms, PROMPT and DECODE; one variant per file type, with the
mix of tensor types of llama.cpp:2416-2440 for n_layer = 2 (use_more_bits(i, 2) is false for layer 0, true for layer
1).  TYPE_MAP below is that table; tok_embeddings.weight takes the variant's base type and output.weight is Q6_K in
every variant, q4_0_q6k included (what the reference's default build writes for a q4_0 file).

                 ftype  layer matrices   exceptions
    q4_0_q6k       2    Q4_0             -
    q2_k          10    Q2_K             wv, wo, w2: Q4_K
    q3_k_s        11    Q3_K             -
    q3_k_m        12    Q3_K             wv, wo, w2: Q4_K
    q3_k_l        13    Q3_K             wv, wo, w2: Q5_K
    q4_k_s        14    Q4_K             -
    q4_k_m        15    Q4_K             wv, w2 of layer 1: Q6_K
    q5_k_s        16    Q5_K             -
    q5_k_m        17    Q5_K             wv, w2 of layer 1: Q6_K
    q6_k          18    Q6_K             -

The k-quant matrices are random valid blocks of the per-matrix tests' generators (q23k_ref.random_q23_K,
q45k_ref.random_q45_K, q6k_ref.random_q6_K) without their special blocks, with d and dmin scaled per type so that the
dequantized matrix has a standard deviation near 0.05 (layer matrices, output.weight) or 1 (tok_embeddings), as the
q4_0 model's matrices have.  The Q4_0 matrices are ggjt_model's (same seeds, O.quantize_q4_0).  Nothing is assumed
about a real quantizer's output: the golden logits are computed by the reference from these very files
(tests/golden/gen_llama_kq_golden.py)."""
import hashlib
import struct

import numpy as np

import oracle as O
import q23k_ref as R23
import q45k_ref as R45
import q6k_ref as R6
from ggjt_model import DECODE, HP as HP4, PROMPT, n_ff  # noqa: F401  (re-exported for the tests)

GGML_TYPE_F32, GGML_TYPE_Q4_0 = 0, 2
Q2_K, Q3_K, Q4_K, Q5_K, Q6_K = 10, 11, 12, 13, 14                   # ggml.h:245-249
TYPE_NAME = {GGML_TYPE_Q4_0: "Q4_0", Q2_K: "Q2_K", Q3_K: "Q3_K", Q4_K: "Q4_K", Q5_K: "Q5_K", Q6_K: "Q6_K"}
BLOCK_BYTES = {Q2_K: R23.Q2KB, Q3_K: R23.Q3KB, Q4_K: R45.Q4KB, Q5_K: R45.Q5KB, Q6_K: R6.Q6KB}

# variant -> (ftype (llama.h LLAMA_FTYPE_MOSTLY_*), base type, {matrix: type} for every layer, the same for layer 1 only)
_ATT_FFN = ("wv", "wo", "w2")
VARIANT_DEF = {
    "q4_0_q6k": (2, GGML_TYPE_Q4_0, {}, {}),
    "q2_k": (10, Q2_K, dict.fromkeys(_ATT_FFN, Q4_K), {}),
    "q3_k_s": (11, Q3_K, {}, {}),
    "q3_k_m": (12, Q3_K, dict.fromkeys(_ATT_FFN, Q4_K), {}),
    "q3_k_l": (13, Q3_K, dict.fromkeys(_ATT_FFN, Q5_K), {}),
    "q4_k_s": (14, Q4_K, {}, {}),
    "q4_k_m": (15, Q4_K, {}, {"wv": Q6_K, "w2": Q6_K}),
    "q5_k_s": (16, Q5_K, {}, {}),
    "q5_k_m": (17, Q5_K, {}, {"wv": Q6_K, "w2": Q6_K}),
    "q6_k": (18, Q6_K, {}, {}),
}
VARIANTS = tuple(VARIANT_DEF)
MATRICES = ("wq", "wk", "wv", "wo", "w1", "w2", "w3")            # the seven weight mul_mats of a layer, in file order

# standard deviation of a dequantized matrix of the generators at d_scale = 1 (d ~ 0.01 N(0, 1), dmin ~ 0.005 N(0, 1),
# uniform random scales and quants); d_scale = target / this
_STD_AT_1 = {Q2_K: 0.17, Q3_K: 0.4, Q4_K: 3.2, Q5_K: 6.6, Q6_K: 13.0}
STD_LAYER, STD_EMBED = 0.05, 1.0


def hparams(v):
    return dict(HP4, ftype=VARIANT_DEF[v][0])


def matrix_type(v, layer, w):
    _, base, every, last = VARIANT_DEF[v]
    if layer == HP4["n_layer"] - 1 and w in last:
        return last[w]
    return every.get(w, base)


def type_map(v):
    """{tensor name: ggml type} of every 2-D tensor of variant v"""
    out = {"tok_embeddings.weight": VARIANT_DEF[v][1], "output.weight": Q6_K}
    for i in range(HP4["n_layer"]):
        for w in MATRICES:
            part = "attention" if w in ("wq", "wk", "wv", "wo") else "feed_forward"
            out[f"layers.{i}.{part}.{w}.weight"] = matrix_type(v, i, w)
    return out


def random_matrix(typ, ne, seed, std):
    """bytes of a random valid [M][K] matrix of k-quant type typ whose dequantized std is near `std`"""
    K, M = ne
    rng = np.random.default_rng([0x4B51, seed])
    s = std / _STD_AT_1[typ]
    if typ in (Q2_K, Q3_K):
        b = R23.random_q23_K(rng, M, K, typ == Q3_K, special=False, d_scale=s)
    elif typ in (Q4_K, Q5_K):
        b = R45.random_q45_K(rng, M, K, typ == Q5_K, special=False, d_scale=s)
    else:
        b = R6.random_q6_K(rng, M, K, special_d=False, d_scale=s)
    assert b.shape == (M, K // 256 * BLOCK_BYTES[typ])
    return np.ascontiguousarray(b).tobytes()


def dequantize(typ, data, ne):
    """f32 [M, K] of a 2-D tensor's bytes (the numpy dequantizers of the per-matrix tests)"""
    K, M = ne
    wq = np.frombuffer(data, np.uint8).reshape(M, -1)
    if typ == GGML_TYPE_Q4_0:
        return O.dequantize_q4_0(wq, K)
    if typ in (Q2_K, Q3_K):
        return R23.dequantize(wq, K, typ == Q3_K)
    if typ in (Q4_K, Q5_K):
        return R45.dequantize_q45_K(wq, K, typ == Q5_K)
    return R6.dequantize_q6_K(wq, K)


def tensors(v, seed=0x5EED9000):
    """[(name, ggml_type, ne (ggml order), bytes)]: ggjt_model.tensors' order and seeds (one per tensor)."""
    hp = hparams(v)
    E, V, F = hp["n_embd"], hp["n_vocab"], n_ff(hp)
    types = type_map(v)
    out = []
    k = [0]

    def mat(name, ne, std):
        k[0] += 1
        typ = types[name]
        K, M = ne
        if typ == GGML_TYPE_Q4_0:
            w = O.gaussian(M * K, seed + k[0], 0.0, std).reshape(M, K)
            data = O.quantize_q4_0(w)[0].tobytes()
        else:
            data = random_matrix(typ, ne, seed + k[0], std)
        out.append((name, typ, ne, data))

    def f32(name, ne, mean, std):
        k[0] += 1
        vv = (O.gaussian(int(np.prod(ne)), seed + k[0], mean, std)).astype(np.float32)
        out.append((name, GGML_TYPE_F32, ne, vv.tobytes()))

    mat("tok_embeddings.weight", (E, V), STD_EMBED)
    f32("norm.weight", (E,), 1.0, 0.05)
    mat("output.weight", (E, V), STD_LAYER)
    for i in range(hp["n_layer"]):
        p = f"layers.{i}."
        f32(p + "attention_norm.weight", (E,), 1.0, 0.05)
        for w in ("wq", "wk", "wv", "wo"):
            mat(p + f"attention.{w}.weight", (E, E), STD_LAYER)
        f32(p + "ffn_norm.weight", (E,), 1.0, 0.05)
        mat(p + "feed_forward.w1.weight", (E, F), STD_LAYER)
        mat(p + "feed_forward.w2.weight", (F, E), STD_LAYER)
        mat(p + "feed_forward.w3.weight", (E, F), STD_LAYER)
    return out


def write(path, v, seed=0x5EED9000):
    """Write the model of variant v (ggjt_model.write's container); returns the file's sha256."""
    hp = hparams(v)
    buf = bytearray()
    buf += struct.pack("<II", 0x67676A74, 3)
    buf += struct.pack("<7I", hp["n_vocab"], hp["n_embd"], hp["n_mult"], hp["n_head"], hp["n_layer"], hp["n_rot"],
                       hp["ftype"])
    for i in range(hp["n_vocab"]):
        tok = f"<t{i}>".encode()
        buf += struct.pack("<I", len(tok)) + tok + struct.pack("<f", -float(i))
    for name, typ, ne, data in tensors(v, seed):
        nb = name.encode()
        buf += struct.pack("<III", len(ne), len(nb), typ) + struct.pack(f"<{len(ne)}I", *ne) + nb
        buf += b"\0" * (-len(buf) & 31)
        buf += data
    with open(path, "wb") as f:
        f.write(buf)
    return hashlib.sha256(bytes(buf)).hexdigest()
