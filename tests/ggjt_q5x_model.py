"""The tiny LLaMA of tests/ggjt_model.py as a "mostly Q4_1", "mostly Q5_0" or "mostly Q5_1" GGJT v3 file: the same
shapes, seeds and f32 norms, every 2-D tensor in the one type (ggml type 3, 6 or 7), ftype 3, 8 or 9
(LLAMA_FTYPE_MOSTLY_Q4_1 / _Q5_0 / _Q5_1, llama.h).  The tensors are quantized with the restatement of
quantize_row_q4_1_reference / _q5_0_ / _q5_1_ (tests/q5x_ref.py, bit-exact to the reference's on its fixtures,
tests/test_q5x_ref.py).  Nothing is assumed about which quantizer a real file was written with: the golden logits are
computed by the reference from these very files (tests/golden/gen_llama_q5x_golden.py)."""
import hashlib
import struct

import numpy as np

import oracle as O
import q5x_ref as R
from ggjt_model import DECODE, HP as HP4, PROMPT, n_ff  # noqa: F401  (re-exported for the tests)

GGML_TYPE_F32 = 0
FTYPE = {"q41": 3, "q50": 8, "q51": 9}
VARIANTS = R.VARIANTS


def hparams(t):
    return dict(HP4, ftype=FTYPE[t])


def tensors(t, seed=0x5EED9000):
    """[(name, ggml_type, ne (ggml order), bytes)]: ggjt_model.tensors' order, seeds and distributions."""
    hp = hparams(t)
    E, V, F = hp["n_embd"], hp["n_vocab"], n_ff(hp)
    gtype = R.TYPES[t][0]
    out = []
    k = [0]

    def q(ne, std):
        k[0] += 1
        K, M = ne
        w = O.gaussian(M * K, seed + k[0], 0.0, std).reshape(M, K)
        return (gtype, ne, R.quantize_w(t, w).tobytes())

    def f32(ne, mean, std):
        k[0] += 1
        v = (O.gaussian(int(np.prod(ne)), seed + k[0], mean, std)).astype(np.float32)
        return (GGML_TYPE_F32, ne, v.tobytes())

    out.append(("tok_embeddings.weight",) + q((E, V), 1.0))
    out.append(("norm.weight",) + f32((E,), 1.0, 0.05))
    out.append(("output.weight",) + q((E, V), 0.05))
    for i in range(hp["n_layer"]):
        p = f"layers.{i}."
        out.append((p + "attention_norm.weight",) + f32((E,), 1.0, 0.05))
        for w in ("wq", "wk", "wv", "wo"):
            out.append((p + f"attention.{w}.weight",) + q((E, E), 0.05))
        out.append((p + "ffn_norm.weight",) + f32((E,), 1.0, 0.05))
        out.append((p + "feed_forward.w1.weight",) + q((E, F), 0.05))
        out.append((p + "feed_forward.w2.weight",) + q((F, E), 0.05))
        out.append((p + "feed_forward.w3.weight",) + q((E, F), 0.05))
    return out


def write(path, t, seed=0x5EED9000):
    """Write the model of type t (ggjt_model.write's container); returns the file's sha256."""
    hp = hparams(t)
    buf = bytearray()
    buf += struct.pack("<II", 0x67676A74, 3)
    buf += struct.pack("<7I", hp["n_vocab"], hp["n_embd"], hp["n_mult"], hp["n_head"], hp["n_layer"], hp["n_rot"],
                       hp["ftype"])
    for i in range(hp["n_vocab"]):
        tok = f"<t{i}>".encode()
        buf += struct.pack("<I", len(tok)) + tok + struct.pack("<f", -float(i))
    for name, typ, ne, data in tensors(t, seed):
        nb = name.encode()
        buf += struct.pack("<III", len(ne), len(nb), typ) + struct.pack(f"<{len(ne)}I", *ne) + nb
        buf += b"\0" * (-len(buf) & 31)
        buf += data
    with open(path, "wb") as f:
        f.write(buf)
    return hashlib.sha256(bytes(buf)).hexdigest()
