"""The tiny LLaMA of tests/ggjt_model.py as an "all F32" GGJT v3 file: the same shapes, seeds and f32 norms, every
tensor F32 (ggml type 0), ftype 0 (LLAMA_FTYPE_ALL_F32, llama.h): what the converter writes with --outtype f32.  The
weights are the oracle's gaussians as they are.  The golden logits are computed by the reference from this very file
(tests/golden/gen_llama_f32_golden.py)."""
import hashlib
import struct

import numpy as np

import oracle as O
from ggjt_model import DECODE, HP as HP4, PROMPT, n_ff  # noqa: F401  (re-exported for the tests)

GGML_TYPE_F32 = 0
HP = dict(HP4, ftype=0)


def tensors(hp=HP, seed=0x5EED9000):
    """[(name, ggml_type, ne (ggml order), bytes)]: ggjt_model.tensors' order, seeds and distributions."""
    E, V, F = hp["n_embd"], hp["n_vocab"], n_ff(hp)
    out = []
    k = [0]

    def f32(ne, mean, std):
        k[0] += 1
        v = (O.gaussian(int(np.prod(ne)), seed + k[0], mean, std)).astype(np.float32)
        return (GGML_TYPE_F32, ne, v.tobytes())

    out.append(("tok_embeddings.weight",) + f32((E, V), 0.0, 1.0))
    out.append(("norm.weight",) + f32((E,), 1.0, 0.05))
    out.append(("output.weight",) + f32((E, V), 0.0, 0.05))
    for i in range(hp["n_layer"]):
        p = f"layers.{i}."
        out.append((p + "attention_norm.weight",) + f32((E,), 1.0, 0.05))
        for w in ("wq", "wk", "wv", "wo"):
            out.append((p + f"attention.{w}.weight",) + f32((E, E), 0.0, 0.05))
        out.append((p + "ffn_norm.weight",) + f32((E,), 1.0, 0.05))
        out.append((p + "feed_forward.w1.weight",) + f32((E, F), 0.0, 0.05))
        out.append((p + "feed_forward.w2.weight",) + f32((F, E), 0.0, 0.05))
        out.append((p + "feed_forward.w3.weight",) + f32((E, F), 0.0, 0.05))
    return out


def write(path, hp=HP, seed=0x5EED9000):
    """Write the model (ggjt_model.write's container); returns the file's sha256."""
    buf = bytearray()
    buf += struct.pack("<II", 0x67676A74, 3)
    buf += struct.pack("<7I", hp["n_vocab"], hp["n_embd"], hp["n_mult"], hp["n_head"], hp["n_layer"], hp["n_rot"],
                       hp["ftype"])
    for i in range(hp["n_vocab"]):
        tok = f"<t{i}>".encode()
        buf += struct.pack("<I", len(tok)) + tok + struct.pack("<f", -float(i))
    for name, typ, ne, data in tensors(hp, seed):
        nb = name.encode()
        buf += struct.pack("<III", len(ne), len(nb), typ) + struct.pack(f"<{len(ne)}I", *ne) + nb
        buf += b"\0" * (-len(buf) & 31)
        buf += data
    with open(path, "wb") as f:
        f.write(buf)
    return hashlib.sha256(bytes(buf)).hexdigest()
