#!/usr/bin/env python3
"""The Q3_K and Q2_K decode GEMVs at HBM rate against the Q4_K GEMV, in one process (profiles/q23k_gemv.json).

N = 1 on the LLaMA-7B shapes 4096 -> 4096, 4096 -> 11008, 11008 -> 4096 (a layer is 4 + 2 + 1 = seven such launches).
Each arm (Q3_K, Q2_K, Q4_K weights through ggml_hip_mul_mat_q3_K / _q2_K / _q4_K algo 1) launches over a ROTATION of
distinct copies of its matrix whose total exceeds --set-mb (default 512 MB, twice the 256 MB last-level cache), so
every launch streams its weights from HBM.  One rotation is one HIP graph; after --settle-ms of load the arms' graphs
are replayed alternately for --rounds rounds, each replay timed by device events.  Reported per shape and arm:
microseconds per launch (median, min, max over rounds), TB/s of the algorithmic weight bytes, the fraction of 8 TB/s
(with its min-max spread), the time relative to the Q4_K arm's, and whether the arm is faster than Q4_K outside both
spreads.  The Q4_K arm is an existing kernel: the yardstick of the run (Q3_K and Q2_K read 0.76 and 0.58 of its
bytes).  Fails without a HIP device.

    python tools/q23k_bench.py [--rounds 10] [--out-dir profiles]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "llama.cpp-q_4_0_amd", "python"))
import ggml_hip  # noqa: E402

SHAPES = ((4096, 4096), (4096, 11008), (11008, 4096))          # (K, M)
# arm: (bytes per block, elements per block, byte offset of the fp16 d [and dmin] to make finite)
ARMS = {"q3_K": (110, 256, (108,)), "q2_K": (84, 256, (80, 82)), "q4_K": (144, 256, (0, 2))}
HBM_TBS = 8.0
DB = ggml_hip.DeviceBuffer


def random_blocks(rng, nblocks, bsize, d_offsets):
    """nblocks quantized blocks of bsize bytes: random payload, finite fp16 scale fields."""
    w = rng.integers(0, 256, size=(nblocks, bsize), dtype=np.uint8)
    for off in d_offsets:
        w[:, off:off + 2] = np.array([0.01], np.float16).view(np.uint8)
    return w


def launch(name, w, K, M, xd, yd, s, off):
    f = {"q3_K": ggml_hip.mul_mat_q3_K, "q2_K": ggml_hip.mul_mat_q2_K, "q4_K": ggml_hip.mul_mat_q4_K}[name]
    f(w, K, M, xd, 1, yd, algo=1, stream=s, w_off=off)


def timed_rounds(s, graphs, rounds, settle_ms, per_graph):
    e0, e1 = ggml_hip.Event(), ggml_hip.Event()
    e0.record(s)
    while True:                                                # settle: at least settle_ms of back-to-back load
        for g in graphs.values():
            g.launch()
        e1.record(s)
        if e0.elapsed_ms(e1) >= settle_ms:
            break
    us = {k: [] for k in graphs}
    for _ in range(rounds):
        for k, g in graphs.items():
            e0.record(s)
            g.launch()
            e1.record(s)
            ms = e0.elapsed_ms(e1)
            if ms < 0:
                sys.exit("q23k_bench: event timing failed")
            us[k].append(ms * 1e3 / per_graph[k])
    return us


def run(L, s, a):
    rng = np.random.default_rng(0x23B)
    rows = []
    for K, M in SHAPES:
        x = rng.standard_normal((1, K)).astype(np.float32)
        xd = DB.from_array(x)
        arms, graphs, per_graph = {}, {}, {}
        for name, (bsize, bel, d_offsets) in ARMS.items():
            mat = M * (K // bel) * bsize                       # a multiple of 16 on these shapes
            copies = max(2, -(-a.set_mb * (1 << 20) // mat))
            chunk = random_blocks(rng, (1 << 22) // bel * 8, bsize, d_offsets).ravel()
            host = np.tile(chunk, -(-copies * mat // chunk.size))[:copies * mat]
            arm = arms[name] = {"bytes": mat, "copies": copies, "w": DB.from_array(host), "y": DB(M * 4)}
            del host
            launch(name, arm["w"], K, M, xd, arm["y"], s, 0)   # code objects loaded
            ggml_hip.check(L.ggml_hip_stream_synchronize(s))
            g = ggml_hip.Graph(s)
            with g:
                for i in range(copies):
                    launch(name, arm["w"], K, M, xd, arm["y"], s, i * mat)
            graphs[name], per_graph[name] = g, copies
        us = timed_rounds(s, graphs, a.rounds, a.settle_ms, per_graph)
        row = {"K": K, "M": M}
        for name, arm in arms.items():
            med, lo, hi = float(np.median(us[name])), min(us[name]), max(us[name])
            tbs = arm["bytes"] / med * 1e-6
            row[name] = {"us": round(med, 2), "us_min": round(lo, 2), "us_max": round(hi, 2),
                         "weight_bytes": arm["bytes"], "copies": arm["copies"], "TBs": round(tbs, 3),
                         "frac_hbm": round(tbs / HBM_TBS, 3),
                         "frac_hbm_best": round(arm["bytes"] / lo * 1e-6 / HBM_TBS, 3),
                         "frac_hbm_worst": round(arm["bytes"] / hi * 1e-6 / HBM_TBS, 3)}
        for name in ("q3_K", "q2_K"):
            row[f"{name}_over_q4_K_us"] = round(row[name]["us"] / row["q4_K"]["us"], 3)
            row[f"{name}_over_q4_K_bytes"] = round(row[name]["weight_bytes"] / row["q4_K"]["weight_bytes"], 3)
            row[f"{name}_faster_than_q4_K_outside_spread"] = bool(row[name]["us_max"] < row["q4_K"]["us_min"])
        rows.append(row)
        del arms, graphs
    layer = {name: round(sum(r[name]["us"] * mult for r, mult in zip(rows, (4, 2, 1))), 1) for name in ARMS}
    return {"bench": "q23k_gemv", "N": 1, "set_mb": a.set_mb, "rounds": a.rounds, "settle_ms": a.settle_ms,
            "hbm_TBs": HBM_TBS, "shapes": rows, "layer_us": layer,
            "layer_us_note": "4 x (4096 -> 4096) + 2 x (4096 -> 11008) + 1 x (11008 -> 4096) launches, one LLaMA-7B layer",
            "timing": "HIP-graph replays over a rotation of weight copies larger than the last-level cache, device "
                      "events, arms interleaved, median over rounds"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--settle-ms", type=float, default=40.0)
    ap.add_argument("--set-mb", type=int, default=512)
    ap.add_argument("--out-dir", default=None)
    a = ap.parse_args()
    L = ggml_hip.load()
    if L.ggml_hip_device_count() < 1:
        sys.exit("q23k_bench: no HIP device")
    ggml_hip.check(L.ggml_hip_set_device(0))
    ggml_hip.check(L.ggml_hip_set_exact(0))
    s = L.ggml_hip_default_stream()
    line = json.dumps(run(L, s, a))
    print(line, flush=True)
    if a.out_dir:
        os.makedirs(a.out_dir, exist_ok=True)
        with open(os.path.join(a.out_dir, "q23k_gemv.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
