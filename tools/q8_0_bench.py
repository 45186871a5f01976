#!/usr/bin/env python3
"""Q8_0 weights on the device: the decode GEMV at HBM rate against the q4_0 GEMV, and the prefill crossover
between the column-tiled GEMV and the per-call int8 image + k_gemm8, in one process.

Decode (profiles/q8_0_gemv.json).  N = 1 on the LLaMA-7B shapes 4096 -> 4096, 4096 -> 11008, 11008 -> 4096.  Each
arm (Q8_0 weights through ggml_hip_mul_mat_q8_0 algo 1, q4_0 weights through ggml_hip_mul_mat_q4_0_ex algo 1)
launches over a ROTATION of distinct copies of its matrix whose total exceeds --set-mb (default 512 MB, twice the
256 MB last-level cache), so every launch streams its weights from HBM.  One rotation is one HIP graph; after
--settle-ms of load the two arms' graphs are replayed alternately for --rounds rounds, each replay timed by
device events.  Reported per shape and arm: microseconds per launch (median, min, max over rounds), TB/s of
weight bytes, and the fraction of 8 TB/s.

Prefill (profiles/q8_0_gemm.json).  M = K = 4096, N = 9 .. 512: algo 1 (GEMV tiles of 8 columns) against algo 2
(gemm8_prep_x + k_prep8_w<W8_0> + k_gemm8: the weight-image launch is inside the timed arm), graphs of --launches
calls, warm, interleaved as above.  `min_n` is the smallest swept N from which the GEMM arm wins at every larger
swept N (the value for the default of q8_0_gemm_min_n); null if it never does.  The two arms are checked against
each other within 1e-3 of the largest |y| before they are timed.  Fails without a HIP device.

    python tools/q8_0_bench.py [--what decode|prefill|both] [--rounds 10] [--out-dir profiles]
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
NS = (9, 16, 32, 64, 128, 256, 512)
HBM_TBS = 8.0
DB = ggml_hip.DeviceBuffer


def random_blocks(rng, nblocks, bsize):
    """nblocks quantized blocks of bsize bytes (fp16 d first): random payload, a finite d in every block."""
    w = rng.integers(0, 256, size=(nblocks, bsize), dtype=np.uint8)
    w[:, 0:2] = np.array([0.01], np.float16).view(np.uint8)
    return w


def timed_rounds(L, s, graphs, rounds, settle_ms, per_graph, who):
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
                sys.exit(f"{who}: event timing failed")
            us[k].append(ms * 1e3 / per_graph[k])
    return us


def stats(us):
    return {"us": round(float(np.median(us)), 2), "us_min": round(min(us), 2), "us_max": round(max(us), 2)}


def decode(L, s, a):
    rng = np.random.default_rng(0x80D)
    chunk_blocks = 1 << 20
    rows = []
    for K, M in SHAPES:
        arms = {}
        for name, bsize in (("q8_0", 34), ("q4_0", 18)):
            mat = M * (K // 32) * bsize
            copies = max(2, -(-a.set_mb * (1 << 20) // mat))
            chunk = random_blocks(rng, chunk_blocks, bsize).ravel()
            host = np.tile(chunk, -(-copies * mat // chunk.size))[:copies * mat]
            arms[name] = {"bytes": mat, "copies": copies, "w": DB.from_array(host), "y": DB(M * 4)}
            del host
        x = rng.standard_normal((1, K)).astype(np.float32)
        xd = DB.from_array(x)
        graphs, per_graph = {}, {}
        for name, arm in arms.items():
            def fn(i, name=name, arm=arm):
                off = i * arm["bytes"]
                if name == "q8_0":
                    ggml_hip.mul_mat_q8_0(arm["w"], K, M, xd, 1, arm["y"], algo=1, stream=s, w_off=off)
                else:
                    ggml_hip.mul_mat(arm["w"], K, M, xd, 1, arm["y"], algo=1, stream=s, w_off=off)
            fn(0)                                              # code objects loaded
            ggml_hip.check(L.ggml_hip_stream_synchronize(s))
            g = ggml_hip.Graph(s)
            with g:
                for i in range(arm["copies"]):
                    fn(i)
            graphs[name], per_graph[name] = g, arm["copies"]
        us = timed_rounds(L, s, graphs, a.rounds, a.settle_ms, per_graph, "q8_0_bench decode")
        row = {"K": K, "M": M}
        for name, arm in arms.items():
            st = stats(us[name])
            tbs = arm["bytes"] / st["us"] * 1e-6
            row[name] = dict(st, weight_bytes=arm["bytes"], copies=arm["copies"], TBs=round(tbs, 3),
                             frac_hbm=round(tbs / HBM_TBS, 3),
                             frac_hbm_best=round(arm["bytes"] / st["us_min"] * 1e-6 / HBM_TBS, 3),
                             frac_hbm_worst=round(arm["bytes"] / st["us_max"] * 1e-6 / HBM_TBS, 3))
        row["q8_0_over_q4_0_us"] = round(row["q8_0"]["us"] / row["q4_0"]["us"], 3)
        rows.append(row)
        del arms, graphs
    tok = {name: round(sum(r[name]["us"] * mult for r, mult in zip(rows, (4, 2, 1))), 1) for name in ("q8_0", "q4_0")}
    return {"bench": "q8_0_gemv", "N": 1, "set_mb": a.set_mb, "rounds": a.rounds, "settle_ms": a.settle_ms,
            "hbm_TBs": HBM_TBS, "shapes": rows, "layer_us": tok,
            "layer_us_note": "4 x (4096 -> 4096) + 2 x (4096 -> 11008) + 1 x (11008 -> 4096) launches, one LLaMA-7B layer",
            "timing": "HIP-graph replays over a rotation of weight copies larger than the last-level cache, device "
                      "events, arms interleaved, median over rounds"}


def prefill(L, s, a):
    K = M = 4096
    rng = np.random.default_rng(0x80E)
    w = random_blocks(rng, M * (K // 32), 34)
    x = rng.standard_normal((max(NS), K)).astype(np.float32)
    wd, xd = DB.from_array(w), DB.from_array(x)
    yd = {algo: DB(max(NS) * M * 4) for algo in (1, 2)}
    ggml_hip.check(L.ggml_hip_reserve_workspace_mm(K, max(NS), M))
    sweep = []
    for N in NS:
        graphs, per_graph = {}, {}
        for algo in (1, 2):
            def fn(algo=algo):
                ggml_hip.mul_mat_q8_0(wd, K, M, xd, N, yd[algo], algo=algo, stream=s)
            fn()
            ggml_hip.check(L.ggml_hip_stream_synchronize(s))
            g = ggml_hip.Graph(s)
            with g:
                for _ in range(a.launches):
                    fn()
            graphs[algo], per_graph[algo] = g, a.launches
        g.launch()
        ggml_hip.check(L.ggml_hip_stream_synchronize(s))
        y1, y2 = yd[1].download((N, M), np.float32), yd[2].download((N, M), np.float32)
        if not np.abs(y1 - y2).max() <= 1e-3 * np.abs(y1).max():
            sys.exit(f"q8_0_bench prefill: algo 2 differs from algo 1 at N = {N}")
        us = timed_rounds(L, s, graphs, a.rounds, a.settle_ms, per_graph, "q8_0_bench prefill")
        row = {"N": N}
        for algo, name in ((1, "gemv"), (2, "gemm")):
            st = stats(us[algo])
            row.update({f"{name}_{k}": v for k, v in st.items()})
            row[f"{name}_TOPs"] = round(2.0 * M * K * N / st["us"] * 1e-6, 1)
        row["gemv_over_gemm"] = round(row["gemv_us"] / row["gemm_us"], 3)
        sweep.append(row)
    min_n = None
    for row in reversed(sweep):
        if row["gemv_over_gemm"] <= 1.0:
            break
        min_n = row["N"]
    return {"bench": "q8_0_gemm", "K": K, "M": M, "weight_bytes": M * (K // 32) * 34, "launches_per_graph": a.launches,
            "rounds": a.rounds, "settle_ms": a.settle_ms, "sweep": sweep, "min_n": min_n,
            "gemm_arm": "gemm8_prep_x + k_prep8_w<W8_0> (weight image per call) + k_gemm8",
            "timing": "warm HIP-graph replays, device events, arms interleaved, median over rounds"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=("decode", "prefill", "both"), default="both")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--settle-ms", type=float, default=40.0)
    ap.add_argument("--set-mb", type=int, default=512)
    ap.add_argument("--out-dir", default=None)
    a = ap.parse_args()
    L = ggml_hip.load()
    if L.ggml_hip_device_count() < 1:
        sys.exit("q8_0_bench: no HIP device")
    ggml_hip.check(L.ggml_hip_set_device(0))
    ggml_hip.check(L.ggml_hip_set_exact(0))
    s = L.ggml_hip_default_stream()
    for what, fn, out in (("decode", decode, "q8_0_gemv.json"), ("prefill", prefill, "q8_0_gemm.json")):
        if a.what not in (what, "both"):
            continue
        line = json.dumps(fn(L, s, a))
        print(line, flush=True)
        if a.out_dir:
            os.makedirs(a.out_dir, exist_ok=True)
            with open(os.path.join(a.out_dir, out), "w") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
