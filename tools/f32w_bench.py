#!/usr/bin/env python3
"""F32 weights on the device (csrc/f32_w.hip, csrc/f32_w_gemm.hip), in one process, into profiles/f32w.json.

GEMV.  N = 1, 4 and 8 on the LLaMA-7B shapes 4096 -> 4096, 4096 -> 11008, 11008 -> 4096 and the lm_head 4096 -> 32000:
ggml_hip_mul_mat_f32 algo 1 (k_gemv_f32w) against ggml_hip_mul_mat_f16 algo 1 (k_gemv_f16w) on a matrix of the same
shape.  The F32 launch moves twice the bytes, so its time is expected within 2 x the F16 time plus the run's spread.
Each arm launches over a ROTATION of distinct copies of its matrix whose total exceeds --set-mb (default 512 MB, twice
the 256 MB last-level cache), so every launch streams its weights from HBM.  One rotation is one HIP graph; after
--settle-ms of load the arms' graphs are replayed alternately for --rounds rounds, each replay timed by device events.
Per shape, N and arm: microseconds per call (median, min, max over rounds), TB/s of weight bytes, the fraction of
8 TB/s, and f32 / f16.

GEMM.  The same four shapes, N = 9 .. 512, over the same rotation, graphs and alternation: algo 1 (GEMV column tiles of
gemv_f32w_max_tokens(K)), algo 12 (k_gemm_f32w) with the K split auto takes, and algo 12 under each pinned split (what
the auto rule is held against).  Per cell: median, min, max; for algo 12 the fraction of the derived floor
max(4 M K / 8 TB/s, 2 M K N / 157 TF).  algo 12 WINS a cell where its median is below the GEMV's and its max below the
GEMV's min.  `recommended_min_n` is the smallest swept N from which it wins every cell of every layer shape (the
default of GGML_HIP_F32W_GEMM_MIN_N); null if there is none.  The arms are checked against each other before they are
timed.  Fails without a HIP device.

    python tools/f32w_bench.py [--what gemv|gemm|both] [--rounds 10] [--out-dir profiles]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "llama.cpp-q_4_0_amd", "python"))
import ggml_hip  # noqa: E402

LAYER_SHAPES = ((4096, 4096), (4096, 11008), (11008, 4096))    # (K, M)
SHAPES = LAYER_SHAPES + ((4096, 32000),)
DECODE_NS = (1, 4, 8)
SWEEP_NS = (9, 16, 32, 64, 128, 512)
SPLITS = (1, 2, 4)
HBM_TBS = 8.0
MFMA_TFS = 157.0
DB = ggml_hip.DeviceBuffer


def timed_rounds(s, graphs, rounds, settle_ms, per_graph, who):
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


def rotation(rng, K, M, set_mb, dtype):
    """(device buffer of `copies` distinct matrices [M][K] of 0.02 N(0, 1), bytes of one, copies)"""
    mat = M * K * np.dtype(dtype).itemsize
    copies = max(2, -(-set_mb * (1 << 20) // mat))
    chunk = (rng.standard_normal(1 << 22) * 0.02).astype(dtype)
    host = np.tile(chunk, -(-copies * M * K // chunk.size))[:copies * M * K]
    if dtype == np.float16:
        host = host.view(np.uint16)
    return DB.from_array(host), mat, copies


def graph_of(s, copies, fn):
    fn(0)                                                      # code objects loaded
    g = ggml_hip.Graph(s)
    with g:
        for i in range(copies):
            fn(i)
    return g


def gemv(L, s, a):
    rng = np.random.default_rng(0xF32D)
    rows = []
    for K, M in SHAPES:
        w32, mat32, c32 = rotation(rng, K, M, a.set_mb, np.float32)
        w16, mat16, c16 = rotation(rng, K, M, a.set_mb, np.float16)
        xd = DB.from_array(rng.standard_normal((max(DECODE_NS), K)).astype(np.float32))
        yd = {name: DB(max(DECODE_NS) * M * 4) for name in ("f32", "f16")}
        for N in DECODE_NS:
            def f32(i):
                ggml_hip.mul_mat_f32(w32, K, M, xd, N, yd["f32"], algo=1, stream=s, w_off=i * mat32)

            def f16(i):
                ggml_hip.mul_mat_f16(w16, K, M, xd, N, yd["f16"], algo=1, stream=s, w_off=i * mat16)
            graphs = {"f32": graph_of(s, c32, f32), "f16": graph_of(s, c16, f16)}
            ggml_hip.check(L.ggml_hip_stream_synchronize(s))
            us = timed_rounds(s, graphs, a.rounds, a.settle_ms, {"f32": c32, "f16": c16}, "f32w_bench gemv")
            row = {"K": K, "M": M, "N": N, "copies": {"f32": c32, "f16": c16}}
            for name, mat in (("f32", mat32), ("f16", mat16)):
                st = stats(us[name])
                tbs = mat / st["us"] * 1e-6
                row[name] = dict(st, weight_bytes=mat, TBs=round(tbs, 3), frac_hbm=round(tbs / HBM_TBS, 3))
            row["f32_over_f16_us"] = round(row["f32"]["us"] / row["f16"]["us"], 2)
            row["within_2x_plus_spread"] = row["f32"]["us"] <= 2 * row["f16"]["us"] + (row["f16"]["us_max"] - row["f16"]["us_min"]) \
                + (row["f32"]["us_max"] - row["f32"]["us_min"])
            rows.append(row)
            del graphs
        for b in [w32, w16, xd] + list(yd.values()):
            b.free()
    return {"set_mb": a.set_mb, "rounds": a.rounds, "settle_ms": a.settle_ms, "hbm_TBs": HBM_TBS,
            "nt_weight_loads": os.environ.get("GGML_HIP_F32W_NT", "1") != "0", "rows": rows,
            "arms": {"f32": "ggml_hip_mul_mat_f32 algo 1 (k_gemv_f32w; K = 11008 takes 2 columns per launch, so N = 4 "
                            "and 8 are 2 and 4 launches)",
                     "f16": "ggml_hip_mul_mat_f16 algo 1 (k_gemv_f16w; K = 11008 takes 5 columns per launch)"}}


def gemm(L, s, a):
    rng = np.random.default_rng(0xF32E)
    pin = L.ggml_hip_debug_set_f32w_gemm_ksplit
    arms = {"gemv": (1, 0), "gemm": (12, 0)}                   # arm -> (algo, pinned split; 0 auto)
    arms.update({f"gemm_s{k}": (12, k) for k in SPLITS})
    shapes = []
    for K, M in SHAPES:
        wd, mat, copies = rotation(rng, K, M, a.set_mb, np.float32)
        nmax = max(SWEEP_NS)
        xd = DB.from_array(rng.standard_normal((nmax, K)).astype(np.float32))
        yd = {name: DB(nmax * M * 4) for name in arms}
        pin(4)                                                 # the workspace of the widest split, ahead of the captures
        ggml_hip.check(L.ggml_hip_reserve_workspace_mm(K, nmax, M), "reserve")
        pin(0)
        sweep = []
        for N in SWEEP_NS:
            def call(name, i):
                algo, split = arms[name]
                pin(split)
                ggml_hip.mul_mat_f32(wd, K, M, xd, N, yd[name], algo=algo, stream=s, w_off=i * mat)
                pin(0)
            ys = {}
            for name in arms:
                call(name, 0)
                ggml_hip.check(L.ggml_hip_stream_synchronize(s))
                ys[name] = yd[name].download((N, M), np.float32)
                if not np.abs(ys[name] - ys["gemv"]).max() <= 1e-4 * np.abs(ys["gemv"]).max():
                    sys.exit(f"f32w_bench gemm: arm {name} differs from gemv at K = {K}, M = {M}, N = {N}")
            graphs, per_graph = {}, {}
            for name in arms:
                g = ggml_hip.Graph(s)
                with g:
                    for i in range(copies):
                        call(name, i)
                graphs[name], per_graph[name] = g, copies
            us = timed_rounds(s, graphs, a.rounds, a.settle_ms, per_graph, "f32w_bench gemm")
            floor = max(mat / (HBM_TBS * 1e12), 2.0 * K * M * N / (MFMA_TFS * 1e12)) * 1e6
            row = {"N": N, "floor_us": round(floor, 2), "auto_split": L.ggml_hip_debug_f32w_gemm_ksplit(K, M, N)}
            for name in arms:
                row.update({f"{name}_{k}": v for k, v in stats(us[name]).items()})
            row["gemm_floor_frac"] = round(floor / row["gemm_us"], 3)
            row["gemm_TFLOPs"] = round(2.0 * M * K * N / row["gemm_us"] * 1e-6, 1)
            row["gemm_wins"] = row["gemm_us"] < row["gemv_us"] and row["gemm_us_max"] < row["gemv_us_min"]
            best = min(SPLITS, key=lambda k: row[f"gemm_s{k}_us"])
            row["best_split"] = best
            row["auto_over_best"] = round(row["gemm_us"] / row[f"gemm_s{best}_us"], 3)
            sweep.append(row)
            del graphs
        shapes.append({"K": K, "M": M, "weight_bytes": mat, "copies": copies, "sweep": sweep})
        for b in [wd, xd] + list(yd.values()):
            b.free()
    rec = None
    layer = [sh for sh in shapes if (sh["K"], sh["M"]) in LAYER_SHAPES]
    for i in reversed(range(len(SWEEP_NS))):
        if not all(sh["sweep"][i]["gemm_wins"] for sh in layer):
            break
        rec = SWEEP_NS[i]
    return {"set_mb": a.set_mb, "rounds": a.rounds, "settle_ms": a.settle_ms, "hbm_TBs": HBM_TBS, "mfma_TFs": MFMA_TFS,
            "shapes": shapes, "recommended_min_n": rec,
            "arms": {"gemv": "algo 1, column tiles of gemv_f32w_max_tokens(K)",
                     "gemm": "algo 12, k_gemm_f32w, the K split auto takes (auto_split)",
                     "gemm_sK": "algo 12 with the split K pinned (a split without whole chunks per slice runs as the next "
                                "smaller one)"}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=("gemv", "gemm", "both"), default="both")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--settle-ms", type=float, default=40.0)
    ap.add_argument("--set-mb", type=int, default=512)
    ap.add_argument("--out-dir", default=None)
    a = ap.parse_args()
    L = ggml_hip.load()
    if L.ggml_hip_device_count() < 1:
        sys.exit("f32w_bench: no HIP device")
    ggml_hip.check(L.ggml_hip_set_device(0))
    ggml_hip.check(L.ggml_hip_set_exact(0))
    s = L.ggml_hip_default_stream()
    out = {"bench": "f32w",
           "timing": "HIP-graph replays over a rotation of weight copies larger than the last-level cache, device events, "
                     "arms interleaved, median / min / max over rounds; algo 12's slab sum included"}
    if a.what in ("gemv", "both"):
        out["gemv"] = gemv(L, s, a)
        print(json.dumps({"gemv": out["gemv"]}), flush=True)
    if a.what in ("gemm", "both"):
        out["gemm"] = gemm(L, s, a)
        print(json.dumps({"gemm": out["gemm"]}), flush=True)
    if a.out_dir:
        os.makedirs(a.out_dir, exist_ok=True)
        with open(os.path.join(a.out_dir, "f32w.json"), "w") as f:
            f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
