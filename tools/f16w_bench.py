#!/usr/bin/env python3
"""F16 weights on the device: the decode GEMV (csrc/f16_w.hip) against the kernels an F16 weight's node ran on before
it existed, and the prefill crossover between the column-tiled GEMV, the tiled bitwise kernel and the MFMA kernel, in
one process.

Decode (profiles/f16w_gemv.json).  N = 1, 4 and 8 on the LLaMA-7B shapes 4096 -> 4096, 4096 -> 11008, 11008 -> 4096
and the lm_head 4096 -> 32000.  Two arms through ggml_hip_mul_mat_f16 on the same F16 matrix: algo 1 (k_gemv_f16w) and
algo 4, which is op_mul_mat_f16_f32's own choice among the bitwise kernels: k_mul_mat_f16_f32 (32 lanes per output,
what ggml_hip_debug_f16_mul_mat runs with tiled = 0) below 8 columns, the LDS-tiled kernel from 8, exactly what an
F16 src0 ran on at these N outside exact mode before.  Each arm launches over a ROTATION of distinct copies of the
matrix whose total exceeds --set-mb (default 512 MB, twice the 256 MB last-level cache), so every launch streams its
weights from HBM.  One rotation is one HIP graph; after --settle-ms of load the arms' graphs are replayed alternately
for --rounds rounds, each replay timed by device events.  Reported per shape, N and arm: microseconds per call (median,
min, max over rounds), TB/s of weight bytes and the fraction of 8 TB/s, and old / new.

Prefill (profiles/f16w_gemm.json).  The three layer shapes, N = 9 .. 512: algo 1 (GEMV column tiles), algo 4 (the
tiled bitwise kernel) and algo 9 (k_mul_mat_f16_f32_mfma), over the same rotation.  `min_n` per shape is the
smallest swept N from which the MFMA arm beats the GEMV arm at every larger swept N (the value for the default of
f16w_gemm_min_n); null if it never does.  The arms are checked against each other within 1e-3 of the largest |y|
before they are timed.  Fails without a HIP device.

Weight-shaped GEMM (profiles/f16w_wgemm.json; --what wgemm).  The three layer shapes and the lm_head, N = 9 .. 512, over
the same rotation, graphs and alternation: algo 1 (GEMV column tiles), algo 9 (k_mul_mat_f16_f32_mfma) and algo 11
(k_gemm_f16w, csrc/f16_w_gemm.hip) with the plan auto takes, and algo 11 under each pinned plan (the per-plan sweep the
plan rule is held against).  Per cell and arm: median, min and max over rounds; for algo 11 the fraction of the
derived floor max(weight bytes / 8 TB/s, 2 K M N / 2.5 PF).  algo 11 WINS a cell where its median is below both other
arms' and its max below their min (the spreads do not overlap).  `recommended_min_n` is the smallest swept N from which
it wins every cell of every layer shape; null if there is none.

    python tools/f16w_bench.py [--what decode|prefill|wgemm|both] [--rounds 10] [--out-dir profiles]
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
DECODE_SHAPES = LAYER_SHAPES + ((4096, 32000),)
DECODE_NS = (1, 4, 8)
SWEEP_NS = (9, 16, 32, 64, 128, 512)
HBM_TBS = 8.0
MFMA_PFS = 2.5
WGEMM_PLANS = (1, 2, 3)
DB = ggml_hip.DeviceBuffer
ARMS = {"gemv": 1, "bitwise": 4, "mfma": 9}


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


def rotation(rng, K, M, set_mb):
    """(device buffer of `copies` distinct F16 matrices [M][K] of 0.02 N(0, 1), bytes of one, copies)"""
    mat = M * K * 2
    copies = max(2, -(-set_mb * (1 << 20) // mat))
    chunk = (rng.standard_normal(1 << 22) * 0.02).astype(np.float16).view(np.uint16)
    host = np.tile(chunk, -(-copies * M * K // chunk.size))[:copies * M * K]
    return DB.from_array(host), mat, copies


def arm_graphs(L, s, wd, mat, copies, K, M, xd, N, yd, arms):
    graphs, per_graph = {}, {}
    for name in arms:
        def fn(i, name=name):
            ggml_hip.mul_mat_f16(wd, K, M, xd, N, yd[name], algo=ARMS[name], stream=s, w_off=i * mat)
        fn(0)                                                  # code objects loaded
        ggml_hip.check(L.ggml_hip_stream_synchronize(s))
        g = ggml_hip.Graph(s)
        with g:
            for i in range(copies):
                fn(i)
        graphs[name], per_graph[name] = g, copies
    return graphs, per_graph


def check_arms(L, s, wd, K, M, xd, N, yd, arms, who):
    ys = {}
    for name in arms:
        ggml_hip.mul_mat_f16(wd, K, M, xd, N, yd[name], algo=ARMS[name], stream=s)
        ggml_hip.check(L.ggml_hip_stream_synchronize(s))
        ys[name] = yd[name].download((N, M), np.float32)
    first = ys[arms[0]]
    for name in arms[1:]:
        if not np.abs(ys[name] - first).max() <= 1e-3 * np.abs(first).max():
            sys.exit(f"{who}: arm {name} differs from {arms[0]} at K = {K}, M = {M}, N = {N}")


def decode(L, s, a):
    rng = np.random.default_rng(0xF16D)
    arms = ("gemv", "bitwise")
    rows = []
    for K, M in DECODE_SHAPES:
        wd, mat, copies = rotation(rng, K, M, a.set_mb)
        xd = DB.from_array(rng.standard_normal((max(DECODE_NS), K)).astype(np.float32))
        yd = {name: DB(max(DECODE_NS) * M * 4) for name in arms}
        for N in DECODE_NS:
            check_arms(L, s, wd, K, M, xd, N, yd, arms, "f16w_bench decode")
            graphs, per_graph = arm_graphs(L, s, wd, mat, copies, K, M, xd, N, yd, arms)
            us = timed_rounds(L, s, graphs, a.rounds, a.settle_ms, per_graph, "f16w_bench decode")
            row = {"K": K, "M": M, "N": N, "weight_bytes": mat, "copies": copies}
            for name in arms:
                st = stats(us[name])
                tbs = mat / st["us"] * 1e-6
                row[name] = dict(st, TBs=round(tbs, 3), frac_hbm=round(tbs / HBM_TBS, 3))
            row["bitwise_over_gemv_us"] = round(row["bitwise"]["us"] / row["gemv"]["us"], 2)
            rows.append(row)
            del graphs
        for b in [wd, xd] + list(yd.values()):
            b.free()
    return {"bench": "f16w_gemv", "set_mb": a.set_mb, "rounds": a.rounds, "settle_ms": a.settle_ms, "hbm_TBs": HBM_TBS,
            "nt_weight_loads": os.environ.get("GGML_HIP_F16W_NT", "1") != "0", "rows": rows,
            "gemv_faster_everywhere": all(r["bitwise_over_gemv_us"] > 1.0 for r in rows),
            "arms": {"gemv": "ggml_hip_mul_mat_f16 algo 1 (k_gemv_f16w; K = 11008 takes 5 columns per launch, so N = 8 "
                             "is two launches)",
                     "bitwise": "ggml_hip_mul_mat_f16 algo 4 (k_mul_mat_f16_f32 for N < 8, k_mul_mat_f16_f32_tiled at 8)"},
            "timing": "HIP-graph replays over a rotation of weight copies larger than the last-level cache, device "
                      "events, arms interleaved, median over rounds"}


def prefill(L, s, a):
    rng = np.random.default_rng(0xF16E)
    arms = ("gemv", "bitwise", "mfma")
    shapes = []
    for K, M in LAYER_SHAPES:
        wd, mat, copies = rotation(rng, K, M, a.set_mb)
        xd = DB.from_array(rng.standard_normal((max(SWEEP_NS), K)).astype(np.float32))
        yd = {name: DB(max(SWEEP_NS) * M * 4) for name in arms}
        sweep = []
        for N in SWEEP_NS:
            check_arms(L, s, wd, K, M, xd, N, yd, arms, "f16w_bench prefill")
            graphs, per_graph = arm_graphs(L, s, wd, mat, copies, K, M, xd, N, yd, arms)
            us = timed_rounds(L, s, graphs, a.rounds, a.settle_ms, per_graph, "f16w_bench prefill")
            row = {"N": N}
            for name in arms:
                st = stats(us[name])
                row.update({f"{name}_{k}": v for k, v in st.items()})
                row[f"{name}_TFLOPs"] = round(2.0 * M * K * N / st["us"] * 1e-6, 1)
            row["gemv_over_mfma"] = round(row["gemv_us"] / row["mfma_us"], 3)
            sweep.append(row)
            del graphs
        min_n = None
        for row in reversed(sweep):
            if row["gemv_over_mfma"] <= 1.0:
                break
            min_n = row["N"]
        shapes.append({"K": K, "M": M, "weight_bytes": mat, "copies": copies, "sweep": sweep, "min_n": min_n})
        for b in [wd, xd] + list(yd.values()):
            b.free()
    return {"bench": "f16w_gemm", "set_mb": a.set_mb, "rounds": a.rounds, "settle_ms": a.settle_ms, "shapes": shapes,
            "arms": {"gemv": "algo 1, column tiles of gemv_f16w_max_tokens(K)", "bitwise": "algo 4, k_mul_mat_f16_f32_tiled",
                     "mfma": "algo 9, k_mul_mat_f16_f32_mfma"},
            "timing": "HIP-graph replays over a rotation of weight copies larger than the last-level cache, device "
                      "events, arms interleaved, median over rounds"}


def wgemm(L, s, a):
    rng = np.random.default_rng(0xF16F)
    pin = L.ggml_hip_debug_set_f16w_wgemm_plan
    # arm -> (algo, pinned plan; 0 auto)
    arms = {"gemv": (1, 0), "mfma": (9, 0), "wgemm": (11, 0)}
    arms.update({f"wgemm_p{p}": (11, p) for p in WGEMM_PLANS})
    shapes = []
    for K, M in DECODE_SHAPES:
        wd, mat, copies = rotation(rng, K, M, a.set_mb)
        nmax = max(SWEEP_NS)
        xd = DB.from_array(rng.standard_normal((nmax, K)).astype(np.float32))
        yd = {name: DB(nmax * M * 4) for name in arms}
        for p in WGEMM_PLANS:                                  # the workspace of every plan, ahead of the captures
            pin(p)
            ggml_hip.check(L.ggml_hip_reserve_workspace_mm(K, nmax, M), "reserve")
        pin(0)
        sweep = []
        for N in SWEEP_NS:
            def call(name, i):
                algo, plan = arms[name]
                pin(plan)
                ggml_hip.mul_mat_f16(wd, K, M, xd, N, yd[name], algo=algo, stream=s, w_off=i * mat)
                pin(0)
            ys = {}
            for name in arms:
                call(name, 0)
                ggml_hip.check(L.ggml_hip_stream_synchronize(s))
                ys[name] = yd[name].download((N, M), np.float32)
                if not np.abs(ys[name] - ys["gemv"]).max() <= 1e-3 * np.abs(ys["gemv"]).max():
                    sys.exit(f"f16w_bench wgemm: arm {name} differs from gemv at K = {K}, M = {M}, N = {N}")
            graphs, per_graph = {}, {}
            for name in arms:
                g = ggml_hip.Graph(s)
                with g:
                    for i in range(copies):
                        call(name, i)
                graphs[name], per_graph[name] = g, copies
            us = timed_rounds(L, s, graphs, a.rounds, a.settle_ms, per_graph, "f16w_bench wgemm")
            floor = max(mat / (HBM_TBS * 1e12), 2.0 * K * M * N / (MFMA_PFS * 1e15)) * 1e6
            row = {"N": N, "floor_us": round(floor, 2), "auto_plan": L.ggml_hip_debug_f16w_wgemm_plan(K, M, N)}
            for name in arms:
                row.update({f"{name}_{k}": v for k, v in stats(us[name]).items()})
            row["wgemm_floor_frac"] = round(floor / row["wgemm_us"], 3)
            row["wgemm_wins"] = all(row["wgemm_us"] < row[f"{o}_us"] and row["wgemm_us_max"] < row[f"{o}_us_min"]
                                    for o in ("gemv", "mfma"))
            best = min(WGEMM_PLANS, key=lambda p: row[f"wgemm_p{p}_us"])
            row["best_plan"] = best
            row["auto_plan_over_best"] = round(row[f"wgemm_p{row['auto_plan']}_us"] / row[f"wgemm_p{best}_us"], 3)
            sweep.append(row)
            del graphs
        shapes.append({"K": K, "M": M, "weight_bytes": mat, "copies": copies, "sweep": sweep})
        for b in [wd, xd] + list(yd.values()):
            b.free()
    rec = None
    layer = [sh for sh in shapes if (sh["K"], sh["M"]) in LAYER_SHAPES]
    for i in reversed(range(len(SWEEP_NS))):
        if not all(sh["sweep"][i]["wgemm_wins"] for sh in layer):
            break
        rec = SWEEP_NS[i]
    wins = {n: all(sh["sweep"][SWEEP_NS.index(n)]["wgemm_wins"] for sh in layer) for n in (64, 512)}
    return {"bench": "f16w_wgemm", "set_mb": a.set_mb, "rounds": a.rounds, "settle_ms": a.settle_ms, "hbm_TBs": HBM_TBS,
            "mfma_PFs": MFMA_PFS, "shapes": shapes, "recommended_min_n": rec,
            "wins_on_every_layer_shape_at_64_and_512": wins,
            "arms": {"gemv": "algo 1, column tiles of gemv_f16w_max_tokens(K)", "mfma": "algo 9, k_mul_mat_f16_f32_mfma",
                     "wgemm": "algo 11, k_gemm_f16w, the plan auto takes (auto_plan)",
                     "wgemm_pK": "algo 11 with plan K pinned: 1 = 32 x 64 tiles, K split over the waves and 4 workgroups; "
                                 "2 = 64 x 128, K split 2; 3 = 128 x 128, no split"},
            "timing": "HIP-graph replays over a rotation of weight copies larger than the last-level cache, device "
                      "events, arms interleaved, median / min / max over rounds; algo 11's x image and slab sum included"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=("decode", "prefill", "wgemm", "both"), default="both")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--settle-ms", type=float, default=40.0)
    ap.add_argument("--set-mb", type=int, default=512)
    ap.add_argument("--out-dir", default=None)
    a = ap.parse_args()
    L = ggml_hip.load()
    if L.ggml_hip_device_count() < 1:
        sys.exit("f16w_bench: no HIP device")
    ggml_hip.check(L.ggml_hip_set_device(0))
    ggml_hip.check(L.ggml_hip_set_exact(0))
    s = L.ggml_hip_default_stream()
    for what, fn, out in (("decode", decode, "f16w_gemv.json"), ("prefill", prefill, "f16w_gemm.json"),
                          ("wgemm", wgemm, "f16w_wgemm.json")):
        if a.what != what and (a.what != "both" or what == "wgemm"):
            continue
        line = json.dumps(fn(L, s, a))
        print(line, flush=True)
        if a.out_dir:
            os.makedirs(a.out_dir, exist_ok=True)
            with open(os.path.join(a.out_dir, out), "w") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
