#!/usr/bin/env python3
"""Q3_K / Q2_K prefill on the LLaMA-7B layer shapes (4096 -> 4096, 4096 -> 11008, 11008 -> 4096): the column-tiled
GEMV (algo 1, the prefill path before the GEMM existed and still the default) against the int8-MFMA GEMM (algo 8)
over N = 9 .. 512, in one process.

Weights: a rotation of distinct device buffers whose total exceeds --rotate-mb (default 320 MB, above the 256 MB
of last-level cache), so that every call reads its matrix from memory as a layer of a prefill does; call i of a
graph takes buffer i mod R.  For every N each arm is captured as a HIP graph of one pass over the rotation (the GEMM
arm includes its q8_K quantization of x, which the GEMV fuses); after both graphs have been replayed for
--settle-ms of device time the graphs are replayed alternately for --rounds rounds, each replay timed by device
events.  One JSON line: per type, shape and N the microseconds per call (median, min, max over the rounds) of both
arms, TOP/s for 2 M K N and the ratio GEMV / GEMM with its worst case over the rounds (GEMV min / GEMM max);
`min_n` is the smallest swept N from which the GEMM wins on every shape of both types at that N and every larger
one, a win being a worst-case ratio above 1, so by more than the spread (the value to give
GGML_HIP_Q23K_GEMM_MIN_N; null: it never does).  Both arms are checked bitwise equal before they are timed.  Fails
without a HIP device.

    python tools/q23k_gemm_bench.py [--rounds 10] [--out profiles/q23k_gemm.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "llama.cpp-q_4_0_amd", "python"))
import ggml_hip  # noqa: E402

NS = (9, 16, 32, 64, 128, 256, 512)
SHAPES = ((4096, 4096), (4096, 11008), (11008, 4096))      # (K, M)
ARMS = (("gemv", 1), ("gemm", 8))
# name: (block bytes, offsets of the fp16 fields, binding)
TYPES = {
    "q3_K": (110, (108,), "mul_mat_q3_K"),
    "q2_K": (84, (80, 82), "mul_mat_q2_K"),
}


def random_rows(rng, M, K, bs, halves):
    w = rng.integers(0, 256, size=(M * (K // 256), bs), dtype=np.uint8)
    for off in halves:                                         # finite fp16 fields in every block
        w[:, off:off + 2] = np.array([0.01], np.float16).view(np.uint8)
    return w


def sweep_one(L, a, name, K, M, s, e0, e1):
    bs, halves, binding = TYPES[name]
    mm = getattr(ggml_hip, binding)
    rng = np.random.default_rng([0x23, bs, K, M])
    w = random_rows(rng, M, K, bs, halves)
    R = max(2, -(-int(a.rotate_mb * 1e6) // w.nbytes))
    wds = [ggml_hip.DeviceBuffer.from_array(w) for _ in range(R)]
    x = rng.standard_normal((max(NS), K)).astype(np.float32)
    xd = ggml_hip.DeviceBuffer.from_array(x)
    yd = {arm: ggml_hip.DeviceBuffer(max(NS) * M * 4) for arm, _ in ARMS}
    ggml_hip.check(L.ggml_hip_reserve_workspace(K, max(NS)))
    rows = []
    for N in NS:
        graphs = {}
        for arm, algo in ARMS:
            def fn(i, arm=arm, algo=algo):
                mm(wds[i % R], K, M, xd, N, yd[arm], algo=algo, stream=s)
            fn(0)                                              # code objects loaded, attributes set
            ggml_hip.check(L.ggml_hip_stream_synchronize(s))
            g = ggml_hip.Graph(s)
            with g:
                for i in range(R):
                    fn(i)
            graphs[arm] = g
        ys = [yd[arm].download((N, M), np.uint32) for arm, _ in ARMS]
        if not np.array_equal(ys[0], ys[1]):
            sys.exit(f"q23k_gemm_bench: {name} algo 8 differs from algo 1 at K = {K}, M = {M}, N = {N}")
        e0.record(s)
        while True:                                            # settle: at least --settle-ms of back-to-back load
            for g in graphs.values():
                g.launch()
            e1.record(s)
            if e0.elapsed_ms(e1) >= a.settle_ms:
                break
        us = {arm: [] for arm in graphs}
        for _ in range(a.rounds):
            for arm, g in graphs.items():
                e0.record(s)
                g.launch()
                e1.record(s)
                ms = e0.elapsed_ms(e1)
                if ms < 0:
                    sys.exit("q23k_gemm_bench: event timing failed")
                us[arm].append(ms * 1e3 / R)
        row = {"N": N}
        for arm in graphs:
            med = float(np.median(us[arm]))
            row.update({f"{arm}_us": round(med, 2), f"{arm}_us_min": round(min(us[arm]), 2),
                        f"{arm}_us_max": round(max(us[arm]), 2), f"{arm}_TOPs": round(2.0 * M * K * N / med * 1e-6, 1)})
        row["gemv_over_gemm"] = round(row["gemv_us"] / row["gemm_us"], 3)
        row["gemv_over_gemm_worst"] = round(row["gemv_us_min"] / row["gemm_us_max"], 3)
        rows.append(row)
    for b in wds + [xd] + list(yd.values()):
        b.free()
    return {"type": name, "K": K, "M": M, "weight_bytes": int(w.nbytes), "rotation": R, "sweep": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--rotate-mb", type=float, default=320.0)
    ap.add_argument("--settle-ms", type=float, default=40.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L = ggml_hip.load()
    if L.ggml_hip_device_count() < 1:
        sys.exit("q23k_gemm_bench: no HIP device")
    ggml_hip.check(L.ggml_hip_set_device(0))
    ggml_hip.check(L.ggml_hip_set_exact(0))
    s = L.ggml_hip_default_stream()
    e0, e1 = ggml_hip.Event(), ggml_hip.Event()
    results = [sweep_one(L, a, name, K, M, s, e0, e1) for name in TYPES for K, M in SHAPES]
    min_n = None
    for i in reversed(range(len(NS))):
        if any(r["sweep"][i]["gemv_over_gemm_worst"] <= 1.0 for r in results):
            break
        min_n = NS[i]
    line = json.dumps({"bench": "q23k_gemm", "rounds": a.rounds, "rotate_mb": a.rotate_mb, "settle_ms": a.settle_ms,
                       "results": results, "min_n": min_n,
                       "timing": "HIP-graph replays over a rotation of weight buffers larger than the last-level "
                                 "cache, device events, arms interleaved, median / min / max over rounds"})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
