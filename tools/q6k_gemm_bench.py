#!/usr/bin/env python3
"""Q6_K lm_head prefill (M = 32000, K = 4096): the column-tiled GEMV (algo 1) against the int8-MFMA GEMM (algo 5)
over N = 9 .. 512, in one process.

For every N each arm is captured as a HIP graph of --launches back-to-back ggml_hip_mul_mat_q6_K calls on the same
operands (the GEMM arm includes its q8_K quantization of x, which the GEMV fuses); after both graphs have been
replayed for --settle-ms of device time (the clocks need about 25 ms of load) the two graphs are replayed
alternately for --rounds rounds, each replay timed by device events.  One JSON line: per N the microseconds per call (median, min, max) of both arms,
TOP/s for 2 M K N, and the ratio GEMV / GEMM; `min_n` is the smallest swept N from which the GEMM wins at every
larger N (the value for q6k_gemm_min_n).  The replays are warm: the 107.5 MB of weights stay below the 256 MB of
last-level cache.  Both arms are checked bitwise equal before they are timed.  Fails without a HIP device.

    python tools/q6k_gemm_bench.py [--rounds 10] [--launches 10] [--out profiles/q6k_gemm.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--settle-ms", type=float, default=40.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L = ggml_hip.load()
    if L.ggml_hip_device_count() < 1:
        sys.exit("q6k_gemm_bench: no HIP device")
    ggml_hip.check(L.ggml_hip_set_device(0))
    ggml_hip.check(L.ggml_hip_set_exact(0))
    K, M = 4096, 32000
    rng = np.random.default_rng(0x6D)
    w = rng.integers(0, 256, size=(M * (K // 256), 210), dtype=np.uint8)
    w[:, 208:210] = np.array([0.01], np.float16).view(np.uint8)           # a finite d in every block
    x = rng.standard_normal((max(NS), K)).astype(np.float32)
    wd, xd = ggml_hip.DeviceBuffer.from_array(w), ggml_hip.DeviceBuffer.from_array(x)
    yd = {algo: ggml_hip.DeviceBuffer(max(NS) * M * 4) for algo in (1, 5)}
    s = L.ggml_hip_default_stream()
    ggml_hip.check(L.ggml_hip_reserve_workspace(K, max(NS)))
    e0, e1 = ggml_hip.Event(), ggml_hip.Event()
    sweep = []
    for N in NS:
        graphs = {}
        for algo in (1, 5):
            def fn(algo=algo):
                ggml_hip.mul_mat_q6_K(wd, K, M, xd, N, yd[algo], algo=algo, stream=s)
            fn()                                               # code objects loaded, attributes set
            ggml_hip.check(L.ggml_hip_stream_synchronize(s))
            g = ggml_hip.Graph(s)
            with g:
                for _ in range(a.launches):
                    fn()
            graphs[algo] = g
        if not np.array_equal(yd[1].download((N, M), np.uint32), yd[5].download((N, M), np.uint32)):
            sys.exit(f"q6k_gemm_bench: algo 5 differs from algo 1 at N = {N}")
        e0.record(s)
        while True:                                            # settle: at least --settle-ms of back-to-back load
            for g in graphs.values():
                g.launch()
            e1.record(s)
            if e0.elapsed_ms(e1) >= a.settle_ms:
                break
        us = {algo: [] for algo in graphs}
        for _ in range(a.rounds):
            for algo, g in graphs.items():
                e0.record(s)
                g.launch()
                e1.record(s)
                ms = e0.elapsed_ms(e1)
                if ms < 0:
                    sys.exit("q6k_gemm_bench: event timing failed")
                us[algo].append(ms * 1e3 / a.launches)
        row = {"N": N}
        for algo, name in ((1, "gemv"), (5, "gemm")):
            med = float(np.median(us[algo]))
            row.update({f"{name}_us": round(med, 2), f"{name}_us_min": round(min(us[algo]), 2),
                        f"{name}_us_max": round(max(us[algo]), 2), f"{name}_TOPs": round(2.0 * M * K * N / med * 1e-6, 1)})
        row["gemv_over_gemm"] = round(row["gemv_us"] / row["gemm_us"], 3)
        sweep.append(row)
    min_n = None
    for row in reversed(sweep):
        if row["gemv_over_gemm"] <= 1.0:
            break
        min_n = row["N"]
    line = json.dumps({"bench": "q6k_gemm", "K": K, "M": M, "weight_bytes": M * (K // 256) * 210,
                       "launches_per_graph": a.launches, "rounds": a.rounds, "settle_ms": a.settle_ms,
                       "sweep": sweep, "min_n": min_n,
                       "timing": "warm HIP-graph replays, device events, arms interleaved, median over rounds"})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
