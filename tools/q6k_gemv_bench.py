#!/usr/bin/env python3
"""Time of the Q6_K lm_head GEMV launch (M = 32000, K = 4096, N = 1; 107.5 MB of weights) beside the q4_0 GEMV at
equal weight bytes (K = 4096, M = 46656), in one process.

Each kernel is captured as a HIP graph of --launches back-to-back launches on the same operands; after a warm-up
the two graphs are replayed alternately for --rounds rounds, each replay timed by device events.  One JSON line:
the median microseconds per launch and the achieved weight bytes per second (the bytes the algorithm must read,
from the shapes) for both, and their ratio.  The replays are warm: both weight sets together are below the 256 MB
of last-level cache, so the rates are launch rates on repeated operands, not cold HBM reads; the comparison holds
because both kernels run under the same conditions.  Fails without a HIP device.

    python tools/q6k_gemv_bench.py [--rounds 30] [--launches 200] [--out profiles/q6k_gemv.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "llama.cpp-q_4_0_amd", "python"))
import ggml_hip  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L = ggml_hip.load()
    if L.ggml_hip_device_count() < 1:
        sys.exit("q6k_gemv_bench: no HIP device")
    ggml_hip.check(L.ggml_hip_set_device(0))
    ggml_hip.check(L.ggml_hip_set_exact(0))
    K, M6, M4 = 4096, 32000, 46656
    rng = np.random.default_rng(0x6B)
    w6 = rng.integers(0, 256, size=(M6 * (K // 256), 210), dtype=np.uint8)
    w6[:, 208:210] = np.array([0.01], np.float16).view(np.uint8)          # a finite d in every block
    w4 = rng.integers(0, 256, size=(M4 * (K // 32), 18), dtype=np.uint8)
    w4[:, 0:2] = np.array([0.01], np.float16).view(np.uint8)
    x = rng.standard_normal((1, K)).astype(np.float32)
    w6d, w4d, xd = (ggml_hip.DeviceBuffer.from_array(v) for v in (w6, w4, x))
    y6d, y4d = ggml_hip.DeviceBuffer(M6 * 4), ggml_hip.DeviceBuffer(M4 * 4)
    s = L.ggml_hip_default_stream()

    def q6():
        ggml_hip.mul_mat_q6_K(w6d, K, M6, xd, 1, y6d, algo=1, stream=s)

    def q4():
        ggml_hip.mul_mat(w4d, K, M4, xd, 1, y4d, algo=1, stream=s)

    graphs = {}
    for name, fn in (("q6_K", q6), ("q4_0", q4)):
        fn()                                                   # code objects loaded, attributes set
        ggml_hip.check(L.ggml_hip_stream_synchronize(s))
        g = ggml_hip.Graph(s)
        with g:
            for _ in range(a.launches):
                fn()
        graphs[name] = g
    for _ in range(3):
        for g in graphs.values():
            g.launch()
    ggml_hip.check(L.ggml_hip_stream_synchronize(s))
    us = {name: [] for name in graphs}
    e0, e1 = ggml_hip.Event(), ggml_hip.Event()
    for _ in range(a.rounds):
        for name, g in graphs.items():
            e0.record(s)
            g.launch()
            e1.record(s)
            ms = e0.elapsed_ms(e1)
            if ms < 0:
                sys.exit("q6k_gemv_bench: event timing failed")
            us[name].append(ms * 1e3 / a.launches)
    bytes6, bytes4 = M6 * (K // 256) * 210, M4 * (K // 32) * 18
    m6, m4 = float(np.median(us["q6_K"])), float(np.median(us["q4_0"]))
    line = json.dumps({
        "bench": "q6k_gemv", "K": K, "N": 1, "q6_K_M": M6, "q4_0_M": M4, "q6_K_weight_bytes": bytes6,
        "q4_0_weight_bytes": bytes4, "launches_per_graph": a.launches, "rounds": a.rounds,
        "q6_K_us_per_launch": round(m6, 3), "q6_K_us_min": round(min(us["q6_K"]), 3), "q6_K_us_max": round(max(us["q6_K"]), 3),
        "q6_K_warm_TBps": round(bytes6 / m6 * 1e-6, 3),
        "q4_0_us_per_launch": round(m4, 3), "q4_0_us_min": round(min(us["q4_0"]), 3), "q4_0_us_max": round(max(us["q4_0"]), 3),
        "q4_0_warm_TBps": round(bytes4 / m4 * 1e-6, 3),
        "q6_K_over_q4_0": round(m6 / m4, 3), "timing": "warm HIP-graph replays, device events, median over rounds"})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
