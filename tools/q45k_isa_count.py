#!/usr/bin/env python3
"""Instruction counts of the Q5_K / Q4_K GEMV's main loop (profiles/q45k_gemv_isa.json), from the compiler's
assembly of csrc/q45_k.hip for gfx950 with the Makefile's kernel flags.  Needs hipcc, no device.

For k_gemv_q45_K<QH, 1> (QH = 1 Q5_K, 0 Q4_K) the main loop is the kernel's last innermost loop: one trip is one
batch of GEMV45_UNROLL steps of two superblocks.  Reported per kernel: instructions per trip by class (vector ALU,
those of them with a DPP modifier, LDS, scalar, global memory) and instructions per superblock.

    python tools/q45k_isa_count.py [--out-dir profiles]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "llama.cpp-q_4_0_amd")
FLAGS = ["-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "--offload-arch=gfx950", "-I../include", "-mllvm",
         "-amdgpu-kernarg-preload-count=16", "-fno-slp-vectorize", "--offload-device-only", "-S"]


def kernel_lines(asm, qh):
    name = f"_ZN4ghip12k_gemv_q45_KILb{qh}ELi1EEEvPKhiiPKfPfl:"
    out, on = [], False
    for line in asm:
        if line.startswith(name):
            on = True
        if on:
            out.append(line)
            if "s_endpgm" in line:
                break
    if not out:
        sys.exit(f"q45k_isa_count: {name} not found")
    return out


def count(lines):
    heads = [i for i, l in enumerate(lines) if "Inner Loop Header" in l]
    start = heads[-1]
    end = max(i for i, l in enumerate(lines) if "s_cbranch" in l and i > start)
    body = [l.strip() for l in lines[start:end + 1] if l.startswith("\t") and not l.strip().startswith((";", "."))]
    op = [l.split()[0] for l in body]
    return {"per_trip": len(body), "valu": sum(o.startswith("v_") for o in op),
            "valu_dpp": sum(bool(re.search(r"\b(quad_perm|row_\w+):", l)) for l in body),
            "lds": sum(o.startswith("ds_") for o in op), "salu": sum(o.startswith("s_") for o in op),
            "vmem": sum(o.startswith(("global_", "buffer_", "flat_")) for o in op)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=None)
    ap.add_argument("--hipcc", default=os.path.join(os.environ.get("ROCM", "/opt/rocm"), "bin", "hipcc"))
    a = ap.parse_args()
    src = open(os.path.join(PKG, "csrc", "q45_k.hip")).read()
    unroll = int(re.search(r"GEMV45_UNROLL = (\d+);", src).group(1))
    with tempfile.TemporaryDirectory() as tmp:
        s = os.path.join(tmp, "q45_k.s")
        subprocess.check_call([a.hipcc, *FLAGS, "csrc/q45_k.hip", "-o", s], cwd=PKG, stderr=subprocess.DEVNULL)
        asm = open(s).read().split("\n")
    res = {"bench": "q45k_gemv_isa", "superblocks_per_trip": 2 * unroll}
    for name, qh in (("q5_K", 1), ("q4_K", 0)):
        c = count(kernel_lines(asm, qh))
        c["per_superblock"] = round(c["per_trip"] / (2 * unroll), 1)
        res[name] = c
    line = json.dumps(res)
    print(line)
    if a.out_dir:
        with open(os.path.join(a.out_dir, "q45k_gemv_isa.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
