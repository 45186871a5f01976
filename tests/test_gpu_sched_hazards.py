"""The hook scheduler's reordering (csrc/ggml-hip-fuse.cpp: held nodes, hoisted sibling mul_mats, chains run in a
GEMV's prologue, held nodes finished in its epilogue, batched elementwise nodes) against ggml's order when buffers
alias.  Each case of tests/sched_model.py is a hand-built node sequence whose ring tensors are placed by the product's
own ggml_hip_assign_buffers on a 64 KiB scratch ring (1 MiB for the 65-row prefill cases; steered with filler
assignments and the ring's wrap, every offset asserted), driven through ggml_hip_compute_forward, and compared byte for byte, the whole ring and every
buffer with an allocation of its own, with the in-order numpy model: with fusion off (which validates the model and
the placement against the path that reorders nothing) and with fusion on, in exact and in fast mode.

A hazard case arranges for one byte-range check to be the only thing between the scheduler and a wrong answer; it
asserts results only (declining the fusion is one right answer, an alias-safe kernel another).  Its twin differs in
the placement of one buffer and also asserts the fused counters of the path, which shows that these hand-built nodes
reach the path the hazard case has denied.  tests/test_sched_model.py shows on the CPU that each hazard is visible in
the result.

In fast mode the model's q4_0 mul_mat is one tensor-free ggml_hip mul_mat on the model's current x (the hook mul_mat
is pinned bitwise to that call elsewhere); in exact mode it is the oracle's.  The prefill cases pin k_gemm9's tile,
without which a group's one launch is not bitwise its members' own launches.

What these cases found in the scheduler, and what csrc/ggml-hip-fuse.cpp does now:
* rope_cpy_strided_span: try_fuse compared nbytes where the group code compares spans, and fused a rope with a copy
  into a strided target that lay on the rope's input (1,932 wrong bytes).  overlaps() compares spans now
  (merge_cb_on_v_span pins the same for the merge copy against the strided V view).
* attn_cb_on_q, attn_cb_on_scaled, attn_kqv_on_q, attn_kqv_on_kq, attn_scaled_on_q: the decode attention launch was
  checked for four overlaps of the merge copy's target only.  What KQV and the copy store is now checked against
  everything the launch reads or stores, and KQ is folded in only when no store lies on K or q.
* attn_inplace_193: with scale / mask / soft_max in place on KQ and KQ run as its own launch, the launch skipped the
  chain's stores (the other workgroups read kq there), so the buffer kept KQ instead of the soft_max.  KQ's launch
  now writes into the stream workspace, the attention launch reads it there and stores the soft_max in place.
* The x image fold that try_fuse turns on again after its alias loop (x9_inplace) and the pointer-only member tests
  of epi_prefix / glu_prefix (qkv_half_view, glu_half_view) gave in-order results: k_row_norm4 works a row per
  workgroup from registers, and both prefixes also compare the element counts."""
import ctypes

import numpy as np
import pytest

import hook_nodes as H
import sched_model as S
from hip_env import ggml_hip, gpu_available

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason="needs a HIP device and libggml_hip.so")]

DB = ggml_hip.DeviceBuffer
GT = {"f32": H.TYPE_F32, "f16": H.TYPE_F16}
OPS = {"add": H.OP_ADD, "mul": H.OP_MUL, "scale": H.OP_SCALE, "silu": H.OP_SILU, "rms_norm": H.OP_RMS_NORM,
       "soft_max": H.OP_SOFT_MAX, "diag_mask_inf": H.OP_DIAG_MASK_INF, "rope": H.OP_ROPE, "mul_mat_f16": H.OP_MUL_MAT}
IDS = [f.__name__ for f in S.CASES]


def device_mul_mat(wq, k, x):
    """the fast-mode model's q4_0 mul_mat: one tensor-free call on this x"""
    m = wq.shape[0]
    wd, xd, yd = DB.from_array(wq), DB.from_array(x), DB(x.shape[0] * m * 4)
    image = x.shape[0] > 64                          # as the hook's prefill: k_gemm9 on the weight's fp6 image
    if image:
        ggml_hip.check(ggml_hip.load().ggml_hip_weight_image_create(wd.ptr, k, m, None), "weight image")
    try:
        ggml_hip.mul_mat(wd, k, m, xd, x.shape[0], yd)
    finally:
        if image:
            ggml_hip.load().ggml_hip_weight_image_free(wd.ptr)
    y = yd.download((x.shape[0], m), np.float32)
    for b in (wd, xd, yd):
        b.free()
    return y


def run_on_device(L, c, fuse):
    """builds c's nodes with its placement, runs them through the hook, returns (memory, fused counters)"""
    g = H.Nodes(L)
    try:
        H.set_fuse(L, fuse)
        g.ring_begin(c.ring_size)
        base = {"ring": g.ring_base}
        own = {}
        for name, init in c.mem.items():
            if name != "ring":
                own[name] = DB.from_array(init)
                base[name] = own[name].ptr
        first, latest = {}, {}                      # model tensor -> its struct as created / as last rewritten

        def realize(t):
            """the struct of an input or view tensor (storage assigned only to ring tensors that are no views)"""
            if id(t) not in first:
                if t.buf == "ring" and not t.view:
                    s = g.ring_place(g.blank(GT[t.typ], t.ne, t.nb), t.off)
                else:
                    s = g.at(base[t.buf] + t.off, GT[t.typ], t.ne, t.nb)
                first[id(t)] = latest[id(t)] = s

        def src(n, t):
            realize(t)
            if c.stale is not None and t is c.stale[1]:
                return first[id(c.nodes[c.stale[0]].out)]           # the rewritten struct's address
            return (first if n.first else latest)[id(t)]

        weights = {k: g.weight_q4_0(*v) for k, v in c.weights.items()}
        structs = []
        for n in c.nodes:
            if n.op == "mul_mat_q4":
                s = g.mm_q4_0(weights[n.src0], src(n, n.src1))
                g.ring_place(s, n.out.off)
            elif n.op == "permute":
                s = g.permute(src(n, n.src0), n.out.ne, n.out.nb)
            elif n.op == "cpy":
                realize(n.out)
                s = g.cpy_node(src(n, n.src0), first[id(n.out)])
                structs.append(s)
                continue                                           # (a view of its target: the target stays what it was)
            else:
                s0 = src(n, n.src0)
                if n.op == "scale":
                    s1 = g.host(np.array([n.p], np.float32), H.TYPE_F32)
                elif n.op == "diag_mask_inf":
                    s1 = g.host(np.array([n.p, int(n.inplace())], np.int32), H.TYPE_I32)
                elif n.op == "rope":
                    s1 = g.host(np.array([n.p[0], n.p[1], 0], np.int32), H.TYPE_I32)
                else:
                    s1 = src(n, n.src1) if n.src1 is not None else None
                s = g.op_tensor(OPS[n.op], n.out.ne, s0, s1, n.inplace())
                if n.inplace():
                    g.assign_inplace(s)
                else:
                    assert n.out.buf == "ring" and not n.out.view
                    g.ring_place(s, n.out.off)
            first.setdefault(id(n.out), s)
            latest[id(n.out)] = s
            structs.append(s)
        g.upload(g.ring_base, c.mem["ring"])                        # after the last assignment, before the first node
        H.op_stats(L)
        rewritten = None
        for i, s in enumerate(structs):
            g.forward(s)
            if c.stale is not None and i == c.stale[0]:
                z = first[id(c.stale[1])]
                rewritten = (s, ctypes.string_at(ctypes.addressof(s), ctypes.sizeof(s)))
                ctypes.memmove(ctypes.addressof(s), ctypes.addressof(z), ctypes.sizeof(s))
        mem = {"ring": g.download(g.ring_base, c.ring_size)}            # (the read flushes what is held)
        if rewritten:                                              # the struct as it was, for close()
            ctypes.memmove(ctypes.addressof(rewritten[0]), rewritten[1], len(rewritten[1]))
        for name, b in own.items():
            mem[name] = b.download((b.nbytes,), np.uint8)
        fused = H.op_stats(L)[1]
        for b in own.values():
            b.free()
        return mem, fused
    finally:
        g.close()


@pytest.fixture(scope="module")
def lib():
    L = ggml_hip.load()
    with H.restore_switches(L):
        yield L


def assert_memory(got, ref, what):
    for name in ref:
        bad = np.flatnonzero(got[name] != ref[name])
        assert bad.size == 0, (what, name, bad.size, bad[:8], got[name][bad[:8]], ref[name][bad[:8]])


@pytest.mark.parametrize("mode", ["exact", "fast"])
@pytest.mark.parametrize("case", S.CASES, ids=IDS)
def test_in_order_results(lib, case, mode):
    c = case()
    ggml_hip.check(lib.ggml_hip_set_exact(1 if mode == "exact" else 0), "set_exact")
    lib.ggml_hip_debug_set_gemm9_wide.argtypes = [ctypes.c_int]
    if c.gemm9_tile is not None:
        ggml_hip.check(lib.ggml_hip_debug_set_gemm9_wide(c.gemm9_tile), "gemm9 tile")
    try:
        ref = c.run(mm=S.exact_mul_mat if mode == "exact" else device_mul_mat)
        got, _ = run_on_device(lib, c, 0)
        assert_memory(got, ref, "fuse off")
        got, fused = run_on_device(lib, c, 1)
    finally:
        lib.ggml_hip_debug_set_gemm9_wide(-1)
    print(c.name, mode, "fused", fused.tolist())
    assert_memory(got, ref, "fuse on")
    for slot in c.fused[mode]:
        assert fused[slot] >= 1, (slot, fused)
