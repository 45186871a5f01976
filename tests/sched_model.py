"""What ggml's order means for a node sequence whose buffers are placed explicitly and may alias: a small numpy
interpreter (no device), and the adversarial sequences the hook scheduler's tests run (tests/test_sched_model.py on
the CPU, tests/test_gpu_sched_hazards.py on the device).

Memory is a dict of named byte buffers: "ring" (the VRAM scratch ring ggml_hip_assign_buffers places node outputs
in) and every buffer with an allocation of its own.  A tensor (T) is (buffer, byte offset, type, ne, nb).  run()
executes the nodes strictly in the order given: each node reads its operands from the memory as it is at that
moment and writes its output back.  The ops are the project's pinned restatements (tests/ggml_ops_ref.py; the q4_0
mul_mat is oracle.mul_mat, or a callback that runs the device GEMV on the model's current x: the subject here is
order, the GEMV's numerics are pinned elsewhere).

A Case also carries `wrong`: the node sequence a scheduler without the hazard check under test would in effect
compute (a hoisted mul_mat, a chain run again after its input was overwritten, ...).  The CPU test asserts that it
changes at least one bit of the memory, so the device comparison can tell the two apart.

Two placements cannot be expressed without a node that overlaps its own operand, which is undefined even in order, so
only their twins are here: a sibling mul_mat whose y lies on x (group_join_ok's m against g.mm[i]->src1: a sibling
reads that same x, same_tensor(m->src1, g.mm[0]->src1) is the entry condition), and a norm chain's second mul_mat
whose y lies on the chain's out (norm_feeds requires out to be its src1); the latter is placed on the chain's norm and
sum instead.
"""
import os
import sys

import numpy as np

import ggml_ops_ref as R

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))

RING = 65536                     # bytes; ggml_hip_assign_buffers' slot granule for a ring this small is 256
SLOT = 256
DT = {"f32": np.float32, "f16": np.uint16}
ES = {"f32": 4, "f16": 2}
K = 256                          # the decode row
HD, NH, NCTX = 64, 4, 8          # head size, heads, cache positions


def ring_granule(size):
    """assign_buffers_impl's slot rule: 64 KiB, halved while above 256 and above 1/2048 of the ring"""
    g = 65536
    while g > 256 and g > size // 2048:
        g >>= 1
    return g


class T:
    """a tensor: `ne` elements of type `typ` (ggml order, ne[0] fastest) at byte strides `nb` from byte `off` of
    buffer `buf`.  view: a view (reshape, permute, cache window) that gets no storage assigned of its own."""

    def __init__(self, buf, off, ne, typ="f32", nb=None, view=False):
        ne = tuple(int(n) for n in ne) + (1,) * (4 - len(ne))
        if nb is None:
            nb = [ES[typ]]
            for i in range(3):
                nb.append(nb[i] * ne[i])
        nb = list(nb)
        while len(nb) < 4:
            nb.append(max(nb[j] * ne[j] for j in range(len(nb))))
        self.buf, self.off, self.ne, self.typ, self.nb, self.view = buf, int(off), ne, typ, tuple(int(b) for b in nb), view

    def layout(self):
        return (self.buf, self.off, self.ne, self.typ, self.nb)

    def offsets(self):
        """byte offset of every element, shape (ne3, ne2, ne1, ne0)"""
        i = [np.arange(self.ne[d], dtype=np.int64) * self.nb[d] for d in range(4)]
        return self.off + i[3][:, None, None, None] + i[2][None, :, None, None] + i[1][None, None, :, None] + i[0]

    def bytes(self):
        """the set of bytes the elements occupy"""
        return np.unique((self.offsets()[..., None] + np.arange(ES[self.typ])).ravel())

    def contiguous(self):
        return self.nb == T(self.buf, self.off, self.ne, self.typ).nb


def ring(slot, ne, typ="f32", nb=None, view=False):
    return T("ring", slot * SLOT, ne, typ, nb, view)


class Node:
    """op(src0, src1) -> out.  p: the op's host parameter (scale: the factor; diag_mask_inf: n_past; rope: (n_past,
    n_dims); mul_mat_q4: src0 is the weight's name).  first: the node's operands are the tensors as first created,
    not the in-place nodes that rewrote them since (ggml graphs can hold both)."""

    def __init__(self, op, out, src0, src1=None, p=None, first=False):
        self.op, self.out, self.src0, self.src1, self.p, self.first = op, out, src0, src1, p, first

    def inplace(self):
        return self.out is self.src0

    def operands(self):
        return [s for s in (self.src0, self.src1) if isinstance(s, T)]


_tables = None


def tables():
    global _tables
    if _tables is None:
        _tables = R.tables()
    return _tables


def load(mem, t):
    v = mem[t.buf].view(DT[t.typ])
    o = t.offsets()
    assert (o % ES[t.typ] == 0).all() and o.min() >= 0 and o.max() + ES[t.typ] <= mem[t.buf].size, "tensor out of its buffer"
    return v[o // ES[t.typ]].copy()


def store(mem, t, a):
    v = mem[t.buf].view(DT[t.typ])
    o = t.offsets()
    assert (o % ES[t.typ] == 0).all() and o.min() >= 0 and o.max() + ES[t.typ] <= mem[t.buf].size, "tensor out of its buffer"
    a = np.asarray(a)
    v[o // ES[t.typ]] = (R.fp16_bits(a) if t.typ == "f16" and a.dtype != np.uint16 else a).reshape(o.shape)


def exact_mul_mat(wq, k, x):
    import oracle as O
    return O.mul_mat(wq, k, x)


def step(mem, n, weights, mm):
    """one node, reading the memory as it is now"""
    if n.op == "permute":
        return
    if n.op == "mul_mat_q4":
        wq, k, m = weights[n.src0]
        x = load(mem, n.src1)
        assert n.src1.ne[0] == k and n.out.ne[0] == m and n.out.ne[1] == n.src1.ne[1]
        store(mem, n.out, mm(wq, k, np.ascontiguousarray(x.reshape(-1, k))))
        return
    a = load(mem, n.src0)
    if n.op == "add":
        y = R.add(a, load(mem, n.src1))
    elif n.op == "mul":
        y = R.mul(a, load(mem, n.src1))
    elif n.op == "scale":
        y = R.scale(a, n.p)
    elif n.op == "silu":
        y = R.silu(a, tables()[0])
    elif n.op == "rms_norm":
        y = R.rms_norm(a)
    elif n.op == "diag_mask_inf":
        y = R.diag_mask_inf(a, n.p)
    elif n.op == "soft_max":
        y = R.soft_max(a, tables()[1])
    elif n.op == "rope":
        assert n.src0.ne[3] == 1
        y = R.rope(a[0], n.p[0], n.p[1])
    elif n.op == "mul_mat_f16":
        y = R.mul_mat_f16_f32(a, load(mem, n.src1))
    elif n.op == "cpy":
        t = n.out
        assert t.ne[3] == 1 and n.src0.typ == "f32"
        dst = mem[t.buf][t.off:].view(DT[t.typ])
        R.cpy(a, dst, t.ne[:3], t.nb[:3])
        return
    else:
        raise ValueError(n.op)
    store(mem, n.out, y)


class Case:
    """one node sequence with its placement.  mem: the initial memory; nodes: ggml's order; wrong: the sequence a
    missing check would amount to (None: nothing here can be reordered wrongly: a twin or a plain variant); fused:
    the g_fused slots that must count up when the sequence runs with fusion on, per mode ("exact" / "fast");
    stale: (i, z): after node i ran, its tensor struct is rewritten in place into tensor z (a new graph's)."""

    def __init__(self, name, ring_size=RING):
        self.name = name
        self.ring_size = ring_size
        self.gemm9_tile = None       # 0 / 1: k_gemm9's tile pinned (a prefill group is bitwise its members' own launches
        self.mem = {"ring": np.zeros(ring_size, np.uint8)}      # only then, include/ggml-hip.h)
        self.weights = {}
        self.nodes = []
        self.wrong = None
        self.fused = {"exact": [], "fast": []}
        self.stale = None

    def buf(self, name, nbytes):
        self.mem[name] = np.zeros(nbytes, np.uint8)

    def put(self, t, a):
        """initial contents of t"""
        if t.buf not in self.mem:
            self.buf(t.buf, t.off + int(np.prod(t.ne)) * ES[t.typ])
        store(self.mem, t, np.asarray(a))
        return t

    def weight(self, name, m, k, seed):
        import oracle as O
        w = (np.random.default_rng([0x5C4ED, seed]).standard_normal((m, k)) * 0.02).astype(np.float32)
        self.weights[name] = (np.ascontiguousarray(O.quantize_q4_0(w)[0]), k, m)
        return name

    def add(self, op, out, src0, src1=None, p=None, first=False):
        self.nodes.append(Node(op, out, src0, src1, p, first))
        return out

    def order(self, idx):
        """the wrong sequence as indices into nodes (repeats allowed)"""
        self.wrong = [self.nodes[i] for i in idx]

    def run(self, seq=None, mm=exact_mul_mat):
        mem = {k: v.copy() for k, v in self.mem.items()}
        for n in (self.nodes if seq is None else seq):
            step(mem, n, self.weights, mm)
        return mem

    def self_overlaps(self):
        """nodes whose output partially overlaps one of their operands (undefined even in order); exact in-place
        (the same layout) is allowed"""
        bad = []
        for i, n in enumerate(self.nodes):
            if n.op == "permute":
                continue
            for s in n.operands():
                if s.buf == n.out.buf and s.layout() != n.out.layout() and np.intersect1d(s.bytes(), n.out.bytes()).size:
                    bad.append(i)
        return bad


def differ(m0, m1):
    return any(not np.array_equal(m0[k], m1[k]) for k in m0)


# ------------------------------------------------------------------------------------------------ the cases
def _rng(*seed):
    return np.random.default_rng([0x5C4ED] + list(seed))


def _row(seed, n=K):
    return _rng(seed).standard_normal((1, n)).astype(np.float32)


def _group(name, y2_slot=6, held=True, m=64):
    """mm1(x) -> y1, [scale(y1) held,] mm2(x) -> y2 joins the group"""
    c = Case(name)
    x = c.put(ring(0, (K, 1)), _row(1))
    c.weight("w1", m, K, 1)
    c.weight("w2", m, K, 2)
    y1 = c.add("mul_mat_q4", ring(4, (m, 1)), "w1", x)
    if held:
        c.add("scale", ring(5, (m, 1)), y1, p=0.5)
    c.add("mul_mat_q4", ring(y2_slot, (m, 1)), "w2", x)
    return c


def group_twin():
    c = _group("group_twin")
    c.fused = {"exact": [6], "fast": [6]}
    return c


def group_y2_on_held_src():
    """mm2's y on y1's slot, which the held scale still has to read (group_join_ok: m against A->src0)"""
    c = _group("group_y2_on_held_src", 4)
    c.order([0, 2, 1])
    return c


def group_y2_on_held_out():
    """mm2's y on the held scale's output (m against A)"""
    c = _group("group_y2_on_held_out", 5)
    c.order([0, 2, 1])
    return c


def group_y2_on_y1():
    """mm2's y on y1 with nothing held (m against g.mm[i]): one launch would store both in no order"""
    c = _group("group_y2_on_y1", 4, held=False)
    c.order([1, 0])
    return c


def group_held_add_into_x():
    """a held in-place add into x, then mm2 on the original x tensor (A against m->src1)"""
    c = Case("group_held_add_into_x")
    x = c.put(ring(0, (K, 1)), _row(1))
    d = c.put(T("d", 0, (K, 1)), _row(2))
    c.weight("w1", 64, K, 1)
    c.weight("w2", 64, K, 2)
    c.add("mul_mat_q4", ring(4, (64, 1)), "w1", x)
    c.add("add", x, x, d)
    c.add("mul_mat_q4", ring(6, (64, 1)), "w2", x, first=True)
    c.order([0, 2, 1])
    return c


def group_held_cpy_into_x():
    """a held cpy of y1 into a view over x, then mm2 (A->src1 of a CPY against m->src1)"""
    c = Case("group_held_cpy_into_x")
    x = c.put(ring(0, (K, 1)), _row(1))
    c.weight("w1", 64, K, 1)
    c.weight("w2", 64, K, 2)
    y1 = c.add("mul_mat_q4", ring(4, (64, 1)), "w1", x)
    c.add("cpy", ring(1, (64, 1), view=True), y1)
    c.add("mul_mat_q4", ring(6, (64, 1)), "w2", x)
    c.order([0, 2, 1])
    return c


def group_five_siblings():
    """five siblings: the fifth opens a new group; its y lies on the first's (dead in order)"""
    c = Case("group_five_siblings")
    x = c.put(ring(0, (K, 1)), _row(1))
    for i in range(5):
        c.weight("w%d" % i, 64, K, i)
        c.add("mul_mat_q4", ring(4 + (i if i < 4 else 0), (64, 1)), "w%d" % i, x)
    c.order([4, 0, 1, 2, 3])
    c.fused = {"exact": [6], "fast": [6]}
    return c


def group_17_held():
    """seventeen held nodes, past the cap of 16: the group flushes, and mm2, whose y lies on what the held nodes
    read and wrote, comes after them"""
    c = Case("group_17_held")
    x = c.put(ring(0, (K, 1)), _row(1))
    c.weight("w1", 64, K, 1)
    c.weight("w2", 64, K, 2)
    y1 = c.add("mul_mat_q4", ring(4, (64, 1)), "w1", x)
    s = y1
    for i in range(17):
        s = c.add("scale", ring(5 + (i & 1), (64, 1)), s, p=1.5)
    c.add("mul_mat_q4", ring(6, (64, 1)), "w2", x)
    c.order([0, 18] + list(range(1, 18)))
    return c


def group_other_k():
    """a sibling with another K (and so another x): it joins nothing; its y lies on y1, which the held scale reads"""
    c = _group("group_other_k")
    c.nodes.pop()
    x2 = c.put(ring(8, (128, 1)), _row(3, 128))
    c.weight("w2", 64, 128, 2)
    c.add("mul_mat_q4", ring(4, (64, 1)), "w2", x2)
    c.order([0, 2, 1])
    return c


def _norm(name, y1_slot=20, y2_slot=21, inplace=False, with_add=True, m=64, seed=R.rms_seed(K, 1)):
    """[add(a, b) ->] rms_norm -> mul(w) -> mm1, mm2; slots: a 0, b 4, sum 8, norm 12, out 16"""
    c = Case(name)
    av, bv, rep = R.rms_rows(K, 1, seed, with_add)
    assert not rep
    a = c.put(ring(0, (K, 1)), av)
    b = c.put(ring(4, (K, 1)), bv)
    w = c.put(T("w", 0, (K, 1)), 1.0 + 0.1 * _row(5))
    c.weight("w1", m, K, 1)
    c.weight("w2", m, K, 2)
    x = c.add("add", ring(8, (K, 1)), a, b) if with_add else b
    nrm = c.add("rms_norm", x if inplace else ring(12, (K, 1)), x)
    out = c.add("mul", nrm if inplace else ring(16, (K, 1)), nrm, w)
    c.add("mul_mat_q4", ring(y1_slot, (m, 1)), "w1", out)
    c.add("mul_mat_q4", ring(y2_slot, (m, 1)), "w2", out)
    return c


NORM_FUSED = {"exact": [0, 6], "fast": [0, 6, 9]}


def norm_twin():
    c = _norm("norm_twin")
    c.fused = NORM_FUSED
    return c


def norm_inplace():
    """rms_norm and mul in place on b: the chain's outputs alias its input, which every workgroup of a prologue
    would read while one stores (try_fuse's alias loop)"""
    c = _norm("norm_inplace", inplace=True, with_add=False)
    c.order([0, 1, 0, 1, 2, 3])
    return c


def norm_add_inplace():
    """add, then rms_norm and mul in place on the sum: the outputs alias each other, not the inputs"""
    c = _norm("norm_add_inplace", inplace=True)
    c.order([0, 2, 1, 3, 4])
    return c


def norm_y1_on_a():
    """mm1's y on a's slot: a is dead in order, but a prologue still reads it (norm_feeds)"""
    c = _norm("norm_y1_on_a", y1_slot=1)
    c.order([0, 1, 2, 3, 0, 1, 2, 4])
    return c


def norm_y2_on_norm():
    """mm2's y on the chain's norm, which the group's launch stores too (norm_feeds from group_join_ok)"""
    c = _norm("norm_y2_on_norm", y2_slot=13)
    c.order([0, 1, 2, 3, 4, 1])
    return c


def norm_y2_on_sum():
    c = _norm("norm_y2_on_sum", y2_slot=9)
    c.order([0, 1, 2, 3, 4, 0])
    return c


def _silu(name, y_slot=20, inplace=False):
    """silu(a) -> mul(silu, b) -> mm; slots: a 0, b 4, u 8, out 12"""
    c = Case(name)
    a = c.put(ring(0, (K, 1)), R.silu_spread(_rng(7), K)[None, :])
    b = c.put(ring(4, (K, 1)), _row(8))
    c.weight("w1", 64, K, 1)
    u = c.add("silu", ring(8, (K, 1)), a)
    out = c.add("mul", u if inplace else ring(12, (K, 1)), u, b)
    c.add("mul_mat_q4", ring(y_slot, (64, 1)), "w1", out)
    return c


def silu_twin():
    c = _silu("silu_twin")
    c.fused = {"exact": [2], "fast": [2, 10]}
    return c


def silu_y_on_a():
    """the mm's y on the silu's input"""
    c = _silu("silu_y_on_a", y_slot=2)
    c.order([0, 1, 2, 0, 1])
    return c


def silu_mul_inplace():
    """mul in place on the silu's output: one launch stores both to one address"""
    c = _silu("silu_mul_inplace", inplace=True)
    c.order([0, 1, 0, 2])
    return c


def _bypass(name, y_slot=20, x_is_silu=False):
    """silu(a) pending, mm(x) runs ahead of it, mul(silu, b) completes; slots: a 0, b 4, x 8, u 12, out 16"""
    c = Case(name)
    a = c.put(ring(0, (K, 1)), R.silu_spread(_rng(7), K)[None, :])
    b = c.put(ring(4, (K, 1)), _row(8))
    x = c.put(ring(8, (K, 1)), _row(9))
    c.weight("w1", 64, K, 1)
    u = c.add("silu", ring(12, (K, 1)), a)
    c.add("mul_mat_q4", ring(y_slot, (64, 1)), "w1", u if x_is_silu else x)
    c.add("mul", ring(16, (K, 1)), u, b)
    return c


def bypass_twin():
    c = _bypass("bypass_twin")
    c.fused = {"exact": [5, 2], "fast": [5, 2]}
    return c


def bypass_y_on_a():
    c = _bypass("bypass_y_on_a", y_slot=1)
    c.order([1, 0, 2])
    return c


def bypass_y_on_silu():
    c = _bypass("bypass_y_on_silu", y_slot=13)
    c.order([1, 0, 2])
    return c


def bypass_x_is_silu():
    c = _bypass("bypass_x_is_silu", x_is_silu=True)
    c.order([1, 0, 2])
    return c


ROPE_P = (3, HD)                 # n_past, n_dims


def _rope_cpy(name, target):
    """rope(x [64, 4 heads, 8 tokens]) -> cpy into `target`; x at slot 32, the rope's output at slot 64"""
    c = Case(name)
    x = c.put(ring(32, (HD, NH, NCTX)), _rng(11).standard_normal((1, NCTX, NH, HD)).astype(np.float32))
    if target.buf != "ring":
        c.buf(target.buf, 2 * HD * NH * NCTX)
    r = c.add("rope", ring(64, (HD, NH, NCTX)), x, p=ROPE_P)
    c.add("cpy", target, r)
    return c


def rope_cpy_twin():
    c = _rope_cpy("rope_cpy_twin", T("kc", 0, (HD * NH, NCTX), "f16", view=True))
    c.fused = {"exact": [3], "fast": [3]}
    return c


def rope_cpy_on_input():
    """an f16 target that overlaps the rope's input"""
    c = _rope_cpy("rope_cpy_on_input", ring(40, (HD * NH, NCTX), "f16", view=True))
    c.order([1, 0])
    return c


def rope_cpy_strided_span():
    """a strided f32 target (rows 512 B apart, tokens 2048 B apart) from byte 0: its first nbytes (8192) end where
    the rope's input begins, its span (16128) covers most of that input: tokens 4 .. 7 land on it"""
    c = _rope_cpy("rope_cpy_strided_span", ring(0, (HD, NH, NCTX), nb=(4, 512, 2048), view=True))
    c.order([1, 0])
    return c


def _merge(name, cb):
    """f16 mul_mat(V, p) -> permute(0, 2, 1, 3) -> cpy into cb (two tokens, so the mul_mat is no decode KQ)"""
    c = Case(name)
    ntok = 2
    v = c.put(T("vc", 0, (NCTX, HD, NH), "f16", view=True),
              (_rng(12).standard_normal((1, NH, HD, NCTX))).astype(np.float16).view(np.uint16))
    p = c.put(ring(0, (NCTX, ntok, NH)), _rng(13).standard_normal((1, NH, ntok, NCTX)).astype(np.float32))
    kqv = c.add("mul_mat_f16", ring(8, (HD, ntok, NH)), v, p)
    m = T("ring", kqv.off, (HD, NH, ntok), nb=(4, kqv.nb[2], kqv.nb[1]), view=True)
    c.add("permute", m, kqv)
    c.add("cpy", cb, m)
    return c


def merge_twin():
    c = _merge("merge_twin", ring(16, (HD * NH, 2), view=True))
    c.fused = {"exact": [4], "fast": [4]}
    return c


def merge_cb_on_src1():
    """the merge copy's target on the mul_mat's src1"""
    c = _merge("merge_cb_on_src1", ring(0, (HD * NH, 2), view=True))
    c.order([2, 0, 1, 2])
    return c


def _batch(name, t2_off=512, rope_of_target=False):
    """a plain group mm1 | mm2 (no norm) with held copies behind it"""
    c = Case(name)
    m = HD * NH
    x = c.put(ring(0, (K, 1)), _row(1))
    c.weight("w1", m, K, 1)
    c.weight("w2", m, K, 2)
    c.buf("tg", 8192)
    y1 = c.add("mul_mat_q4", ring(4, (m, 1)), "w1", x)
    y2 = c.add("mul_mat_q4", ring(8, (m, 1)), "w2", x)
    t1 = T("tg", 0, (m, 1), "f32", view=True)
    c.add("cpy", t1, y1)
    if rope_of_target:
        c.add("rope", ring(12, (HD, NH, 1)), T("tg", 0, (HD, NH, 1), view=True), p=ROPE_P)
    else:
        c.add("cpy", T("tg", t2_off, (m, 1), "f16", view=True), y2)
    return c


def batch_twin():
    c = _batch("batch_twin", t2_off=1024)
    c.fused = {"exact": [6, 7], "fast": [6, 7]}
    return c


def batch_targets_overlap():
    """two held copies into overlapping targets: the later one must win"""
    c = _batch("batch_targets_overlap")
    c.order([0, 1, 3, 2])
    return c


def batch_rope_of_target():
    """a held rope whose input is an earlier held copy's target"""
    c = _batch("batch_rope_of_target", rope_of_target=True)
    c.order([0, 1, 3, 2])
    return c


def _glu(name, u_slot=22, p_slot=23, gate=0, n=64):
    """add -> rms_norm -> mul(w) -> w1 | w3, silu(y1) -> mul(silu, y3); y1 slot 20, y3 slot 21.  n < 64: the silu and
    the mul read the members' outputs through views of their first n elements"""
    c = _norm(name)
    y = [c.nodes[3].out, c.nodes[4].out]
    if n < 64:
        y = [T("ring", t.off, (n, 1), view=True) for t in y]
    u = c.add("silu", ring(u_slot, (n, 1)), y[gate])
    c.add("mul", ring(p_slot, (n, 1)), u, y[1 - gate])
    return c


GLU_FUSED = {"exact": [0, 6, 2], "fast": [0, 6, 9, 13]}


def glu_twin():
    c = _glu("glu_twin")
    c.fused = GLU_FUSED
    return c


def glu_gate_is_w3():
    """silu taken of w3's output: the second member is the gate"""
    c = _glu("glu_gate_is_w3", gate=1)
    c.fused = GLU_FUSED
    return c


def glu_silu_on_a():
    """the silu's output on the chain's a"""
    c = _glu("glu_silu_on_a", u_slot=1)
    c.order([0, 1, 2, 3, 4, 5, 6, 0, 1, 2])
    return c


def glu_mul_on_y3():
    """the mul's output on y3 (a ggml mul whose destination is its src1)"""
    c = _glu("glu_mul_on_y3", p_slot=21)
    c.order([0, 1, 2, 3, 5, 6, 4])
    return c


def glu_half_view():
    """silu and mul of views whose device pointers are the members' but which have half their elements (glu_prefix
    tells "reads that member's output" by the pointer): no order hazard, a shape the epilogue must not take for
    the whole rows"""
    return _glu("glu_half_view", n=32)


def _qkv(name, kt_slot=None, on_b=False, vt_off=None, half_view=False):
    """the decode attention head of a layer behind its norm: wk, rope(k) -> cpy into the f16 K cache, wv, cpy(v)
    into the transposed V cache, wq, rope(q) in place.  yk slot 20, yv 24, yq 28, the roped k 32; position 3"""
    c = Case(name)
    m, pos = HD * NH, 3
    av, bv, rep = R.rms_rows(K, 1, R.rms_seed(K, 1), True)
    assert not rep
    a = c.put(ring(0, (K, 1)), av)
    b = c.put(ring(4, (K, 1)), bv)
    w = c.put(T("w", 0, (K, 1)), 1.0 + 0.1 * _row(5))
    for i in range(3):
        c.weight("w%d" % i, m, K, i)
    c.buf("kc", NCTX * m * 2)
    c.buf("vc", m * NCTX * 2)
    s = c.add("add", ring(8, (K, 1)), a, b)
    nrm = c.add("rms_norm", ring(12, (K, 1)), s)
    out = c.add("mul", ring(16, (K, 1)), nrm, w)
    yk = c.add("mul_mat_q4", ring(20, (m, 1)), "w0", out)
    nh = NH // 2 if half_view else NH
    kr = c.add("rope", ring(32, (HD, nh, 1)), T("ring", yk.off, (HD, nh, 1), view=True), p=(pos, HD))
    if on_b:
        kt = ring(5, (HD * nh, 1), "f16", view=True)
    elif kt_slot is not None:
        kt = ring(kt_slot, (HD * nh, 1), "f16", view=True)
    else:
        kt = T("kc", pos * m * 2, (HD * nh, 1), "f16", view=True)
    c.add("cpy", kt, kr)
    yv = c.add("mul_mat_q4", ring(24, (m, 1)), "w1", out)
    vt = T("vc", pos * 2, (1, m), "f16", nb=(2, NCTX * 2), view=True) if vt_off is None else \
        T("kc", vt_off, (1, m), "f16", nb=(2, NCTX * 2), view=True)
    c.add("cpy", vt, T("ring", yv.off, (1, m), nb=(m * 4, 4), view=True))
    yq = c.add("mul_mat_q4", ring(28, (m, 1)), "w2", out)
    q3 = T("ring", yq.off, (HD, NH, 1), view=True)
    c.add("rope", q3, q3, p=(pos, HD))
    return c


QKV_FUSED = {"exact": [0, 6], "fast": [0, 6, 9, 12]}


def qkv_twin():
    c = _qkv("qkv_twin")
    c.fused = QKV_FUSED
    return c


def qkv_kt_on_member():
    """the K-cache target on a member's output (yk, dead in order once the rope has read it)"""
    c = _qkv("qkv_kt_on_member", kt_slot=21)
    c.order(list(range(10)) + [3])
    return c


def qkv_kt_on_b():
    """the K-cache target on the chain's b"""
    c = _qkv("qkv_kt_on_b", on_b=True)
    c.order(list(range(10)) + [0, 1, 2])
    return c


def qkv_targets_overlap():
    """the two copies' targets overlapping each other (V's column, 16 B apart from byte 6 of the K cache's buffer,
    walks through K's row at bytes 1536 .. 2047)"""
    c = _qkv("qkv_targets_overlap", vt_off=6)
    c.order([0, 1, 2, 3, 4, 7, 5, 6, 8, 9])
    return c


def qkv_half_view():
    """a rope that reads a member's output through a view whose device pointer is the member's but which has half
    its elements: not an order hazard (nothing the epilogue could do in another order), a shape the epilogue
    must not take for the member's whole row"""
    return _qkv("qkv_half_view", half_view=True)


def _attn(name, nkv=NCTX, inplace=False, scaled_slot=20, sm_slot=52, kqv_slot=68, cb_slot=72):
    """the decode attention of one token: KQ = mul_mat(K view, q) (held), scale -> diag_mask_inf -> soft_max,
    KQV = mul_mat(V view, soft_max), permute, cpy into the merged heads.  Slots: q 0, KQ 4, scaled 20, masked 36,
    soft_max 52, KQV 68, merged 72 (16 slots hold a row of 193 keys for 4 heads)"""
    c = Case(name)
    r = _rng(21, nkv)
    n_embd = HD * NH
    c.put(T("kc", 0, (n_embd, nkv), "f16", view=True), (r.standard_normal((1, 1, nkv, n_embd)) * 0.5).astype(np.float16).view(np.uint16))
    c.put(T("vc", 0, (nkv, n_embd), "f16", view=True), r.standard_normal((1, 1, n_embd, nkv)).astype(np.float16).view(np.uint16))
    kview = T("kc", 0, (HD, nkv, NH), "f16", nb=(2, n_embd * 2, HD * 2), view=True)
    vview = T("vc", 0, (nkv, HD, NH), "f16", nb=(2, nkv * 2, HD * nkv * 2), view=True)
    q = c.put(ring(0, (HD, 1, NH)), r.standard_normal((1, NH, 1, HD)).astype(np.float32))
    kq = c.add("mul_mat_f16", ring(4, (nkv, 1, NH)), kview, q)
    sc = c.add("scale", kq if inplace else ring(scaled_slot, (nkv, 1, NH)), kq, p=float(np.float32(1.0 / np.sqrt(HD))))
    mk = c.add("diag_mask_inf", sc if inplace else ring(36, (nkv, 1, NH)), sc, p=nkv - 1)
    sm = c.add("soft_max", mk if inplace else ring(sm_slot, (nkv, 1, NH)), mk)
    kqv = c.add("mul_mat_f16", ring(kqv_slot, (HD, 1, NH)), vview, sm)
    m = T("ring", kqv.off, (HD, NH, 1), nb=(4, kqv.nb[2], kqv.nb[1]), view=True)
    c.add("permute", m, kqv)
    c.add("cpy", ring(cb_slot, (n_embd, 1), view=True), m)
    return c


ATTN_ALL = list(range(7))


def attn_twin():
    c = _attn("attn_twin")
    c.fused = {"exact": [8, 14], "fast": [8, 14]}
    return c


def attn_inplace_192():
    """scale / mask / soft_max in place on KQ, at the most keys whose KQ the chain's launch still computes"""
    c = _attn("attn_inplace_192", 192, True)
    c.fused = {"exact": [8, 14], "fast": [8, 14]}
    return c


def attn_inplace_193():
    """... and one key past GGML_HIP_KQ_FOLD_MAX: KQ runs as its own launch first"""
    c = _attn("attn_inplace_193", 193, True)
    c.fused = {"exact": [8], "fast": [8]}
    return c


def attn_cb_on_softmax():
    """the merged-heads target on the soft_max node"""
    c = _attn("attn_cb_on_softmax", cb_slot=52)
    c.order(ATTN_ALL + [3])
    return c


def attn_cb_on_q():
    """the merged-heads target on q, which the launch that also computes KQ still reads"""
    c = _attn("attn_cb_on_q", cb_slot=0)
    c.order(ATTN_ALL + ATTN_ALL)
    return c


def attn_cb_on_scaled():
    """the merged-heads target on the scale node, which the launch stores too"""
    c = _attn("attn_cb_on_scaled", cb_slot=20)
    c.order(ATTN_ALL + [1])
    return c


def attn_kqv_on_q():
    """KQV's output on q"""
    c = _attn("attn_kqv_on_q", kqv_slot=0)
    c.order(ATTN_ALL + ATTN_ALL)
    return c


def attn_kqv_on_kq():
    """KQV's output on KQ, which every workgroup of the launch reads (or, with KQ folded in, one stores)"""
    c = _attn("attn_kqv_on_kq", kqv_slot=4)
    c.order(ATTN_ALL + [1, 2, 3])
    return c


def attn_scaled_on_q():
    """the scale node's output on q"""
    c = _attn("attn_scaled_on_q", scaled_slot=1)
    c.order(ATTN_ALL + ATTN_ALL)
    return c


def merge_cb_on_v_span():
    """the merge copy's target inside the span of the mul_mat's strided V view, past its first nbytes"""
    c = Case("merge_cb_on_v_span")
    ntok, nctx = 2, 2 * NCTX
    c.put(T("vc", 0, (nctx, HD * NH), "f16", view=True),
          _rng(12).standard_normal((1, 1, HD * NH, nctx)).astype(np.float16).view(np.uint16))
    v = T("vc", 0, (NCTX, HD, NH), "f16", nb=(2, nctx * 2, HD * nctx * 2), view=True)
    p = c.put(ring(0, (NCTX, ntok, NH)), _rng(13).standard_normal((1, NH, ntok, NCTX)).astype(np.float32))
    kqv = c.add("mul_mat_f16", ring(8, (HD, ntok, NH)), v, p)
    m = T("ring", kqv.off, (HD, NH, ntok), nb=(4, kqv.nb[2], kqv.nb[1]), view=True)
    c.add("permute", m, kqv)
    c.add("cpy", T("vc", NCTX * HD * NH * 2, (HD * NH, ntok), view=True), m)
    c.order([2, 0, 1, 2])
    return c


X9_N, X9_RING = 65, 1 << 20     # rows past IMG_MIN_N (64); a 1 MiB ring (512-byte slots) holds their tensors
X9_ROW = X9_N * K * 4            # 66560 = 130 slots


def _x9(name, inplace=False, y1_off=5 * X9_ROW):
    """the prefill chain held for the x image fold: add -> rms_norm -> mul(w) over 65 rows, two q4_0 members (M = 64)
    on fp6 images.  a at 0, b, sum, norm, out one row block apart, y1 behind them, y2 behind y1"""
    c = Case(name, X9_RING)
    c.gemm9_tile = 0
    with_add = not inplace
    av, bv, _ = R.rms_rows(K, X9_N, R.rms_seed(K, X9_N), with_add)
    a = c.put(T("ring", 0, (K, X9_N)), av)
    b = c.put(T("ring", X9_ROW, (K, X9_N)), bv)
    w = c.put(T("w", 0, (K, 1)), 1.0 + 0.1 * _row(5))
    c.weight("w1", 64, K, 1)
    c.weight("w2", 64, K, 2)
    x = c.add("add", T("ring", 2 * X9_ROW, (K, X9_N)), a, b) if with_add else b
    nrm = c.add("rms_norm", x if inplace else T("ring", 3 * X9_ROW, (K, X9_N)), x)
    out = c.add("mul", nrm if inplace else T("ring", 4 * X9_ROW, (K, X9_N)), nrm, w)
    c.add("mul_mat_q4", T("ring", y1_off, (64, X9_N)), "w1", out)
    c.add("mul_mat_q4", T("ring", 5 * X9_ROW + 16896, (64, X9_N)), "w2", out)
    return c


def x9_twin():
    c = _x9("x9_twin")
    c.fused = {"exact": [0, 6], "fast": [0, 6, 11]}
    return c


def x9_inplace():
    """the chain in place on b (try_fuse turns the fold back on after its alias loop turned it off)"""
    c = _x9("x9_inplace", inplace=True)
    c.order([0, 1, 0, 1, 2, 3])
    return c


def x9_y1_on_a():
    """a member's y on the chain's a"""
    c = _x9("x9_y1_on_a", y1_off=512)
    c.order([0, 1, 2, 3, 0, 1, 2, 4])
    return c


def stale_address():
    """a held add; its ggml_tensor struct is then rewritten in place into a tensor of a new graph (z); an rms_norm
    of that address arrives: the add runs as it was held, the norm reads what the new tensor owns"""
    c = Case("stale_address")
    av, bv, _ = R.rms_rows(K, 1, R.rms_seed(K, 1), True)
    _, zv, rep = R.rms_rows(K, 1, R.rms_seed(K, 1) + 1, False)
    assert not rep
    a = c.put(ring(0, (K, 1)), av)
    b = c.put(ring(4, (K, 1)), bv)
    z = c.put(ring(12, (K, 1)), zv)
    s = c.add("add", ring(8, (K, 1)), a, b)
    c.add("rms_norm", ring(16, (K, 1)), z)
    c.stale = (0, z)
    c.wrong = [c.nodes[0], Node("rms_norm", c.nodes[1].out, s)]
    return c


CASES = [group_twin, group_y2_on_held_src, group_y2_on_held_out, group_y2_on_y1, group_held_add_into_x,
         group_held_cpy_into_x, group_five_siblings, group_17_held, group_other_k,
         norm_twin, norm_inplace, norm_add_inplace, norm_y1_on_a, norm_y2_on_norm, norm_y2_on_sum,
         silu_twin, silu_y_on_a, silu_mul_inplace,
         bypass_twin, bypass_y_on_a, bypass_y_on_silu, bypass_x_is_silu,
         rope_cpy_twin, rope_cpy_on_input, rope_cpy_strided_span, merge_twin, merge_cb_on_src1, merge_cb_on_v_span,
         batch_twin, batch_targets_overlap, batch_rope_of_target,
         glu_twin, glu_gate_is_w3, glu_silu_on_a, glu_mul_on_y3, glu_half_view,
         qkv_twin, qkv_kt_on_member, qkv_kt_on_b, qkv_targets_overlap, qkv_half_view,
         attn_twin, attn_inplace_192, attn_inplace_193, attn_cb_on_softmax, attn_cb_on_q, attn_cb_on_scaled,
         attn_kqv_on_q, attn_kqv_on_kq, attn_scaled_on_q, x9_twin, x9_inplace, x9_y1_on_a,
         stale_address]
# the cases in which nothing can be reordered wrongly: the twins and the plain variants
NO_HAZARD = {"group_twin", "norm_twin", "silu_twin", "bypass_twin", "rope_cpy_twin", "merge_twin", "batch_twin",
             "glu_twin", "glu_gate_is_w3", "glu_half_view", "qkv_twin", "qkv_half_view", "attn_twin", "attn_inplace_192",
             "attn_inplace_193", "x9_twin"}
