"""The q4_0 decode GEMV's x prologues (csrc/q4_0_gemv.hip k_gemv_q4_0 PRO 1: [add ->] rms_norm -> mul, PRO 2: silu ->
mul; ghip::gemv_q4_0_multi_norm) at every width ghip::gemv_norm_supported holds a chain for, and on the far side of
each of its bounds.

Kernel level, on device pointers through ggml_hip_debug_gemv_norm:
* the chain's tensors (sum, norm, out, stored by workgroup 0) bitwise the numpy restatement of ggml.c's ops
  (tests/ggml_ops_ref.py), in buffers with 64 sentinel floats behind them;
* y of every matrix bitwise the plain GEMV (the same entry with kind 0) on the reference `out` uploaded from the host
  (the contract of csrc/q4_0_kernels.h), and within the project's oracle bound of oracle.mul_mat on that `out`, so that
  the twin kernel cannot hide an error the two share; 64 sentinel floats behind every y;
* the same y with sum, norm and out all null;
* K = 64 (a quarter of one x-wave), 128 and 512 (few whole x-waves), 4096 | 4160 (1 | 2 pairs per lane; a partial last
  x-wave), 8192 (kind 1's maximum: all 16 waves are x-waves), 8256 (3 pairs per lane, kind 2 only), 12288 (kind 2's
  maximum); one to four sibling matrices (the fourth weight pointer is not preloaded);
* 20000 rows, more than 64 per CU of any device with at most 312 CUs, which takes the launcher to the VAR 3 schedule
  at K <= 8192 (K > 8192 always runs VAR 3).  Which schedule ran is not observable: it follows from M, K and the bounds
  in gemv_q4_0_multi_norm;
* every row map and ring depth of ggml_hip_debug_set_gemv_policy: the same bits;
* widths past the bounds are refused with nothing launched (every sentinel in place).

Hook level, through hand-built nodes (tests/hook_nodes.py) in fast mode with fusion on: a one-row chain followed by
one to three q4_0 mul_mats on its output runs as one GEMV launch with the prologue at the supported widths (fused
counters 9 / 10), and as its own launch followed by the plain GEMV at wider ones, LLaMA-13B's n_ff = 13824 and 16384
among them; before gemv_norm_supported the scheduler held chains up to 16384 wide and the launcher's refusal ended
the process."""
import ctypes

import numpy as np
import pytest

import gemv_norm_util as U
import ggml_ops_ref as R
import hook_nodes as H
from ggml_ops_ref import assert_bits
from hip_env import ggml_hip, gpu_available

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason="needs a HIP device and libggml_hip.so")]

DB = ggml_hip.DeviceBuffer


@pytest.fixture(scope="module")
def tabs():
    return R.tables()


_cases = {}


def chain(kind, K, with_add, tabs):
    """chain_case, computed once per (kind, K, with_add) and left unchanged"""
    key = (kind, K, with_add)
    if key not in _cases:
        _cases[key] = U.chain_case(kind, K, with_add, tabs)
        U.assert_case_inputs(_cases[key])
        for v in _cases[key].values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return _cases[key]


KIND_KS = ([(1, True, K) for K in U.KS_KIND1] + [(1, False, K) for K in U.KS_KIND1] +
           [(2, False, K) for K in U.KS_KIND2])
KIND_NAMES = {(1, True): "add_norm", (1, False): "norm", (2, False): "silu"}
KIND_IDS = ["%s-K%d" % (KIND_NAMES[(k, a)], K) for k, a, K in KIND_KS]


class Launch:
    """the device side of one case: weights, the chain's inputs, and launches into fresh sentinel buffers"""

    def __init__(self, L, c, Ms, seed):
        self.L, self.c, self.Ms, self.K = L, c, Ms, c["K"]
        rng = np.random.default_rng(seed)
        self.wq = [U.rand_q4(M, self.K, rng) for M in Ms]
        self.W = [DB.from_array(w) for w in self.wq]
        self.a = DB.from_array(c["a"]) if c["a"] is not None else None
        self.b = DB.from_array(c["b"])
        self.w = DB.from_array(c["w"]) if c["w"] is not None else None
        self.x = DB.from_array(c["out"])                    # the reference `out`, for the plain GEMV

    def run(self, kind, chain_bufs=True, raw=False):
        """-> (rc, y buffers, {sum, norm, out} buffers)"""
        ys = [U.sentinel_buf(M) for M in self.Ms]
        ex = {k: U.sentinel_buf(self.K) for k in ("sum", "norm", "out")} if chain_bufs else {}
        if kind == 0:
            rc, _ = U.gemv_norm_rc(self.L, self.W, self.Ms, self.K, 0, None, self.x, None, ys)
        else:
            rc, _ = U.gemv_norm_rc(self.L, self.W, self.Ms, self.K, kind, self.a, self.b, self.w, ys, extra=ex)
        if not raw:
            ggml_hip.check(rc, "gemv_norm")
        return rc, ys, ex

    def read_y(self, ys):
        return [U.read_checked(y, M) for y, M in zip(ys, self.Ms)]

    def assert_chain(self, ex):
        c = self.c
        for k in ("sum", "norm", "out"):
            if c[k] is None:                                 # kind 2 has no sum: the buffer stays as it was
                assert U.untouched(ex[k], self.K)
            else:
                assert_bits(U.read_checked(ex[k], self.K), c[k])


def check_prologue(L, c, Ms, seed):
    ln = Launch(L, c, Ms, seed)
    _, ys, ex = ln.run(c["kind"])
    ln.assert_chain(ex)
    got = ln.read_y(ys)
    _, yt, _ = ln.run(0)
    twin = ln.read_y(yt)
    for i, M in enumerate(Ms):
        assert_bits(got[i], twin[i])
        U.assert_oracle(ln.wq[i], ln.K, c["out"], got[i])
    _, yn, _ = ln.run(c["kind"], chain_bufs=False)           # no chain tensor wanted: the same y
    for g, n in zip(got, ln.read_y(yn)):
        assert_bits(n, g)
    return ln, got


@pytest.mark.parametrize("Ms", U.ROW_SETS, ids=lambda m: "M" + "_".join(map(str, m)))
@pytest.mark.parametrize("kind,with_add,K", KIND_KS, ids=KIND_IDS)
def test_prologue(tabs, kind, with_add, K, Ms):
    check_prologue(ggml_hip.load(), chain(kind, K, with_add, tabs), Ms, K + sum(Ms) + len(Ms))


@pytest.mark.parametrize("K", [64, 4160])
@pytest.mark.parametrize("kind,with_add", [(1, True), (2, False)], ids=["add_norm", "silu"])
def test_prologue_many_rows(tabs, kind, with_add, K):
    """20000 rows: above 64 rows per CU the launcher takes the VAR 3 schedule (the x-waves issue their weights before
    they quantize) at two workgroups per CU; implied by M and the bounds in gemv_q4_0_multi_norm / launch_gemv_w, not
    observed"""
    check_prologue(ggml_hip.load(), chain(kind, K, with_add, tabs), [20000], K + 20000)


@pytest.mark.parametrize("K", [64, 4160, 8192])
@pytest.mark.parametrize("kind,with_add", [(1, True), (2, False)], ids=["add_norm", "silu"])
def test_prologue_policies(tabs, kind, with_add, K):
    """every row map (strided, interleaved, blocked) and ring depth: the same bits as the automatic policy's"""
    L = ggml_hip.load()
    c = chain(kind, K, with_add, tabs)
    ln, want = check_prologue(L, c, [64, 2, 130], K + 7)
    L.ggml_hip_debug_set_gemv_policy.argtypes = [ctypes.c_int] * 4
    try:
        for map_ in (0, 1, 2):
            for depth in (1, 2):
                ggml_hip.check(L.ggml_hip_debug_set_gemv_policy(map_, depth, 1, 0), "policy")
                _, ys, ex = ln.run(kind)
                ln.assert_chain(ex)
                for g, y in zip(want, ln.read_y(ys)):
                    assert_bits(y, g)
    finally:
        L.ggml_hip_debug_set_gemv_policy(-1, 0, 1, 0)


@pytest.mark.parametrize("kind,with_add,K", [(1, True, 8256), (1, False, 8256), (1, True, 12352), (2, False, 12352),
                                             (1, True, 16384), (2, False, 16384)])
def test_unsupported_width_is_refused(tabs, kind, with_add, K):
    """past gemv_norm_supported the launcher returns an error and launches nothing: every word of y, sum, norm and out
    is still the sentinel.  (The inputs are those of a supported width, cut or repeated to K: nothing reads them.)"""
    L = ggml_hip.load()
    base = chain(kind, 4160, with_add, tabs)
    c = {k: (np.resize(v, K) if isinstance(v, np.ndarray) else v) for k, v in base.items()}
    c["K"] = K
    ln = Launch(L, c, [64, 2, 130], K)
    rc, ys, ex = ln.run(kind, raw=True)
    assert rc != 0
    assert all(U.untouched(y, M) for y, M in zip(ys, ln.Ms))
    assert all(U.untouched(ex[k], K) for k in ex)


# ------------------------------------------------------------------------------------------------ hook level
FUSED_NORM, FUSED_SILU, FUSED_GROUP, FUSED_GEMV_NORM, FUSED_GEMV_SILU = 0, 2, 6, 9, 10      # g_fused slots
HOOK_MS = (17, 64, 130)


@pytest.fixture
def g():
    """a node builder in fast mode with fusion and the prologue fold on, the counters reset"""
    L = ggml_hip.load()
    with H.restore_switches(L):
        ggml_hip.check(L.ggml_hip_set_exact(0), "set_exact")
        H.set_fuse(L, 1)
        L.ggml_hip_debug_set_norm_fold.argtypes = [ctypes.c_int]
        ggml_hip.check(L.ggml_hip_debug_set_norm_fold(1), "norm_fold")
        n = H.Nodes(L)
        try:
            yield n
        finally:
            n.close()


def plain_mul_mat(wq, K, x):
    """ggml_hip_mul_mat_q4_0 of one row x"""
    M = wq.shape[0]
    wd, xd, yd = DB.from_array(wq), DB.from_array(x), DB(M * 4)
    ggml_hip.check(ggml_hip.load().ggml_hip_mul_mat_q4_0(wd.ptr, K, M, xd.ptr, 1, yd.ptr, None), "mul_mat_q4_0")
    y = yd.download((M,), np.float32)
    for b in (wd, xd, yd):
        b.free()
    return y


def run_hook_chain(g, c, Ms, seed):
    """chain nodes -> one q4_0 mul_mat per M on the chain's output, every node forwarded, everything read back and
    compared; returns the fused counters"""
    K = c["K"]
    rng = np.random.default_rng(seed)
    wq = [U.rand_q4(M, K, rng) for M in Ms]
    row = lambda v: g.dev(np.array(v[None, :]))
    nodes, ref = [], []
    if c["kind"] == 1:
        tb = row(c["b"])
        if c["a"] is not None:
            nodes.append(g.node(H.OP_ADD, row(c["a"]), tb))
            ref.append(c["sum"])
        nodes.append(g.node(H.OP_RMS_NORM, nodes[-1] if nodes else tb))
        nodes.append(g.node(H.OP_MUL, nodes[-1], row(c["w"])))
    else:
        nodes.append(g.node(H.OP_SILU, row(c["a"])))
        nodes.append(g.node(H.OP_MUL, nodes[-1], row(c["b"])))
    ref += [c["norm"], c["out"]]
    ops = [t.op for t in nodes] + [H.OP_MUL_MAT] * len(Ms)
    mms = []
    for w, M in zip(wq, Ms):
        t = g.mm_q4_0(g.weight_q4_0(w, K, M), nodes[-1])
        g.L.ggml_hip_assign_buffers_no_scratch(ctypes.byref(t))
        assert t.backend == ggml_hip.GGML_BACKEND_GPU and t.extra
        g.owned.append(t)
        mms.append(t)
    H.op_stats(g.L)                                          # (every buffer is assigned: nothing flushes from here)
    for t in nodes + mms:
        g.forward(t)
    ys = [g.read(t, (M,)) for t, M in zip(mms, Ms)]          # (the first read flushes what is held)
    for t, r in zip(nodes, ref):
        assert_bits(g.read(t, (K,)), r)
    got, fused = H.op_stats(g.L)
    want = np.zeros_like(got)
    for op in ops:
        want[op] += 1
    assert np.array_equal(got, want), got.nonzero()
    for w, y in zip(wq, ys):
        assert_bits(y, plain_mul_mat(w, K, c["out"]))
        U.assert_oracle(w, K, c["out"], y)
    return fused


HOOK_CASES = ([(1, a, K, n, 1) for a in (True, False) for K in U.HOOK_KS[1] for n in (1, 2, 3)] +
              [(2, False, K, n, 0) for K in U.HOOK_KS[2] for n in (1, 2, 3)] +
              [(2, False, 8256, 2, 1), (2, False, 64, 3, 1)])


@pytest.mark.parametrize("kind,with_add,K,n,epi", HOOK_CASES)
def test_hook_chain_runs_in_the_prologue(g, tabs, kind, with_add, K, n, epi):
    """one launch: the chain (slot 0 / 2) inside the GEMV (slot 9 / 10) of the n mul_mats (slot 6 when n > 1); the
    epilogue fold switch (w1|w3 and q|k|v epilogues, not in play here) must not matter"""
    g.L.ggml_hip_debug_set_epi_fold.argtypes = [ctypes.c_int]
    ggml_hip.check(g.L.ggml_hip_debug_set_epi_fold(epi), "epi_fold")
    fused = run_hook_chain(g, chain(kind, K, with_add, tabs), HOOK_MS[:n], K + n)
    want = np.zeros_like(fused)
    want[FUSED_NORM if kind == 1 else FUSED_SILU] = 1
    want[FUSED_GEMV_NORM if kind == 1 else FUSED_GEMV_SILU] = 1
    want[FUSED_GROUP] = int(n > 1)
    assert np.array_equal(fused, want), fused


@pytest.mark.parametrize("kind,K", [(k, K) for k in (1, 2) for K in U.HOOK_KS_WIDE[k]])
def test_hook_chain_wider_than_the_prologue(g, tabs, kind, K):
    """not held: the chain is its own fused launch (slot 0 / 2), the mul_mat the plain GEMV, and the process lives.
    (With the hold rule `<= 16384` the launcher's refusal reached HIP_FATAL.)"""
    fused = run_hook_chain(g, chain(kind, K, kind == 1, tabs), [64], K)
    want = np.zeros_like(fused)
    want[FUSED_NORM if kind == 1 else FUSED_SILU] = 1
    assert np.array_equal(fused, want), fused
