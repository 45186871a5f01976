"""The in-order reference of the scheduler hazard tests (tests/sched_model.py), on the CPU: every hazard case's
inputs are such that the order a missing check would amount to changes at least one bit of the memory (without
that, the device comparison of tests/test_gpu_sched_hazards.py would show nothing), no node of any case partially
overlaps its own operands (undefined even in ggml's order), and the interpreter itself reads memory as it is at each
step."""
import numpy as np
import pytest

import ggml_ops_ref as R
import sched_model as S

IDS = [f.__name__ for f in S.CASES]


def test_every_case_is_classified():
    assert len(set(IDS)) == len(IDS) and S.NO_HAZARD <= set(IDS)
    for f in S.CASES:
        c = f()
        assert c.name == f.__name__
        assert (c.wrong is None) == (c.name in S.NO_HAZARD), c.name


@pytest.mark.parametrize("case", S.CASES, ids=IDS)
def test_no_partial_self_overlap(case):
    assert case().self_overlaps() == []


@pytest.mark.parametrize("case", [f for f in S.CASES if f.__name__ not in S.NO_HAZARD],
                         ids=[i for i in IDS if i not in S.NO_HAZARD])
def test_wrong_order_is_visible(case):
    c = case()
    assert S.differ(c.run(), c.run(c.wrong))


@pytest.mark.parametrize("case", S.CASES, ids=IDS)
def test_tensors_inside_their_buffers_and_ring_slots(case):
    """every tensor lies inside its buffer; a ring tensor that gets storage assigned starts on a slot boundary of
    assign_buffers_impl's rule for this ring size"""
    c = case()
    assert S.ring_granule(S.RING) == S.SLOT
    gran = S.ring_granule(c.ring_size)
    for n in c.nodes:
        for t in n.operands() + [n.out]:
            b = t.bytes()
            assert b[0] >= 0 and b[-1] < c.mem[t.buf].size
            if t.buf == "ring" and not t.view:
                assert t.off % gran == 0 and t.contiguous()


def test_rms_inputs_are_order_free():
    """the rows that pass through rms_norm satisfy ggml_ops_ref.rms_order_free, which keeps the numpy norm bitwise
    the device's whatever its summation order"""
    for f in S.CASES:
        c = f()
        mem = {k: v.copy() for k, v in c.mem.items()}
        for n in c.nodes:
            if n.op == "rms_norm":
                for row in S.load(mem, n.src0).reshape(-1, n.src0.ne[0]):
                    assert R.rms_order_free(row), c.name
            S.step(mem, n, c.weights, S.exact_mul_mat)


def test_interpreter_reads_memory_as_it_is():
    """an aliased sequence by hand: y = scale(x, 2) written over x's second half, then add(x, x) in place"""
    c = S.Case("hand")
    x = c.put(S.ring(0, (128, 1)), np.arange(128, dtype=np.float32)[None, :])
    lo, hi = S.ring(0, (64, 1), view=True), S.ring(1, (64, 1), view=True)
    c.add("scale", hi, lo, p=2.0)
    c.add("add", x, x, x)
    got = S.load(c.run(), x).ravel()
    want = np.concatenate([np.arange(64) * 2.0, np.arange(64) * 4.0]).astype(np.float32)
    assert np.array_equal(got, want)
    assert c.self_overlaps() == []
    c.add("scale", S.T("ring", 128, (64, 1), view=True), lo, p=1.0)      # half over its own input
    assert c.self_overlaps() == [2]


def test_ring_granule_rule():
    assert [S.ring_granule(s) for s in (65536, 1 << 20, 1 << 27, 1 << 30)] == [256, 512, 65536, 65536]
