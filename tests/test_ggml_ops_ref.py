"""CPU checks of the layer-op restatement (tests/ggml_ops_ref.py): with the recorded tables and cos / sin it
reproduces every fixture the compiled reference wrote (tests/golden/gen_ops_golden.c) bit for bit; this host's libm
gives the recorded tables and cos / sin (one test of its own, so another libm shows as that failure only); fma32 is
an exact single-rounding fused multiply-add (against rational arithmetic, and on cases where the float64 formula
rounds twice); the rms_norm rows the GPU tests use satisfy the order-independence condition; and the inputs the
GPU tests use to catch two classic mistakes (a soft_max maximum started at 0, squares formed in double) do change
the expected bits under those mistakes."""
import os
from fractions import Fraction

import numpy as np
import pytest

import ggml_ops_ref as R
from ggml_ops_ref import assert_bits
from golden_io import GOLDEN, load, manifest


def ld(name):
    return load("ops", name)


@pytest.fixture(scope="module")
def tabs():
    return ld("silu_table"), ld("exp_table")


def test_fixture_sizes():
    for entry in manifest("ops").values():
        assert entry["bytes"] <= 147456                      # the largest fixture there was before these
        assert os.path.getsize(os.path.join(GOLDEN, entry["file"])) == entry["bytes"]


ROPES = [(d, p) for d in (16, 8) for p in (0, 37)]


def test_host_libm_gives_the_recorded_tables_and_cos_sin(tabs):
    """tables() and rope_cos_sin() with this host's libm against the recorded run's: a host whose expf / cosf / sinf /
    powf differ fails here (and the GPU tests, which build from the host libm as the backend does, stay valid)."""
    silu, ex = R.tables()
    assert np.array_equal(ex, tabs[1])
    assert np.array_equal(silu, tabs[0])
    for d, p in ROPES:
        c, s = R.rope_cos_sin(16, d, p, 3)
        assert_bits(c, ld(f"rope{d}_{p}_cos"))
        assert_bits(s, ld(f"rope{d}_{p}_sin"))


def test_tables_follow_the_formula_with_another_expf(tabs):
    """tables(expf) uses the expf it is given (float64 exp rounded to float: not glibc's expf everywhere)"""
    silu, ex = R.tables(lambda x: np.exp(x.astype(np.float64)).astype(np.float32))
    assert np.mean(ex != tabs[1]) < 0.01 and np.mean(silu != tabs[0]) < 0.01
    fin = np.isfinite(R.fp16_to_f32(np.arange(65536, dtype=np.uint32).astype(np.uint16)))
    assert np.array_equal(ex[~fin], tabs[1][~fin])


def test_silu(tabs):
    x = ld("silu_x")
    h = R.fp16_bits(x)
    e = (h >> 10) & 31
    assert set(range(32)) <= set(e.tolist())                 # every fp16 exponent, subnormals (0) and inf (31)
    assert (np.abs(x) > 65504).any() and (R.bits(x) == 0x80000000).any() and (R.bits(x) == 0).any()
    assert_bits(R.silu(x, tabs[0]), ld("silu_y"))


def test_add_scale_mul_mask():
    assert_bits(R.add(ld("add_a"), ld("add_b")), ld("add_y"))
    assert_bits(R.scale(ld("scale_x"), ld("scale_v")[0]), ld("scale_y"))
    assert_bits(R.mul(ld("mul_a"), ld("mul_b1")), ld("mul_y1"))
    assert_bits(R.mul(ld("mul_a"), ld("mul_b5")), ld("mul_y5"))
    assert not np.array_equal(ld("mul_y1"), ld("mul_y5"))
    for p in (0, 5):
        y = ld(f"mask_y{p}")
        assert_bits(R.diag_mask_inf(ld("mask_x"), p), y)
        assert np.isinf(y).sum() == 2 * sum(max(0, 9 - 1 - p - j) for j in range(3))


@pytest.mark.parametrize("n", [6, 256, 4100])
def test_rms_norm(n):
    x = ld(f"rms{n}_x")
    assert_bits(R.rms_norm(x), ld(f"rms{n}_y"))
    a = np.abs(x[1][x[1] != 0])
    assert n < 256 or a.max() / a.min() > 2.0 ** 30            # the spread row


@pytest.mark.parametrize("n", [1, 65, 700])
def test_soft_max(n, tabs):
    x, y = ld(f"sm{n}_x"), ld(f"sm{n}_y")
    assert_bits(R.soft_max(x, tabs[1]), y)
    assert np.isfinite(y).all()
    if n > 1:
        assert np.isinf(x[1]).any() and (y[1][np.isinf(x[1])] == 0).all()
        d = (x[2] - x[2].max()).astype(np.float32)
        assert ((d < 0) & (d > -2.0 ** -24)).any()           # below the fp16 subnormal step
        h = d.astype(np.float16).astype(np.float32)
        lo, hi = np.nextafter(h.astype(np.float16), np.float16(-np.inf)), np.nextafter(h.astype(np.float16), np.float16(np.inf))
        tie = (np.abs(d - h) == np.abs(d - lo.astype(np.float32))) | (np.abs(d - h) == np.abs(d - hi.astype(np.float32)))
        assert tie.any()                                     # exact fp16 rounding ties of x - max
        assert ((x[3] - x[3].max()) < -65504).any()


@pytest.mark.parametrize("d,p", ROPES)
def test_rope(d, p):
    x = ld(f"rope{d}_{p}_x")
    y = R.rope(x, p, d, ld(f"rope{d}_{p}_cos"), ld(f"rope{d}_{p}_sin"))
    assert_bits(y, ld(f"rope{d}_{p}_y"))
    if d < 16:                                               # this ggml.c's mode 0 rotates the pairs past n_dims too
        assert not np.array_equal(ld(f"rope{d}_{p}_y")[1:, :, d:], x[1:, :, d:])


def test_cpy_into_transposed_f16():
    x = ld("cpy_x")                                          # [2, 5, 7]: ne = (7, 5, 2)
    ref = ld("cpy_y")                                        # base [2, 7, 5] f16; its transpose has ne (7, 5, 2)
    got = R.cpy(x, np.zeros(70, np.uint16), (7, 5, 2), (10, 2, 70))
    assert np.array_equal(got.reshape(2, 7, 5), ref)
    assert np.array_equal(ref.transpose(0, 2, 1), R.fp16_bits(x))


@pytest.mark.parametrize("K", [1, 31, 32, 33, 40, 128, 500])
def test_mul_mat_f16_f32(K):
    x, y, d = ld(f"mm{K}_x"), ld(f"mm{K}_y"), ld(f"mm{K}_d")
    assert_bits(R.mul_mat_f16_f32(x, y), d)
    assert_bits(R.vec_dot_f16(x[2], y[4]), d[4, 2])


def test_decode_attention_is_its_nodes(tabs):
    rng = np.random.default_rng(5)
    K = (rng.standard_normal((2, 37, 16)) * 0.5).astype(np.float16)
    V = rng.standard_normal((2, 16, 37)).astype(np.float16)
    q = rng.standard_normal((2, 16)).astype(np.float32)
    sm, kqv = R.decode_attention(K, q, V, 0.25, 36, tabs[1])
    assert sm.shape == (2, 37) and kqv.shape == (2, 16)
    for h in range(2):
        kq = np.array([R.vec_dot_f16(K[h, j], q[h]) for j in range(37)], np.float32)
        s = R.soft_max(R.scale(kq, 0.25), tabs[1])
        assert_bits(sm[h], s)
        assert_bits(kqv[h], np.array([R.vec_dot_f16(V[h, r], s) for r in range(16)], np.float32))
    sm2, _ = R.decode_attention(K, q, V, 0.25, 30, tabs[1])   # keys past n_past are masked
    assert (sm2[:, 31:] == 0).all() and (sm2[:, :31] > 0).all()


# ------------------------------------------------------------------------------------------------ fma32
def round_f32(q):
    """a Fraction rounded to the nearest float32, ties to even (normal range)"""
    if q == 0:
        return np.float32(0.0)
    a = abs(q)
    e = a.numerator.bit_length() - a.denominator.bit_length() - 24
    while a / Fraction(2) ** e >= 2 ** 24:
        e += 1
    while a / Fraction(2) ** e < 2 ** 23:
        e -= 1
    assert -149 <= e <= 104
    n = round(a / Fraction(2) ** e)                          # half to even
    v = np.float32(float(Fraction(n) * Fraction(2) ** e))    # n <= 2^24: exact
    return -v if q < 0 else v


def exact_fma(a, b, c):
    return np.array([round_f32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z)))
                     for x, y, z in zip(a, b, c)], np.float32)


def test_fma32_equals_exact_arithmetic_on_random_triples():
    rng = np.random.default_rng(32)
    n = 10000

    def rnd():
        return (rng.standard_normal(n) * np.exp2(rng.integers(-20, 21, n))).astype(np.float32)
    a, b, c = rnd(), rnd(), rnd()
    c[:2500] = -(a[:2500] * b[:2500]).astype(np.float32)     # cancellation: c = -fl(a b)
    c[2500:3000] = 0
    assert_bits(R.fma32(a, b, c), exact_fma(a, b, c))
    h = lambda v: np.clip(v, -60000, 60000).astype(np.float16).astype(np.float32)   # fp16 operands, as in vec_dot_f16
    assert_bits(R.fma32(h(a[:2000]), h(b[:2000]), c[:2000]), exact_fma(h(a[:2000]), h(b[:2000]), c[:2000]))


def double_rounding_cases():
    """a b + c just off a float32 rounding midpoint, by less than float64 resolves: a = 2^m (1 + j 2^-23),
    b = 2^m (1 - j 2^-23), so a b = 4^m (1 - j^2 2^-46); c = +-2 4^m (2^23 + t), whose float32 neighbours are
    2 4^m apart: the exact sum is the midpoint c +- 4^m moved towards c by 4^m j^2 2^-46, and rounds to c."""
    out = []
    for m in (0, 3, -5):
        for j in (1, 3, 17, 255, 362):
            for t in (1, 12345, 2, 8388607):
                for sign in (1.0, -1.0):
                    a = np.float32(2.0 ** m * (1 + j * 2.0 ** -23))
                    b = np.float32(sign * 2.0 ** m * (1 - j * 2.0 ** -23))
                    c = np.float32(sign * 2.0 * 4.0 ** m * (2 ** 23 + t))
                    out.append((a, b, c))
    return out


def test_fma32_on_double_rounding_cases_where_the_float64_formula_fails():
    cases = double_rounding_cases()
    a, b, c = (np.array(v, np.float32) for v in zip(*cases))
    for x, y, z in cases:                                    # each within 2^-30 relative of a float32 midpoint
        q = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        f = round_f32(q)
        other = np.nextafter(f, np.float32(np.inf if q > Fraction(float(f)) else -np.inf))
        mid = (Fraction(float(f)) + Fraction(float(other))) / 2
        assert 0 < abs(q - mid) <= abs(q) * Fraction(1, 2 ** 30)
    exact = exact_fma(a, b, c)
    assert_bits(R.fma32(a, b, c), exact)
    assert_bits(exact, c)
    naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    wrong = R.bits(naive) != R.bits(exact)
    assert wrong.sum() >= len(cases) // 2                    # every odd t: the tie goes to the even neighbour
    assert not wrong.all()                                   # (an even c is right by luck)


# ------------------------------------------------------------------------------------------------ rms_norm inputs
def test_order_condition_rejects_a_midpoint_row():
    assert not R._far_from_f32_midpoint(1.0 + 2.0 ** -24, 2.0 ** -50)
    assert R._far_from_f32_midpoint(1.0 + 2.0 ** -24 + 2.0 ** -40, 2.0 ** -50)
    # squares 1, 1, 1, 1 + 2^-22 (the float square of 1 + 2^-23): their mean 1 + 2^-24 is a float32 midpoint
    x = np.array([1.0, 1.0, 1.0, 1.0 + 2.0 ** -23], np.float32)
    sq = (x * x).astype(np.float32).astype(np.float64)
    assert sq.sum() / 4 == 1.0 + 2.0 ** -24
    assert not R.rms_order_free(x)
    assert R.rms_order_free(np.array([1.0, 1.0, 1.0, 1.0 + 2.0 ** -22], np.float32))
    assert R.rms_order_free(np.array([1.0, 2.0, 3.0], np.float32))
    assert not R.rms_order_free(np.zeros(4, np.float32))


@pytest.mark.parametrize("with_add,cases", [(False, R.RMS_NODE_CASES), (True, R.RMS_CHAIN_CASES), (False, R.RMS_CHAIN_CASES)],
                         ids=["node", "add_chain", "chain"])
def test_gpu_rms_norm_rows_do_not_depend_on_summation_order(with_add, cases):
    """every row the GPU tests feed an rms_norm (their seeds exactly): fsum(x^2) / n and mean + eps lie farther than
    n 2^-52 relative from every float32 rounding midpoint, and no seed needed a replacement"""
    for ncols, nrows in cases:
        a, b, replaced = R.rms_rows(ncols, nrows, R.rms_seed(ncols, nrows), with_add)
        x = R.add(a, b) if with_add else b
        assert replaced == [], (ncols, nrows, replaced)
        for r in range(nrows):
            assert R.rms_order_free(x[r]), (ncols, nrows, r)
        # and then every correct double summation gives ggml.c's float mean: pairwise, reversed, per-lane
        m = R.rms_norm_mean(x)
        sq = (x * x).astype(np.float32).astype(np.float64)
        assert np.array_equal(R.bits((np.sum(sq, axis=1) / ncols).astype(np.float32)), R.bits(m))
        assert np.array_equal(R.bits((np.cumsum(sq[:, ::-1], axis=1)[:, -1] / ncols).astype(np.float32)), R.bits(m))
        pad = np.zeros((nrows, -ncols % 64))
        lanes = np.concatenate([sq, pad], axis=1).reshape(nrows, -1, 64)
        per_lane = np.cumsum(lanes, axis=1)[:, -1, :]
        assert np.array_equal(R.bits((np.sum(per_lane, axis=1) / ncols).astype(np.float32)), R.bits(m))


@pytest.mark.parametrize("ncols,with_add", sorted(R.RMS_SQ_SEEDS))
def test_gpu_rms_norm_rows_where_the_rounding_of_the_squares_matters(ncols, with_add):
    """the rows of RMS_SQ_SEEDS: order-free, and ggml.c's float mean (float-rounded squares) differs from the mean of
    exact squares by enough to change the scale, so squaring in double, (double)x * x, changes the output bits"""
    a, b = R.rms_sq_row(ncols, with_add)
    x = R.add(a, b) if with_add else b
    assert R.rms_order_free(x[0])
    assert R.bits(R.rms_norm_mean(x)) != R.bits(R.rms_mean_exact_squares(x))
    assert not np.array_equal(R.bits(R.rms_norm(x)), R.bits(R.rms_norm_exact_squares(x)))


# ------------------------------------------------------------------------------------------------ soft_max inputs
def soft_max_max_from_zero(x, table):
    """soft_max with the running maximum started at 0 instead of -inf (the classic mistake)"""
    x = np.asarray(x, np.float32)
    mx = np.maximum(np.max(x, axis=-1, keepdims=True), np.float32(0.0))
    d = (x - mx).astype(np.float32)
    val = np.where(x == -np.inf, np.float32(0.0), R.fp16_to_f32(np.asarray(table)[R.fp16_bits(d)])).astype(np.float32)
    s = np.cumsum(val.astype(np.float64), axis=-1)[..., -1:]
    with np.errstate(divide="ignore", invalid="ignore"):
        return (val * (1.0 / s).astype(np.float32)).astype(np.float32)


def test_gpu_soft_max_rows_catch_a_maximum_started_at_zero(tabs):
    """the inputs of tests/test_gpu_ops_ref.py::test_soft_max (5 rows) and of the soft_max chain in
    tests/test_gpu_chains_ref.py, seeds included: row 1 is negative throughout, and with the maximum started at 0 its
    expected bits change at every width above 1"""
    for ncols in (63, 64, 65, 700, 2500):
        x = R.soft_max_rows(np.random.default_rng(ncols * 8 + 5), ncols, 5)
        assert x[1].max() < -4
        good, bad = R.soft_max(x, tabs[1]), soft_max_max_from_zero(x, tabs[1])
        assert not np.array_equal(R.bits(good[1]), R.bits(bad[1])), ncols
    v = np.float32(1.0 / np.sqrt(128.0))
    for ncols in (3, 64, 65, 511, 512, 513, 2047, 2048, 2049, 2500):
        x = R.soft_max_rows(np.random.default_rng(ncols), ncols, 6, float(v)).reshape(2, 3, ncols)
        mk = R.diag_mask_inf(R.scale(x, v), ncols - 3)
        vis = mk[0, 1][np.isfinite(mk[0, 1])]
        assert vis.size == ncols - 1 and vis.max() < -4        # the masked row's visible entries are all negative
        good, bad = R.soft_max(mk, tabs[1]), soft_max_max_from_zero(mk, tabs[1])
        assert not np.array_equal(R.bits(good[0, 1]), R.bits(bad[0, 1])), ncols
