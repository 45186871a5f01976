"""numpy restatement of the reference's CPU ops of a LLaMA layer (ggml.c), bit for bit: the fp16 silu / exp
tables of ggml_init, add, mul, scale, silu, diag_mask_inf, rms_norm, soft_max, mode-0 rope, the strided cpy,
ggml_vec_dot_f16 in its AVX F16 schedule with the F16 x F32 mul_mat on top of it, and the decode attention as
its nodes compute it.

Written from ggml.c, not from the device kernels.  Every float32 step is rounded on its own (the reference is
built without contraction); the sums ggml.c forms in ggml_float are formed in float64 in ggml.c's order.  The
transcendental functions (expf, cosf, sinf, powf) are the host libm's, called through ctypes: the same functions
ggml.c and the backend call, so the tables equal theirs on the same host.

Checked against fixtures recorded from the compiled reference (tests/golden/gen_ops_golden.c) by
tests/test_ggml_ops_ref.py; the GPU tests (tests/test_gpu_ops_ref.py, tests/test_gpu_chains_ref.py) use it as their
reference on fresh data.
"""
import ctypes
import ctypes.util

import numpy as np

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _n in ("expf", "cosf", "sinf"):
    getattr(_libm, _n).argtypes = [ctypes.c_float]
    getattr(_libm, _n).restype = ctypes.c_float
_libm.powf.argtypes = [ctypes.c_float, ctypes.c_float]
_libm.powf.restype = ctypes.c_float

f32 = np.float32


def _map(fn, x):
    """fn (float -> float, a libm function) over a float32 array, one call per element."""
    x = np.ascontiguousarray(x, np.float32)
    return np.array([fn(v) for v in x.ravel().tolist()], np.float32).reshape(x.shape)


def expf(x):
    return _map(_libm.expf, x)


def cosf(x):
    return _map(_libm.cosf, x)


def sinf(x):
    return _map(_libm.sinf, x)


def bits(a):
    """the bit patterns of a float32 array (for bitwise comparisons; -0 != +0, NaN payloads count)"""
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def fp16_bits(x):
    """GGML_FP32_TO_FP16 (F16C _cvtss_sh(x, 0): round to nearest even, overflow to inf) -> uint16"""
    with np.errstate(over="ignore"):
        return np.ascontiguousarray(x, np.float32).astype(np.float16).view(np.uint16)


def fp16_to_f32(h):
    """GGML_FP16_TO_FP32 of uint16 bit patterns (exact)"""
    return np.ascontiguousarray(h, np.uint16).view(np.float16).astype(np.float32)


# ------------------------------------------------------------------------------------------------ tables
def tables(expf=expf):
    """(silu_f16, exp_f16), 65,536 uint16 each: ggml_init's table_silu_f16 / table_exp_f16 (ggml.c:4246-4254),
    fp16(f / (1.0f + expf(-f))) and fp16(expf(f)) for every fp16 bit pattern f.  A NaN pattern gives itself with the
    quiet bit set (the conversions quiet it, x + x in expf and the division's first operand carry it through)."""
    i = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    f = fp16_to_f32(i)
    nan = np.isnan(f)
    fz = np.where(nan, f32(0.0), f)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        e = expf(-fz)
        silu = fp16_bits((fz / (f32(1.0) + e).astype(np.float32)).astype(np.float32))
        ex = fp16_bits(expf(fz))
    silu = np.where(nan, i | np.uint16(0x0200), silu).astype(np.uint16)
    ex = np.where(nan, i | np.uint16(0x0200), ex).astype(np.uint16)
    return silu, ex


# ------------------------------------------------------------------------------------------------ elementwise
def add(a, b):
    """ggml_compute_forward_add_f32 (ggml.c:8260)"""
    return (np.asarray(a, np.float32) + np.asarray(b, np.float32)).astype(np.float32)


def mul(a, b):
    """ggml_compute_forward_mul_f32 (ggml.c:9149): a [ne03][ne02][ne01][ne00] (any leading rank), b the same rank
    with each leading extent dividing a's: row (i03, i02, i01) of a times row (i03 % ne13, i02 % ne12, i01 % ne11)"""
    a = np.asarray(a, np.float32)
    b = np.asarray(b, np.float32)
    assert a.ndim == b.ndim and a.shape[-1] == b.shape[-1]
    idx = np.ix_(*[np.arange(n) % m for n, m in zip(a.shape[:-1], b.shape[:-1])])
    return (a * b[idx]).astype(np.float32)


def scale(x, v):
    """ggml_compute_forward_scale_f32 (ggml.c:11633): x * v, v a float"""
    return (np.asarray(x, np.float32) * f32(v)).astype(np.float32)


def silu(x, table):
    """ggml_vec_silu_f32 with GGML_SILU_FP16 (ggml.c:3531): table_silu_f16[fp16(x)] widened"""
    return fp16_to_f32(np.asarray(table, np.uint16)[fp16_bits(x)])


def diag_mask_inf(x, n_past):
    """ggml_compute_forward_diag_mask_f32 (ggml.c:12195): x [..., nr, nc]; element i of row j of each channel
    becomes -inf when i > n_past + j"""
    x = np.array(x, np.float32)
    nr, nc = x.shape[-2], x.shape[-1]
    m = np.arange(nc)[None, :] > n_past + np.arange(nr)[:, None]
    x[..., m] = -np.inf
    return x


# ------------------------------------------------------------------------------------------------ row reductions
def rms_norm_mean(x):
    """the float `mean` of ggml_compute_forward_rms_norm_f32 (ggml.c:10425-10430): sum += (double)(x * x) in
    order along the row (np.cumsum is sequential), mean = (float)(sum / n)"""
    x = np.asarray(x, np.float32)
    sq = (x * x).astype(np.float32).astype(np.float64)
    s = np.cumsum(sq, axis=-1, dtype=np.float64)[..., -1]
    return (s / np.float64(x.shape[-1])).astype(np.float32)


def rms_norm(x):
    """ggml_compute_forward_rms_norm_f32 (ggml.c:10389): scale = 1.0f / sqrtf(mean + 1e-6f), y = x * scale"""
    x = np.asarray(x, np.float32)
    mean = rms_norm_mean(x)
    sc = (f32(1.0) / np.sqrt((mean + f32(1e-6)).astype(np.float32)).astype(np.float32)).astype(np.float32)
    return (x * sc[..., None]).astype(np.float32)


def soft_max(x, table):
    """ggml_compute_forward_soft_max_f32 (ggml.c:12284) over the last axis: max by ggml_vec_max_f32; for
    x != -inf val = f32(table_exp_f16[fp16(x - max)]), summed in double in order, else 0; then
    y = val * (float)(1.0 / sum)"""
    x = np.asarray(x, np.float32)
    mx = np.max(x, axis=-1, keepdims=True)
    with np.errstate(invalid="ignore"):
        d = (x - mx).astype(np.float32)
    val = fp16_to_f32(np.asarray(table, np.uint16)[fp16_bits(d)])
    val = np.where(x == -np.inf, f32(0.0), val).astype(np.float32)
    s = np.cumsum(val.astype(np.float64), axis=-1, dtype=np.float64)[..., -1:]
    with np.errstate(divide="ignore"):
        inv = (np.float64(1.0) / s).astype(np.float32)
    return (val * inv).astype(np.float32)


# ------------------------------------------------------------------------------------------------ rope (mode 0)
def rope_theta(ne0, n_dims, positions):
    """float32 [len(positions), ne0 / 2]: theta of pair j at position p (ggml.c:12771-12815): starts at (float)p
    and is multiplied by the float theta_scale = powf(10000.0, -2.0f / n_dims) once per pair"""
    theta_scale = f32(_libm.powf(10000.0, float(f32(-2.0) / f32(n_dims))))
    th = np.empty((len(positions), ne0 // 2), np.float32)
    t = np.asarray(positions).astype(np.float32)
    for j in range(ne0 // 2):
        th[:, j] = t
        t = (t * theta_scale).astype(np.float32)
    return th


def rope_cos_sin(ne0, n_dims, n_past, ntok):
    """(cos, sin) float32 [ntok, ne0 / 2] of the host libm for tokens at positions n_past .. n_past + ntok - 1"""
    th = rope_theta(ne0, n_dims, np.arange(n_past, n_past + ntok))
    return cosf(th), sinf(th)


def rope(x, n_past, n_dims, cos=None, sin=None):
    """ggml_compute_forward_rope_f32, mode 0 (ggml.c:12714, 12811-12825): x [ntok (ne2), heads (ne1), ne0]; token
    i2 is at position n_past + i2; every pair (2j, 2j + 1) of a row, j < ne0 / 2, is rotated by theta_j:
    y0 = x0 * cos - x1 * sin, y1 = x0 * sin + x1 * cos, each product and sum rounded.  n_dims only sets
    theta_scale: this ggml.c's mode 0 walks the whole row (its loop runs to ne0), so with n_dims < ne0 the
    pairs at and past n_dims are rotated too, by the angles the running theta has reached.  cos / sin
    [ntok, ne0 / 2]: the values to use (a recorded run's); default the host libm's."""
    x = np.asarray(x, np.float32)
    ntok, _, ne0 = x.shape
    if cos is None:
        cos, sin = rope_cos_sin(ne0, n_dims, n_past, ntok)
    c = np.asarray(cos, np.float32)[:, None, :]
    s = np.asarray(sin, np.float32)[:, None, :]
    x0, x1 = x[..., 0::2], x[..., 1::2]
    y = np.empty_like(x)
    y[..., 0::2] = ((x0 * c).astype(np.float32) - (x1 * s).astype(np.float32)).astype(np.float32)
    y[..., 1::2] = ((x0 * s).astype(np.float32) + (x1 * c).astype(np.float32)).astype(np.float32)
    return y


# ------------------------------------------------------------------------------------------------ cpy
def cpy(src, dst, ne, nb):
    """ggml_compute_forward_dup_f32 between 3-d layouts: element i of src (a float32 array, in its logical
    C order = ggml order i0 fastest) goes to element i of the target in the target's logical order, the target
    having extents ne = (ne0, ne1, ne2) and byte strides nb = (nb0, nb1, nb2) inside dst, a 1-d array of float32
    or uint16 (F16 bit patterns: GGML_FP32_TO_FP16).  Returns dst."""
    v = np.ascontiguousarray(src, np.float32).ravel()
    es = dst.dtype.itemsize
    assert v.size == ne[0] * ne[1] * ne[2] and all(b % es == 0 for b in nb)
    i = np.arange(v.size)
    off = (i % ne[0]) * nb[0] + ((i // ne[0]) % ne[1]) * nb[1] + (i // (ne[0] * ne[1])) * nb[2]
    dst[off // es] = fp16_bits(v) if dst.dtype == np.uint16 else v
    return dst


# ------------------------------------------------------------------------------------------------ fma, f16 dot
def fma32(a, b, c):
    """fmaf on float32 arrays, exactly: a * b + c rounded to float32 once.  The product of two float32 values is
    exact in float64 (48 significant bits).  Its sum with c is formed by an error-free TwoSum; when the float64
    sum is inexact it is moved to the neighbour with an odd significand (round to odd), after which the cast to
    float32 rounds as if from the exact value (53 >= 24 + 2 bits).  float64(a * b + c).astype(float32) would round
    twice."""
    a = np.asarray(a, np.float32).astype(np.float64)
    b = np.asarray(b, np.float32).astype(np.float64)
    c = np.asarray(c, np.float32).astype(np.float64)
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)                       # s + err == p + c exactly
    s = np.array(s, np.float64, ndmin=1)
    err = np.broadcast_to(err, s.shape)
    fix = (err != 0) & np.isfinite(s) & ((s.view(np.int64) & 1) == 0)
    away = np.where(err > 0, np.inf, -np.inf)
    s = np.where(fix, np.nextafter(s, away), s)
    return s.astype(np.float32).reshape(np.broadcast(a, b, c).shape)


def vec_dot_f16(x16, y32):
    """ggml_vec_dot_f16 (ggml.c:2303) of F16 rows x16 [..., K] (float16 or uint16 bit patterns) and
    fp16(y32 [..., K]) (ggml_compute_forward_mul_mat_f16_f32 rounds src1 to fp16 first), in the AVX F16 schedule
    with FMA: element e < np = K & ~31 goes to chain e % 32 (4 vectors of 8 lanes), sum = fmaf(x, y, sum) in order
    of e; GGML_F32x8_REDUCE ((v0 + v2) + (v1 + v3), the 128-bit halves, two hadds); then the leftovers
    (ggml_float)(x * y) added in double in order; the result is the double sum rounded to float.  The leading
    axes broadcast."""
    x16 = np.asarray(x16)
    x = (x16.view(np.float16) if x16.dtype == np.uint16 else x16.astype(np.float16)).astype(np.float32)
    y = fp16_to_f32(fp16_bits(y32)).reshape(np.shape(y32))
    K = x.shape[-1]
    assert y.shape[-1] == K
    lead = np.broadcast(x[..., 0], y[..., 0]).shape
    np_ = K & ~31
    acc = np.zeros(lead + (32,), np.float32)
    for i in range(0, np_, 32):
        acc = fma32(x[..., i:i + 32], y[..., i:i + 32], acc)
    v = acc.reshape(lead + (4, 8))
    v0 = (v[..., 0, :] + v[..., 2, :]).astype(np.float32)
    v1 = (v[..., 1, :] + v[..., 3, :]).astype(np.float32)
    v0 = (v0 + v1).astype(np.float32)
    t0 = (v0[..., 0:4] + v0[..., 4:8]).astype(np.float32)
    t1a = (t0[..., 0] + t0[..., 1]).astype(np.float32)
    t1b = (t0[..., 2] + t0[..., 3]).astype(np.float32)
    sumf = (t1a + t1b).astype(np.float32).astype(np.float64)
    for i in range(np_, K):
        sumf = sumf + (x[..., i] * y[..., i]).astype(np.float32).astype(np.float64)
    return sumf.astype(np.float32)


def mul_mat_f16_f32(x16, y32):
    """ggml_compute_forward_mul_mat_f16_f32 (ggml.c:11026): x16 [..., ne01, K] F16, y32 [..., ne11, K] F32 ->
    [..., ne11, ne01], dst[i1][i0] = vec_dot_f16(x16[i0], fp16(y32[i1]))"""
    x16 = np.asarray(x16)
    y32 = np.asarray(y32, np.float32)
    return vec_dot_f16(x16[..., None, :, :], y32[..., :, None, :])


def decode_attention(K, q, V, scale_v, n_past, table):
    """The decode attention of one query row per head as llama.cpp's nodes compute it: KQ = mul_mat(K, q),
    scale, diag_mask_inf(n_past), soft_max, KQV = mul_mat(V, soft_max).  K [heads, nkv, hd] F16, q [heads, hd] F32,
    V [heads, hd, nkv] F16 (the transposed cache's rows), table the exp table.  Returns (softmax rows [heads, nkv],
    KQV [heads, hd])."""
    kq = mul_mat_f16_f32(K, np.asarray(q, np.float32)[:, None, :])              # [heads, 1, nkv]
    sm = soft_max(diag_mask_inf(scale(kq, scale_v), n_past), table)
    kqv = mul_mat_f16_f32(V, sm)                                                # [heads, 1, hd]
    return sm[:, 0, :], kqv[:, 0, :]


# ------------------------------------------------------------------------------------------------ test inputs
# The device forms rms_norm's double sum of squares in another order than ggml.c (per lane, then across lanes).
# Any correct double summation of n non-negative terms is within n 2^-52 relative of another, so the float
# `mean` is the same whenever the exact mean lies farther than that from every float32 rounding midpoint; the
# rows the GPU tests use are required to (tests/test_ggml_ops_ref.py asserts it for the very seeds used).

def _far_from_f32_midpoint(v, rel):
    """is the float64 v > 0 farther than rel * v from both rounding midpoints next to float32(v)?"""
    f = np.float32(v)
    for other in (np.nextafter(f, f32(np.inf)), np.nextafter(f, f32(-np.inf))):
        mid = (np.float64(f) + np.float64(other)) / 2.0                       # exact in float64
        if abs(np.float64(v) - mid) <= rel * abs(np.float64(v)):
            return False
    return True


def rms_order_free(row):
    """the order-independence condition on one float32 row: fsum(x^2) / n, and mean + eps feeding sqrtf, lie farther
    than n 2^-52 (+ 2^-51 for the rounding of fsum and of the division here) relative from every float32 rounding
    midpoint"""
    import math
    row = np.asarray(row, np.float32)
    n = row.size
    sq = (row * row).astype(np.float32).astype(np.float64)
    m = math.fsum(sq.tolist()) / n
    if not (m > 0 and np.isfinite(m)):
        return False
    rel = n * 2.0 ** -52 + 2.0 ** -51
    return _far_from_f32_midpoint(m, rel) and _far_from_f32_midpoint(np.float64(np.float32(m)) + np.float64(f32(1e-6)), rel)


def _rms_candidate(ncols, r, seed):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal(ncols)
    b = rng.standard_normal(ncols)
    if r % 3 == 1:                                        # magnitudes spread over 2^+-20
        a = a * np.exp2(rng.integers(-20, 21, ncols))
        b = b * np.exp2(rng.integers(-20, 21, ncols))
    elif r % 3 == 2:                                      # a mean of a few eps.  (Not within a factor 4 of eps: there
        a, b = a * 3e-3, b * 3e-3                         # float mean + eps, 25 bits, is an exact float32 tie every
                                                          # other time; harmless, but at distance 0 from a midpoint)
    return a.astype(np.float32), b.astype(np.float32)


def rms_rows(ncols, nrows, seed, with_add=False):
    """(a, b, replaced): float32 [nrows, ncols] rows for the rms_norm tests, row r from seed 1000 * seed + r; the
    rms_norm input is b (with_add: a + b, rounded) and satisfies rms_order_free; a row that does not is replaced by
    the next seed's (+ 500, + 1000, ...); `replaced` lists the rows r that were (none, for the seeds in use)."""
    A = np.empty((nrows, ncols), np.float32)
    B = np.empty((nrows, ncols), np.float32)
    replaced = []
    for r in range(nrows):
        s = 1000 * seed + r
        while True:
            a, b = _rms_candidate(ncols, r, s)
            if rms_order_free(add(a, b) if with_add else b):
                break
            s += 500
            replaced.append(r)
        A[r], B[r] = a, b
    return A, B, replaced


# (ncols, nrows) of the single-node rms_norm tests and of the two chain kernels' tests (seed = ncols * 10 + nrows)
RMS_NODE_CASES = [(nc, nr) for nc in (1, 6, 63, 64, 65, 256, 4100, 16388) for nr in (1, 5)]
RMS_CHAIN_CASES = [(nc, nr) for nc in (4, 64, 256, 4100, 16384, 1, 6, 63, 4098, 16388) for nr in (1, 5)]


def rms_seed(ncols, nrows):
    return ncols * 10 + nrows


def silu_spread(rng, n):
    """n float32 values spread over the whole fp16 range and past it (large, tiny, negative)"""
    return (rng.standard_normal(n) * np.exp2(rng.integers(-14, 15, n))).astype(np.float32)


def soft_max_rows(rng, ncols, nrows, scale_v=1.0):
    """float32 [nrows, ncols] soft_max inputs (before a scale by scale_v): N(0, 4) rows; the first has a range beyond
    65504 after the scale; the last carries -inf entries (never all of it); row 1 (nrows > 1) is negative throughout,
    in [-30, -5] after the scale, so a running maximum that starts at 0 instead of -inf changes its result"""
    x = (rng.standard_normal((nrows, ncols)) * 4).astype(np.float32)
    x[0, ::2] = f32(-70000.0 / scale_v)
    x[0, 0] = f32(3.0)
    if nrows > 1:
        x[1] = (rng.uniform(-30.0, -5.0, ncols) / scale_v).astype(np.float32)
    if ncols > 1:
        x[nrows - 1, 1::3] = -np.inf
    return x


def assert_bits(got, ref):
    """bitwise equality of two float32 arrays, reporting the first differences"""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape
    bad = np.flatnonzero(bits(got).ravel() != bits(ref).ravel())
    assert bad.size == 0, (bad.size, bad[:8], got.ravel()[bad[:8]], ref.ravel()[bad[:8]])


# rms_norm rows on which the rounding of each square matters: the float mean of the float-rounded squares (ggml.c's
# (ggml_float)(x * x)) differs from the float mean of the exact squares ((double)x * x) by enough to change the
# scale 1 / sqrtf(mean + eps), so a kernel that squares in double gives other output bits and is caught on purpose.
# {(ncols, with_add): seed of _rms_candidate(ncols, 0, seed)}, found by searching seeds upwards from 0;
# tests/test_ggml_ops_ref.py asserts the property and rms_order_free for each.
RMS_SQ_SEEDS = {(6, False): 17, (6, True): 15, (63, False): 115, (63, True): 108, (64, False): 58, (64, True): 3,
                (4098, False): 872, (4098, True): 512}


def rms_mean_exact_squares(x):
    """the float mean when every square is formed exactly in double: sum += (double)x * x in order"""
    x = np.asarray(x, np.float32).astype(np.float64)
    s = np.cumsum(x * x, axis=-1, dtype=np.float64)[..., -1]
    return (s / np.float64(x.shape[-1])).astype(np.float32)


def rms_norm_exact_squares(x):
    """rms_norm with that mean (what a kernel computes that squares in double)"""
    x = np.asarray(x, np.float32)
    mean = rms_mean_exact_squares(x)
    sc = (f32(1.0) / np.sqrt((mean + f32(1e-6)).astype(np.float32)).astype(np.float32)).astype(np.float32)
    return (x * sc[..., None]).astype(np.float32)


def rms_sq_row(ncols, with_add):
    """(a, b) float32 [1, ncols] from RMS_SQ_SEEDS"""
    a, b = _rms_candidate(ncols, 0, RMS_SQ_SEEDS[(ncols, with_add)])
    return a[None, :], b[None, :]
