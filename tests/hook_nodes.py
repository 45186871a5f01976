"""Test helper: hand-built ggml_tensor nodes driven through ggml_hip_compute_forward (the hook path), with
device-resident operands (ggml_hip_transform_tensor), device destinations (ggml_hip_assign_buffers_no_scratch)
and read-back through ggml_hip_memcpy_d2h, which flushes what the scheduler holds.  Arrays are numpy C-order:
shape (..., ne1, ne0)."""
import ctypes
import os
import re

import numpy as np

from hip_env import PKG, ggml_hip

# the op / type enums and the counter layout, read from the backend's own headers
_abi = open(os.path.join(PKG, "csrc", "ggml_abi.h")).read()
_OPS = {k: int(v) for k, v in re.findall(r"\bOP_(\w+) = (\d+)", _abi)}
OP_ADD, OP_MUL, OP_SILU, OP_RMS_NORM, OP_MUL_MAT, OP_SCALE, OP_CPY = (_OPS[k] for k in (
    "ADD", "MUL", "SILU", "RMS_NORM", "MUL_MAT", "SCALE", "CPY"))
OP_DIAG_MASK_INF, OP_SOFT_MAX, OP_ROPE = _OPS["DIAG_MASK_INF"], _OPS["SOFT_MAX"], _OPS["ROPE"]
TYPE_F32, TYPE_F16, TYPE_I32 = (int(re.search(r"\bTYPE_%s = (\d+)" % k, _abi).group(1)) for k in ("F32", "F16", "I32"))
# ggml_hip_debug_op_stats: per-op node counts first, fused launches per chain last
N_OPS = _OPS["COUNT"]
N_FUSED = int(re.search(r"constexpr int N_FUSED = (\d+);",
                        open(os.path.join(PKG, "csrc", "ggml-hip-internal.h")).read()).group(1))
ES = {TYPE_F32: 4, TYPE_F16: 2, TYPE_I32: 4}
# The scheduler's fusion switch has no getter, so the value restored after a test is a guess from the environment:
# on unless GGML_HIP_FUSE is set to something the backend's atoi reads as 0 (approximated here: "0", "" or a word
# that does not start with a digit or sign).
_f = os.environ.get("GGML_HIP_FUSE")
FUSE_DEFAULT = 1 if _f is None else (0 if not re.match(r"\s*[+-]?0*[1-9]", _f) else 1)


def op_stats(L, reset=True):
    """(nodes taken by the device per ggml op [68], fused launches per chain [15]), optionally reset"""
    L.ggml_hip_debug_op_stats.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    c = np.zeros(2 * N_OPS + 1 + N_FUSED, np.int64)
    ggml_hip.check(L.ggml_hip_debug_op_stats(c.ctypes.data, c.size, 1 if reset else 0), "op stats")
    return c[:N_OPS].copy(), c[-N_FUSED:].copy()


def set_fuse(L, on):
    L.ggml_hip_debug_set_fuse.argtypes = [ctypes.c_int]
    ggml_hip.check(L.ggml_hip_debug_set_fuse(1 if on else 0), "set_fuse")


def _tensor(gtype, ne, nb=None):
    """ggml_hip.make_tensor (contiguous F32 strides) extended to 4-d extents, F16 / I32 elements and given strides"""
    t = ggml_hip.make_tensor(ggml_hip.GGML_TYPE_F32, tuple(ne))
    t.type = gtype
    ne = [t.ne[i] for i in range(4)]
    t.n_dims = max(i + 1 for i in range(4) if ne[i] > 1 or i == 0)
    if nb is None:
        nb = [ES[gtype]]
        for i in range(3):
            nb.append(nb[i] * ne[i])
    nb = list(nb)
    while len(nb) < 4:                                      # missing outer strides: past everything inside
        nb.append(max(nb[j] * ne[j] for j in range(len(nb))))
    for i in range(4):
        t.nb[i] = nb[i]
    return t


class Nodes:
    """Owns the tensors of one hand-built node sequence; close() frees their device storage."""

    def __init__(self, L):
        self.L = L
        self.keep = []           # host arrays and tensors the C side points into
        self.owned = []

    def dev(self, arr, gtype=TYPE_F32):
        """a device-resident contiguous tensor holding arr (shape (..., ne1, ne0))"""
        arr = np.ascontiguousarray(arr)
        assert arr.dtype.itemsize == ES[gtype] and arr.ndim <= 4
        t = _tensor(gtype, arr.shape[::-1])
        t.backend = ggml_hip.GGML_BACKEND_GPU
        t.data = arr.ctypes.data
        self.L.ggml_hip_transform_tensor(arr.ctypes.data_as(ctypes.c_void_p), ctypes.byref(t))
        assert t.backend == ggml_hip.GGML_BACKEND_GPU and t.extra
        self.keep += [arr, t]
        self.owned.append(t)
        return t

    def host(self, arr, gtype):
        """a host tensor (the scalar parameters of scale / diag_mask_inf / rope)"""
        arr = np.ascontiguousarray(arr)
        t = _tensor(gtype, arr.shape[::-1])
        t.data = arr.ctypes.data
        self.keep += [arr, t]
        return t

    def view(self, base, ne, nb, gtype):
        """a strided view of a device tensor's storage"""
        t = _tensor(gtype, ne, nb)
        t.backend, t.data, t.extra = ggml_hip.GGML_BACKEND_GPU, base.data, base.extra
        self.keep.append(t)
        return t

    def node(self, op, src0, src1=None, inplace=False):
        """an F32 node of src0's shape with a device destination of its own, or (inplace) src0's buffer, as ggml's
        _inplace ops take it (the node's data is its source's)"""
        t = _tensor(TYPE_F32, list(src0.ne))
        t.op = op
        t.src0 = ctypes.pointer(src0)
        if src1 is not None:
            t.src1 = ctypes.pointer(src1)
        if inplace:
            t.data = src0.data
        else:
            buf = np.zeros(max(1, int(np.prod(list(src0.ne)))), np.float32)
            t.data = buf.ctypes.data
            self.keep.append(buf)
        self.L.ggml_hip_assign_buffers_no_scratch(ctypes.byref(t))
        assert t.backend == ggml_hip.GGML_BACKEND_GPU and t.extra
        self.keep.append(t)
        self.owned.append(t)
        return t

    def cpy_node(self, src0, target):
        """ggml_cpy(src0, target): a view of the target that shares its storage"""
        t = _tensor(target.type, list(target.ne), list(target.nb))
        t.op = OP_CPY
        t.src0, t.src1 = ctypes.pointer(src0), ctypes.pointer(target)
        t.backend, t.data, t.extra = ggml_hip.GGML_BACKEND_GPU, target.data, target.extra
        self.keep.append(t)
        return t

    def forward(self, t):
        p = ggml_hip.GgmlComputeParams()
        p.type, p.ith, p.nth = ggml_hip.GGML_TASK_COMPUTE, 0, 1
        assert self.L.ggml_hip_compute_forward(ctypes.byref(p), ctypes.byref(t)), "node not taken by the device"

    def read(self, t, shape, dtype=np.float32):
        out = np.empty(shape, dtype)
        dev = ctypes.cast(t.extra, ctypes.POINTER(ctypes.c_void_p * 16)).contents[0]
        ggml_hip.check(self.L.ggml_hip_memcpy_d2h(out.ctypes.data_as(ctypes.c_void_p), dev, out.nbytes, None), "d2h")
        return out

    def close(self):
        for t in reversed(self.owned):
            self.L.ggml_hip_free_data(ctypes.byref(t))
        self.owned = []
        if self.ring_size:
            self.L.ggml_hip_free_scratch()
            self.L.ggml_hip_set_scratch_size(0)          # the process default
            self.ring_size = 0

    # ---- placement in the VRAM scratch ring, by the product's own mechanism (ggml_hip_assign_buffers)
    ring_size = 0

    def ring_begin(self, size):
        """a fresh ring of `size` bytes: the next assignment lands at offset 0.  (set_scratch_size does not
        reallocate, so the old ring is freed first.)"""
        L = self.L
        L.ggml_hip_set_scratch_size.argtypes = [ctypes.c_size_t]
        L.ggml_hip_set_scratch_size.restype = None
        L.ggml_hip_free_scratch()
        L.ggml_hip_set_scratch_size(size)
        self.ring_size, self.ring_off = size, 0
        self.ring_gran = 65536                           # assign_buffers_impl's slot rule
        while self.ring_gran > 256 and self.ring_gran > size // 2048:
            self.ring_gran >>= 1
        probe = self._filler(0)                          # an empty tensor: allocates the ring, moves nothing
        self.ring_base = self.dev_ptr(probe)

    def dev_ptr(self, t):
        return ctypes.cast(t.extra, ctypes.POINTER(ctypes.c_void_p * 16)).contents[0]

    def _assign(self, t):
        """ggml_hip_assign_buffers(t), and where assign_buffers_impl's ring rule puts a tensor of its size"""
        size = int(np.prod([t.ne[i] for i in range(4)])) * ES[t.type]
        if self.ring_off + size > self.ring_size:
            self.ring_off = 0
        at = self.ring_off
        self.ring_off += (size + self.ring_gran - 1) & ~(self.ring_gran - 1)
        self.L.ggml_hip_assign_buffers(ctypes.byref(t))
        assert t.backend == ggml_hip.GGML_BACKEND_GPU and t.extra
        self.keep.append(t)
        self.owned.append(t)                             # (free_data only forgets the extra of a ring tensor)
        return at

    def _filler(self, nbytes):
        assert nbytes % 4 == 0
        t = _tensor(TYPE_F32, [nbytes // 4])
        t.ne[0] = nbytes // 4
        self._assign(t)
        return t

    def ring_place(self, t, off):
        """assign t (not in place, not a CPY) to the ring at byte `off`, steering there with throw-away filler
        assignments and the ring's wrap; asserts the device offset"""
        size = int(np.prod([t.ne[i] for i in range(4)])) * ES[t.type]
        assert off % self.ring_gran == 0 and off + size <= self.ring_size
        if self.ring_off > off:                          # run to the end: the next assignment wraps to 0
            if self.ring_off < self.ring_size:
                self._filler(self.ring_size - self.ring_off)
            self.ring_off = 0                            # (where the next non-empty assignment goes)
        if self.ring_off < off:
            self._filler(off - self.ring_off)
        assert self.ring_off == off, (self.ring_off, off)
        at = self._assign(t)
        assert at == off and self.dev_ptr(t) - self.ring_base == off, (at, off, self.dev_ptr(t) - self.ring_base)
        return t

    def blank(self, gtype, ne, nb=None, op=0):
        """a tensor struct with host data of its own (assign_buffers tells in-place nodes by equal data pointers)"""
        t = _tensor(gtype, ne, nb)
        t.op = op
        buf = np.zeros(8, np.uint8)
        t.data = buf.ctypes.data
        self.keep += [buf, t]
        return t

    def at(self, ptr, gtype, ne, nb=None, op=0, src0=None):
        """a device tensor (or view: reshape, cache window, PERMUTE with op and src0) at device address ptr"""
        t = self.blank(gtype, ne, nb, op)
        extra = (ctypes.c_void_p * 16)()
        extra[0] = ptr
        t.backend, t.extra = ggml_hip.GGML_BACKEND_GPU, ctypes.addressof(extra)
        if src0 is not None:
            t.src0 = ctypes.pointer(src0)
        self.keep.append(extra)
        return t

    def permute(self, src0, ne, nb):
        """a PERMUTE view of src0 with the given extents and strides"""
        return self.at(self.dev_ptr(src0), src0.type, ne, nb, _OPS["PERMUTE"], src0)

    def weight_q4_0(self, wq, k, m):
        """a resident q4_0 weight [m rows of k] (transform_tensor, BACKEND_GPU)"""
        wq = np.ascontiguousarray(wq, np.uint8)
        t = ggml_hip.make_tensor(ggml_hip.GGML_TYPE_Q4_0, (k, m), wq, backend=ggml_hip.GGML_BACKEND_GPU)
        self.L.ggml_hip_transform_tensor(wq.ctypes.data_as(ctypes.c_void_p), ctypes.byref(t))
        assert t.backend == ggml_hip.GGML_BACKEND_GPU and t.extra
        self.keep += [wq, t]
        self.owned.append(t)
        return t

    def op_tensor(self, op, ne, src0, src1=None, inplace=False):
        """an F32 node struct of extents ne, not yet placed; inplace: its data is src0's, as ggml's _inplace ops"""
        t = self.blank(TYPE_F32, ne, op=op)
        t.src0 = ctypes.pointer(src0)
        if src1 is not None:
            t.src1 = ctypes.pointer(src1)
        if inplace:
            t.data = src0.data
        return t

    def mm_q4_0(self, w, x):
        """a q4_0 MUL_MAT node struct (device x, device y once placed)"""
        return self.op_tensor(OP_MUL_MAT, [w.ne[1], x.ne[1]], w, x)

    def assign_inplace(self, t):
        """ggml_hip_assign_buffers of an in-place node: it takes its src0's device address"""
        want = self.dev_ptr(t.src0.contents)
        off = self.ring_off
        self.L.ggml_hip_assign_buffers(ctypes.byref(t))
        self.ring_off = off
        assert t.extra and self.dev_ptr(t) == want
        self.keep.append(t)
        self.owned.append(t)
        return t

    def upload(self, ptr, arr):
        arr = np.ascontiguousarray(arr)
        ggml_hip.check(self.L.ggml_hip_memcpy_h2d(ctypes.c_void_p(ptr), arr.ctypes.data_as(ctypes.c_void_p), arr.nbytes, None), "h2d")

    def download(self, ptr, nbytes):
        """device bytes (the read flushes what the scheduler holds)"""
        out = np.empty(nbytes, np.uint8)
        ggml_hip.check(self.L.ggml_hip_memcpy_d2h(out.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(ptr), nbytes, None), "d2h")
        return out


def _env_switch(name):
    v = os.environ.get(name)
    return 1 if v is None else (0 if not re.match(r"\s*[+-]?0*[1-9]", v) else 1)


class restore_switches:
    """with restore_switches(L): ... puts back the exact mode (its getter's value) and the fusion and fold switches
    (no getters: the defaults their environment variables give) on the way out"""

    def __init__(self, L):
        self.L = L

    def __enter__(self):
        self.exact = self.L.ggml_hip_get_exact()
        return self

    def __exit__(self, *exc):
        L = self.L
        L.ggml_hip_set_exact(self.exact)
        set_fuse(L, FUSE_DEFAULT)
        nf = os.environ.get("GGML_HIP_NORM_FOLD")
        nf = int(nf) if nf is not None and re.fullmatch(r"\s*[012]\s*", nf) else 1
        for fn, v in (("ggml_hip_debug_set_norm_fold", nf), ("ggml_hip_debug_set_epi_fold", _env_switch("GGML_HIP_GEMV_EPI")),
                      ("ggml_hip_debug_set_kq_fold", _env_switch("GGML_HIP_KQ_FOLD")),
                      ("ggml_hip_debug_set_x9_fold", _env_switch("GGML_HIP_X9_FOLD"))):
            f = getattr(L, fn)
            f.argtypes = [ctypes.c_int]
            f(v)
        return False
