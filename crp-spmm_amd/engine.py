"""Host-side mirror of the reference's engine API over the C ABI.

``RpSpmm`` ~ rp_spmm_*  (/root/reference/src/rowpara_spmm.h:60-87)
``Para2dSpmm`` ~ para2d_spmm_* (/root/reference/src/para2d_spmm.h:42-75)

Same argument names, meaning and call protocol (init -> exec ... -> print_stat
-> free) as the reference; B and C are torch tensors (device-resident: the
zero-copy path) or numpy arrays (host pointers, staged like the reference API).
"""
import ctypes as C

import numpy as np

from . import _lib as L
from .hip import _check_dev_vectors, _softmax_vecs


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _ip(a):
    return a.ctypes.data_as(L.c_int_p)


def _dp(a):
    return a.ctypes.data_as(L.c_dbl_p)


def _dtype_of(x):
    """"f64" / "f32" for a 2-D float64 / float32 torch tensor or numpy array; TypeError for anything else."""
    try:
        import torch
        if isinstance(x, torch.Tensor):
            if x.dim() == 2 and x.dtype in (torch.float64, torch.float32):
                return "f64" if x.dtype == torch.float64 else "f32"
            raise TypeError("B and C must be 2-D float64 or float32, got %s of %d dimensions" % (x.dtype, x.dim()))
    except ImportError:
        pass
    if isinstance(x, np.ndarray) and x.ndim == 2 and x.dtype in (np.float64, np.float32):
        return "f64" if x.dtype == np.float64 else "f32"
    raise TypeError("B and C must be 2-D float64 or float32 torch tensors or numpy arrays")


def _operands_dtype(B, C_out):
    """The dtype B and C share ("f64" or "f32"); TypeError when they differ or are neither (before any C call)."""
    db, dc = _dtype_of(B), _dtype_of(C_out)
    if db != dc:
        raise TypeError("B and C must have the same dtype (B is %s, C is %s)" % (db, dc))
    return db


def _ptr_ld(x, layout, f32=False):
    """(address, leading dimension, keepalive) of a 2-D float64 (f32: float32) operand."""
    name, isz = ("float32", 4) if f32 else ("float64", 8)
    try:
        import torch
        if isinstance(x, torch.Tensor):
            if x.dtype != (torch.float32 if f32 else torch.float64) or x.dim() != 2:
                raise TypeError("B and C must be 2-D %s" % name)
            if x.numel() == 0:          # (as below: a tensor made from an empty numpy array keeps its strides of 0)
                return x.data_ptr(), max(int(x.stride(0)), int(x.shape[1]), 1), x
            if x.stride(1) != 1:
                raise ValueError("operand must be contiguous along its fast dimension")
            return x.data_ptr(), x.stride(0), x
    except ImportError:
        pass
    if isinstance(x, np.ndarray) and x.dtype == np.dtype(name) and x.ndim == 2 and x.size == 0:
        # a rank without rows: numpy gives an array without elements strides of 0; nothing of it is read (csrc/operand_view.h), and its
        # leading dimension is its row length
        return x.ctypes.data, max(int(x.shape[1]), 1), x
    if not isinstance(x, np.ndarray) or x.dtype != np.dtype(name) or x.ndim != 2 or x.strides[1] != isz:
        raise TypeError("B and C must be 2-D %s torch tensors or numpy arrays, contiguous along the fast dimension" % name)
    return x.ctypes.data, x.strides[0] // isz, x


def _out_ptr(out, f32, nnz):
    """(address, keepalive) of the 1-D contiguous float64 (f32: float32) result of ``sddmm``, which must hold nnz entries."""
    name = "float32" if f32 else "float64"
    try:
        import torch
        if isinstance(out, torch.Tensor):
            if out.dtype != (torch.float32 if f32 else torch.float64) or out.dim() != 1:
                raise TypeError("out must be 1-D %s, like the operands" % name)
            if not out.is_contiguous():
                raise ValueError("out must be contiguous")
            if out.numel() != nnz:
                raise ValueError("out has %d entries, this rank's rows of A %d nonzeros" % (out.numel(), nnz))
            return out.data_ptr() or None, out
    except ImportError:
        pass
    if not isinstance(out, np.ndarray) or out.dtype != np.dtype(name) or out.ndim != 1:
        raise TypeError("out must be a 1-D %s torch tensor or numpy array, like the operands" % name)
    if not out.flags.c_contiguous or not out.flags.writeable:
        raise ValueError("out must be contiguous and writeable")
    if out.size != nnz:
        raise ValueError("out has %d entries, this rank's rows of A %d nonzeros" % (out.size, nnz))
    return out.ctypes.data or None, out


def _vec_ptr(name, x, f32, count):
    """(address, keepalive) of an optional 1-D contiguous float64 (f32: float32) result of ``attention`` with ``count`` entries,
    on the host or the device; (None, None) for None."""
    if x is None:
        return None, None
    dname = "float32" if f32 else "float64"
    try:
        import torch
        if isinstance(x, torch.Tensor):
            if x.dtype != (torch.float32 if f32 else torch.float64) or x.dim() != 1:
                raise TypeError("%s must be 1-D %s, like the operands" % (name, dname))
            if not x.is_contiguous() or x.numel() != count:
                raise ValueError("%s must be contiguous with %d entries" % (name, count))
            return x.data_ptr() or None, x
    except ImportError:
        pass
    if not isinstance(x, np.ndarray) or x.dtype != np.dtype(dname) or x.ndim != 1:
        raise TypeError("%s must be a 1-D %s torch tensor or numpy array, like the operands" % (name, dname))
    if not x.flags.c_contiguous or not x.flags.writeable or x.size != count:
        raise ValueError("%s must be contiguous and writeable with %d entries" % (name, count))
    return x.ctypes.data or None, x


def _engine_heads(heads, glb_n):
    """``heads`` of the engine's attention calls as an int >= 1 that divides glb_n, checked before any library call"""
    if isinstance(heads, bool) or not isinstance(heads, (int, np.integer)):
        raise TypeError("heads must be an int, got %r" % (heads,))
    if heads < 1:
        raise ValueError("heads must be at least 1, got %d" % heads)
    if glb_n % heads:
        raise ValueError("%d heads do not divide the engine's %d columns" % (heads, glb_n))
    return int(heads)


def _mh_vec(name, x, heads):
    """A per-row or per-nonzero result of a multi-head call -- C-contiguous, (rows, heads) -- as the flat view the single-head
    checks take; ``heads`` = 1 and None pass through."""
    if heads == 1 or x is None:
        return x
    ndim = x.dim() if hasattr(x, "dim") else getattr(x, "ndim", None)
    if ndim != 2 or x.shape[1] != heads:
        raise ValueError("%s must be 2-D with %d columns (one per head)" % (name, heads))
    if not (x.is_contiguous() if hasattr(x, "is_contiguous") else x.flags.c_contiguous):
        raise ValueError("%s must be contiguous" % name)
    return x.view(-1) if hasattr(x, "is_contiguous") else x.reshape(-1)


def _f32_operands(B, C_out):
    """TypeError unless B and C are both float32 (``exec_t_f32``), before any C call."""
    if _operands_dtype(B, C_out) != "f32":
        raise TypeError("exec_t_f32 is fp32 only: B and C must be float32")


def _dev_vals(vals, nnz):
    """(address, f32 flag, keepalive) of the 1-D contiguous float64 / float32 CUDA tensor ``update_values_dev`` takes, which must
    hold nnz entries; TypeError for anything that is not such a tensor on the device, ValueError for a wrong length or strides
    (hip._check_dev_vectors, the checker the row softmax shares)."""
    import torch
    _check_dev_vectors((("vals", vals),), nnz)
    return vals.data_ptr() or None, int(vals.dtype == torch.float32), vals


def _check_blocks(layout, n, blocks):
    """ValueError unless every (name, operand, rows) is a rows x n block (layout 1: (n, ld >= rows)): the kernels index the
    operands by the plan's sizes, a wrong shape would be an out-of-bounds device access.  rows None: not known, not checked."""
    for name, x, rows in blocks:
        if rows is None:
            continue
        want = (rows, n) if layout == 0 else (n, rows)
        got = tuple(x.shape)
        if (layout == 0 and (got[0] < want[0] or got[1] != want[1])) or \
           (layout == 1 and (got[0] != want[0] or got[1] < want[1])):
            raise ValueError("%s has shape %s, the engine needs %s (layout %d)" % (name, got, want, layout))


def _current_stream(x):
    try:
        import torch
        if isinstance(x, torch.Tensor) and x.is_cuda:
            return torch.cuda.current_stream(x.device).cuda_stream
    except ImportError:
        pass
    return None


class RpSpmm:
    """1D row-parallel SpMM engine: C := A * B with A's row block on this rank.

    Arguments as rp_spmm_init (src/rowpara_spmm.h:49-64): ``A_rowptr`` is this
    rank's slice of the GLOBAL row pointer (global nnz offsets), ``B_row_displs``
    has nproc + 1 entries, ``comm`` is a TorchComm / SelfComm and must outlive
    the engine."""

    def __init__(self, A_srow, A_nrow, A_rowptr, A_colidx, A_val, B_row_displs, glb_n, comm, plan_only=False):
        lib = L.load()
        self._lib = lib
        self.comm = comm
        rp, ci, va, bd = _i32(A_rowptr), _i32(A_colidx), _f64(A_val), _i32(B_row_displs)
        if ci.size == 0:
            ci, va = np.zeros(1, np.int32), np.zeros(1, np.float64)
        self.handle = C.c_void_p()
        fn = lib.crp_rp_spmm_init_plan_only if plan_only else lib.crp_rp_spmm_init
        fn(A_srow, A_nrow, _ip(rp), _ip(ci), _dp(va), _ip(bd), glb_n, comm.ptr, C.byref(self.handle))
        self.glb_n = glb_n
        self.A_nrow = A_nrow
        self.loc_B_nrow = int(bd[comm.rank + 1] - bd[comm.rank])
        self._owned = True

    @classmethod
    def _wrap(cls, handle, comm, lib):
        self = cls.__new__(cls)
        self._lib, self.comm, self.handle, self._owned = lib, comm, C.c_void_p(handle), False
        v = self.plan_view()
        self.glb_n, self.A_nrow = v.glb_n, v.A_nrow
        return self

    def exec(self, BC_layout, B, C_out, stream=None):
        """rp_spmm_exec (src/rowpara_spmm.h:69-81); ldB / ldC come from the strides.
        For layout 1 pass the operands as (n, ld) arrays holding the column-major data.
        float64 operands run the fp64 exec, float32 operands the fp32 exec (crp_rp_spmm_exec_f32_ex)."""
        f32 = _operands_dtype(B, C_out) == "f32"
        bp, ldb, _kb = _ptr_ld(B, BC_layout, f32)
        cp, ldc, _kc = _ptr_ld(C_out, BC_layout, f32)
        _check_blocks(BC_layout, self.glb_n, (("B", B, getattr(self, "loc_B_nrow", None)), ("C", C_out, self.A_nrow)))
        if stream is None:
            stream = _current_stream(C_out)
        fn = self._lib.crp_rp_spmm_exec_f32_ex if f32 else self._lib.crp_rp_spmm_exec_ex
        fn(self.handle, BC_layout, bp, ldb, cp, ldc, stream)

    def _exec_t(self, f32, BC_layout, B, C_out, stream):
        bp, ldb, _kb = _ptr_ld(B, BC_layout, f32)
        cp, ldc, _kc = _ptr_ld(C_out, BC_layout, f32)
        _check_blocks(BC_layout, self.glb_n, (("B", B, self.A_nrow), ("C", C_out, getattr(self, "loc_B_nrow", None))))
        if stream is None:
            stream = _current_stream(C_out)
        fn = self._lib.crp_rp_spmm_exec_t_f32_ex if f32 else self._lib.crp_rp_spmm_exec_t_ex
        fn(self.handle, BC_layout, bp, ldb, cp, ldc, stream)

    def exec_t(self, BC_layout, B, C_out, stream=None):
        """C := A^T * B (crp_rp_spmm_exec_t_ex), fp64 only: B is this rank's A_nrow x glb_n block (partitioned like A's
        rows), C_out its loc_B_nrow x glb_n block of the result (partitioned by B_row_displs); layouts and operands as
        ``exec``.  The first call builds the transposed device matrices (``transposed_built``)."""
        if _operands_dtype(B, C_out) != "f64":
            raise TypeError("exec_t is fp64 only: B and C must be float64")
        self._exec_t(False, BC_layout, B, C_out, stream)

    def exec_t_f32(self, BC_layout, B, C_out, stream=None):
        """C := A^T * B in fp32 (crp_rp_spmm_exec_t_f32_ex): float32 operands only, shapes and layouts as ``exec_t``.  The
        transposed device matrices are the ones ``exec_t`` builds; whichever is called first builds them."""
        _f32_operands(B, C_out)
        self._exec_t(True, BC_layout, B, C_out, stream)

    def sddmm(self, BC_layout, X, Y, out, mode=0, stream=None):
        """Sampled dense-dense product over this rank's rows of A (crp_rp_spmm_sddmm_ex / _f32_ex, by the operands' dtype):
        out[p] = <X[i], Y[c]> for every local nonzero p = (i, c), in the order of the A_val given to init; mode 1: times
        the engine's current value of p.  X is this rank's A_nrow x glb_n block, Y its loc_B_nrow x glb_n block (layouts and
        operands as ``exec``), ``out`` a 1-D array or tensor of nnz entries of the same dtype, on the host or the device.
        Mixed dtypes, wrong shapes and a wrong ``out`` length raise before the library is called."""
        dt = _operands_dtype(X, Y)
        f32 = dt == "f32"
        if mode not in (0, 1):
            raise ValueError("mode must be 0 or 1, got %r" % (mode,))
        xp, ldx, _kx = _ptr_ld(X, BC_layout, f32)
        yp, ldy, _ky = _ptr_ld(Y, BC_layout, f32)
        _check_blocks(BC_layout, self.glb_n, (("X", X, self.A_nrow), ("Y", Y, getattr(self, "loc_B_nrow", None))))
        op, _ko = _out_ptr(out, f32, self.nnz())
        if stream is None:
            stream = _current_stream(out)
        if stream is None:
            stream = _current_stream(X)
        fn = self._lib.crp_rp_spmm_sddmm_f32_ex if f32 else self._lib.crp_rp_spmm_sddmm_ex
        fn(self.handle, BC_layout, xp, ldx, yp, ldy, op, int(mode), stream)

    @property
    def sddmm_built(self):
        """True once a ``sddmm`` has uploaded the positions its row parts write through (crp_rp_spmm_sddmm_built)."""
        return bool(self._lib.crp_rp_spmm_sddmm_built(self.handle))

    def attention(self, layout, Q, K, V, out, scale=1.0, bias=False, lse=None, p_out=None, stream=None, heads=1):
        """Fused sparse attention over this rank's rows of A (crp_rp_spmm_attention_ex / _f32_ex, by the operands' dtype):
        out[i] = sum_p softmax_p(scale * <Q[i], K[c_p]> (+ the engine's current value of p with ``bias``)) * V[c_p] over the
        nonzeros p = (i, c_p) of row i.  Q and ``out`` are this rank's A_nrow x glb_n blocks, K and V its loc_B_nrow x glb_n
        blocks (layouts and operands as ``exec``); ``lse`` (A_nrow entries) and ``p_out`` (nnz entries in the order of the A_val
        given to init) are optional 1-D arrays or tensors of the same dtype, on the host or the device.  The engine's values
        are not changed.  Mixed dtypes, wrong shapes and wrong lengths raise before the library is called.
        ``heads`` > 1 (crp_rp_spmm_attention_mh_ex / _f32_ex): glb_n / heads columns per head, side by side; ``lse`` is then a
        contiguous (A_nrow, heads) array and ``p_out`` a contiguous (nnz, heads) one.  ``heads`` must divide glb_n."""
        heads = _engine_heads(heads, self.glb_n)
        dt = _operands_dtype(Q, K)
        if _operands_dtype(V, out) != dt:
            raise TypeError("Q, K, V and out must have the same dtype")
        f32 = dt == "f32"
        if bias not in (False, True, 0, 1):
            raise ValueError("bias must be a bool, got %r" % (bias,))
        scale = float(scale)
        if not np.isfinite(scale):
            raise ValueError("scale must be finite, got %r" % (scale,))
        qp, ldq, _kq = _ptr_ld(Q, layout, f32)
        kp, ldk, _kk = _ptr_ld(K, layout, f32)
        vp, ldv, _kv = _ptr_ld(V, layout, f32)
        op, ldo, _ko = _ptr_ld(out, layout, f32)
        kb = getattr(self, "loc_B_nrow", None)
        _check_blocks(layout, self.glb_n, (("Q", Q, self.A_nrow), ("K", K, kb), ("V", V, kb), ("out", out, self.A_nrow)))
        lp, _kl = _vec_ptr("lse", _mh_vec("lse", lse, heads), f32, self.A_nrow * heads)
        pp, _kp = _vec_ptr("p_out", _mh_vec("p_out", p_out, heads), f32, self.nnz() * heads)
        if stream is None:
            stream = _current_stream(out)
        if stream is None:
            stream = _current_stream(Q)
        fn, mh = L.attention_entry(self._lib, "rp_spmm_attention", heads, f32)
        fn(self.handle, layout, *mh, scale, int(bool(bias)), qp, ldq, kp, ldk, vp, ldv, op, ldo, lp, pp, stream)

    def attention_built(self):
        """True once an ``attention`` has allocated V's receive buffer (crp_rp_spmm_attention_built)."""
        return bool(self._lib.crp_rp_spmm_attention_built(self.handle))

    def gat_attention(self, layout, el, er, V, out, slope=0.2, bias=False, lse=None, p_out=None, stream=None, heads=1):
        """Fused GAT attention over this rank's rows of A (crp_rp_spmm_gat_ex / _f32_ex, by the operands' dtype): for every head h,
        out[i]_h = sum_p softmax_p(leaky_relu(el[i, h] + er[c_p, h], slope) (+ the engine's current value of p with ``bias``))
        * V[c_p]_h over the nonzeros p = (i, c_p) of row i.  V and ``out`` are this rank's loc_B_nrow x glb_n and A_nrow x glb_n
        blocks (layouts and operands as ``exec``) with glb_n / heads columns per head; ``el`` (A_nrow, heads) and ``er``
        (loc_B_nrow, heads) are row-major torch tensors on the device; ``lse`` (A_nrow, heads) and ``p_out`` (nnz, heads), in the
        order of the A_val given to init, are optional contiguous arrays or tensors on the host or the device (1-D with one
        head).  The engine's values are not changed.  Every error is raised before the library is called."""
        import torch
        heads = _engine_heads(heads, self.glb_n)
        dt = _operands_dtype(V, out)
        f32 = dt == "f32"
        want = torch.float32 if f32 else torch.float64
        kb = getattr(self, "loc_B_nrow", None)
        for name, t, rows in (("el", el, self.A_nrow), ("er", er, kb)):
            if not isinstance(t, torch.Tensor):
                raise TypeError("%s must be a torch tensor on the device" % name)
            if t.dtype != want:
                raise TypeError("%s must have the dtype of V and out (%s is %s)" % (name, name, t.dtype))
            if t.dim() != 2:
                raise TypeError("%s must be 2-D" % name)
            if t.shape[1] != heads or (rows is not None and t.shape[0] < rows):
                raise ValueError("%s is %s, this rank needs (%s, %d)" % (name, tuple(t.shape), rows, heads))
            if t.shape[1] > 1 and t.stride(1) != 1:
                raise ValueError("%s must be contiguous along its rows" % name)
        if bias not in (False, True, 0, 1):
            raise ValueError("bias must be a bool, got %r" % (bias,))
        slope = float(slope)
        if not np.isfinite(slope):
            raise ValueError("slope must be finite, got %r" % (slope,))
        vp, ldv, _kv = _ptr_ld(V, layout, f32)
        op, ldo, _ko = _ptr_ld(out, layout, f32)
        _check_blocks(layout, self.glb_n, (("V", V, kb), ("out", out, self.A_nrow)))
        lp, _kl = _vec_ptr("lse", _mh_vec("lse", lse, heads), f32, self.A_nrow * heads)
        pp, _kp = _vec_ptr("p_out", _mh_vec("p_out", p_out, heads), f32, self.nnz() * heads)
        for name, t in (("el", el), ("er", er)):
            if not t.is_cuda:
                raise TypeError("%s must be on the device" % name)
        if stream is None:
            stream = _current_stream(out)
        if stream is None:
            stream = _current_stream(el)
        fn = self._lib.crp_rp_spmm_gat_f32_ex if f32 else self._lib.crp_rp_spmm_gat_ex
        fn(self.handle, layout, heads, slope, int(bool(bias)), el.data_ptr() or None, max(el.stride(0), heads), er.data_ptr() or None,
           max(er.stride(0), heads), vp, ldv, op, ldo, lp, pp, stream)

    def gat_built(self):
        """True once a ``gat_attention`` has set up the narrow exchange of er (crp_rp_spmm_gat_built)."""
        return bool(self._lib.crp_rp_spmm_gat_built(self.handle))

    def gatv2_attention(self, layout, XT, a, XS, out, slope=0.2, bias=False, lse=None, p_out=None, stream=None, heads=1):
        """Fused GATv2 attention over this rank's rows of A (crp_rp_spmm_gatv2_ex / _f32_ex, by the operands' dtype): for every head
        h, out[i]_h = sum_p softmax_p(sum_j a[h, j] leaky_relu(XT[i]_h[j] + XS[c_p]_h[j], slope) (+ the engine's current value of p
        with ``bias``)) * XS[c_p]_h over the nonzeros p = (i, c_p) of row i.  XS and ``out`` are this rank's loc_B_nrow x glb_n and
        A_nrow x glb_n blocks (layouts and operands as ``exec``) with glb_n / heads columns per head; XS travels as B does.  ``XT``
        (A_nrow, glb_n), row-major, and ``a`` (glb_n contiguous elements, 1-D or (heads, dv)) are torch tensors on the device;
        ``lse`` (A_nrow, heads) and ``p_out`` (nnz, heads), in the order of the A_val given to init, are optional contiguous
        arrays or tensors on the host or the device (1-D with one head).  The engine's values are not changed.  Every error is
        raised before the library is called."""
        import torch
        heads = _engine_heads(heads, self.glb_n)
        dt = _operands_dtype(XS, out)
        f32 = dt == "f32"
        want = torch.float32 if f32 else torch.float64
        for name, t in (("XT", XT), ("a", a)):
            if not isinstance(t, torch.Tensor):
                raise TypeError("%s must be a torch tensor on the device" % name)
            if t.dtype != want:
                raise TypeError("%s must have the dtype of XS and out (%s is %s)" % (name, name, t.dtype))
        if XT.dim() != 2:
            raise TypeError("XT must be 2-D")
        if XT.shape[1] != self.glb_n or XT.shape[0] < self.A_nrow:
            raise ValueError("XT is %s, this rank needs (%d, %d)" % (tuple(XT.shape), self.A_nrow, self.glb_n))
        if XT.shape[1] > 1 and XT.stride(1) != 1:
            raise ValueError("XT must be contiguous along its rows")
        if a.dim() not in (1, 2) or a.numel() != self.glb_n or not a.is_contiguous() or (a.dim() == 2 and a.shape[0] != heads):
            raise ValueError("a must hold glb_n = %d contiguous elements, 1-D or (heads, dv); it is %s" % (self.glb_n, tuple(a.shape)))
        cap = 4 * 64 * (4 if f32 else 2)
        if self.glb_n // heads > cap:
            raise ValueError("the fused GATv2 attention takes at most %d columns per head (dv = %d)" % (cap, self.glb_n // heads))
        if bias not in (False, True, 0, 1):
            raise ValueError("bias must be a bool, got %r" % (bias,))
        slope = float(slope)
        if not np.isfinite(slope):
            raise ValueError("slope must be finite, got %r" % (slope,))
        kb = getattr(self, "loc_B_nrow", None)
        xp, ldx, _kx = _ptr_ld(XS, layout, f32)
        op, ldo, _ko = _ptr_ld(out, layout, f32)
        _check_blocks(layout, self.glb_n, (("XS", XS, kb), ("out", out, self.A_nrow)))
        lp, _kl = _vec_ptr("lse", _mh_vec("lse", lse, heads), f32, self.A_nrow * heads)
        pp, _kp = _vec_ptr("p_out", _mh_vec("p_out", p_out, heads), f32, self.nnz() * heads)
        for name, t in (("XT", XT), ("a", a)):
            if not t.is_cuda:
                raise TypeError("%s must be on the device" % name)
        if stream is None:
            stream = _current_stream(out)
        if stream is None:
            stream = _current_stream(XT)
        fn = self._lib.crp_rp_spmm_gatv2_f32_ex if f32 else self._lib.crp_rp_spmm_gatv2_ex
        fn(self.handle, layout, heads, slope, int(bool(bias)), XT.data_ptr() or None, max(XT.stride(0), self.glb_n), a.data_ptr() or None,
           xp, ldx, op, ldo, lp, pp, stream)

    def gatv2_built(self):
        """True once a ``gatv2_attention`` has uploaded the parts' positions (crp_rp_spmm_gatv2_built)."""
        return bool(self._lib.crp_rp_spmm_gatv2_built(self.handle))

    def attention_bwd(self, Q, K, V, O, dO, lse, dQ, dK, dV, scale=1.0, bias=False, ds_out=None, stream=None, heads=1):
        """The fused backward of ``attention`` over this rank's rows of A (crp_rp_spmm_attention_bwd_ex / _f32_ex, by the operands'
        dtype): with ``O`` and ``lse`` as the forward wrote them and the upstream gradient ``dO``, writes dQ (A_nrow x glb_n), dK
        and dV (loc_B_nrow x glb_n) and optionally ``ds_out`` (nnz entries in A_val's order: the gradient of the bias).  Every
        operand is a row-major torch tensor on the device; host arrays and layout 1 are not offered.  glb_n is at most 512
        (float64) / 1024 (float32).  Wrong types, dtypes, shapes and devices raise before the library is called.
        ``heads`` > 1 (crp_rp_spmm_attention_bwd_mh_ex / _f32_ex): glb_n / heads columns per head, to which the cap applies;
        ``lse`` is a contiguous (A_nrow, heads) tensor and ``ds_out`` a contiguous (nnz, heads) one.  ``heads`` must divide
        glb_n."""
        import torch
        heads = _engine_heads(heads, self.glb_n)
        if isinstance(lse, torch.Tensor):
            lse = _mh_vec("lse", lse, heads)
        if isinstance(ds_out, torch.Tensor):
            ds_out = _mh_vec("ds_out", ds_out, heads)
        two_d = (("Q", Q, self.A_nrow), ("O", O, self.A_nrow), ("dO", dO, self.A_nrow), ("dQ", dQ, self.A_nrow),
                 ("K", K, getattr(self, "loc_B_nrow", None)), ("V", V, getattr(self, "loc_B_nrow", None)),
                 ("dK", dK, getattr(self, "loc_B_nrow", None)), ("dV", dV, getattr(self, "loc_B_nrow", None)))
        vecs = (("lse", lse, self.A_nrow * heads),) + ((("ds_out", ds_out, self.nnz() * heads),) if ds_out is not None else ())
        for name, t, _ in two_d + vecs:
            if not isinstance(t, torch.Tensor):
                raise TypeError("%s must be a torch tensor on the device" % name)
            if t.dtype not in (torch.float64, torch.float32) or t.dtype != Q.dtype:
                raise TypeError("the operands must be float64 or float32, all alike (%s is %s)" % (name, t.dtype))
        for name, t, rows in two_d:
            if t.dim() != 2:
                raise TypeError("%s must be 2-D" % name)
            if t.shape[1] != self.glb_n or (rows is not None and t.shape[0] != rows):
                raise ValueError("%s is %s, this rank needs (%s, %d)" % (name, tuple(t.shape), rows, self.glb_n))
            if t.shape[1] > 1 and t.stride(1) != 1:
                raise ValueError("%s must be contiguous along its rows" % name)
        for name, t, count in vecs:
            if t.dim() != 1 or not t.is_contiguous() or t.numel() != count:
                raise ValueError("%s must be 1-D and contiguous with %d entries" % (name, count))
        if bias not in (False, True, 0, 1):
            raise ValueError("bias must be a bool, got %r" % (bias,))
        scale = float(scale)
        if not np.isfinite(scale):
            raise ValueError("scale must be finite, got %r" % (scale,))
        cap = 512 if Q.dtype == torch.float64 else 1024
        if self.glb_n // heads > cap:
            raise ValueError("the fused backward takes at most %d columns%s in %s, this engine has %d"
                             % (cap, "" if heads == 1 else " per head", Q.dtype, self.glb_n // heads))
        for name, t, _ in two_d + vecs:
            if not t.is_cuda or t.device != Q.device:
                raise TypeError("%s must be on the device, with Q" % name)
        if stream is None:
            stream = _current_stream(dQ)
        ptr = lambda t: (t.data_ptr() or None) if t is not None else None
        fn, mh = L.attention_entry(self._lib, "rp_spmm_attention_bwd", heads, Q.dtype == torch.float32)
        fn(self.handle, *mh, scale, int(bool(bias)), ptr(Q), Q.stride(0), ptr(K), K.stride(0), ptr(V), V.stride(0), ptr(O), O.stride(0), ptr(dO),
           dO.stride(0), ptr(lse), ptr(dQ), dQ.stride(0), ptr(dK), dK.stride(0), ptr(dV), dV.stride(0), ptr(ds_out), stream)

    def attention_bwd_built(self):
        """True once an ``attention_bwd`` has allocated the engine's delta (crp_rp_spmm_attention_bwd_built)."""
        return bool(self._lib.crp_rp_spmm_attention_bwd_built(self.handle))

    @property
    def transposed_built(self):
        """True once an ``exec_t`` has built the transposed device matrices (crp_rp_spmm_transposed_built)."""
        return bool(self._lib.crp_rp_spmm_transposed_built(self.handle))

    def print_stat(self):
        self._lib.crp_rp_spmm_print_stat(self.handle)

    def clear_stat(self):
        self._lib.crp_rp_spmm_clear_stat(self.handle)

    def set_timing(self, on):
        self._lib.crp_rp_spmm_set_timing(self.handle, int(bool(on)))

    def kernel_info(self):
        """-> dict(variant, variant_name, reordered, lattice) of the local SpMM (crp_rp_spmm_kernel_info)."""
        v, ro, la = C.c_int(), C.c_int(), C.c_int()
        self._lib.crp_rp_spmm_kernel_info(self.handle, C.byref(v), C.byref(ro), C.byref(la))
        name = self._lib.crp_spmm_variant_name(v.value)
        return dict(variant=v.value, variant_name=name.decode() if name else None, reordered=bool(ro.value), lattice=bool(la.value))

    def set_variant(self, variant):
        self._lib.crp_rp_spmm_set_variant(self.handle, int(variant))

    def set_variant_f32(self, variant):
        """Kernel variant of the fp32 exec: 0 auto (default), 1 row-group, 5 team kernel."""
        if int(variant) not in (0, 1, 5):
            raise ValueError("fp32 variant must be 0, 1 or 5, got %r" % (variant,))
        self._lib.crp_rp_spmm_set_variant_f32(self.handle, int(variant))

    def overlap_rows(self):
        """(interior rows, boundary rows) of the exchange / compute overlap split; (0, 0) when off."""
        a, b = C.c_int(), C.c_int()
        self._lib.crp_rp_spmm_overlap_rows(self.handle, C.byref(a), C.byref(b))
        return a.value, b.value

    def update_values(self, A_val):
        va = _f64(A_val)
        self._lib.crp_rp_spmm_update_values(self.handle, _dp(va))

    def update_values_dev(self, vals, stream=None):
        """New values from device memory (crp_rp_spmm_update_values_dev): a 1-D contiguous float64 or float32 CUDA tensor of
        ``nnz()`` entries in the order of the A_val given to init -- what ``sddmm`` writes.  Asynchronous on ``stream`` (default:
        the current torch stream of the tensor's device); nothing leaves the device.  ``host_values_stale`` turns true."""
        ptr, f32, _keep = _dev_vals(vals, self.nnz())
        if stream is None:
            stream = _current_stream(vals)
        self._lib.crp_rp_spmm_update_values_dev(self.handle, ptr, f32, stream)

    def row_softmax(self, s, out=None, stream=None):
        """Row softmax over this rank's rows of A (crp_rp_spmm_row_softmax_ex): out[p] = exp(s[p] - max) / sum over every row's
        nonzeros.  ``s`` is a 1-D contiguous float64 or float32 CUDA tensor of ``nnz()`` entries in the order of the A_val given to
        init -- what ``sddmm`` writes and ``update_values_dev`` takes; ``out`` one like it (allocated when None; ``out is s`` is
        allowed).  Asynchronous on ``stream`` (default: the current torch stream), no communication, not collective; -inf entries
        are masked edges.  Every argument is checked before the library is called.  Returns ``out``."""
        s, out = _softmax_vecs((("s", s),), out, self.nnz())
        if stream is None:
            stream = _current_stream(out)
        f32 = int(s.dtype.itemsize == 4)
        self._lib.crp_rp_spmm_row_softmax_ex(self.handle, s.data_ptr() or None, out.data_ptr() or None, f32, stream)
        return out

    def row_softmax_bwd(self, y, dy, out=None, stream=None):
        """The Jacobian product of ``row_softmax`` (crp_rp_spmm_row_softmax_bwd_ex): out[p] = y[p] * (dy[p] - D), D = the row's
        sum of y * dy.  Tensors as in ``row_softmax``, one dtype; ``out`` may be ``dy`` or ``y``.  Returns ``out``."""
        y, dy, out = _softmax_vecs((("y", y), ("dy", dy)), out, self.nnz())
        if stream is None:
            stream = _current_stream(out)
        f32 = int(y.dtype.itemsize == 4)
        self._lib.crp_rp_spmm_row_softmax_bwd_ex(self.handle, y.data_ptr() or None, dy.data_ptr() or None, out.data_ptr() or None, f32, stream)
        return out

    @property
    def row_softmax_built(self):
        """True once a ``row_softmax`` / ``row_softmax_bwd`` has uploaded the row pointer (crp_rp_spmm_row_softmax_built)."""
        return bool(self._lib.crp_rp_spmm_row_softmax_built(self.handle))

    @property
    def host_values_stale(self):
        """True after ``update_values_dev`` until the host values are read (``plan``) or replaced (``update_values``)."""
        return bool(self._lib.crp_rp_spmm_host_values_stale(self.handle))

    def alg_bytes(self):
        return int(self._lib.crp_rp_spmm_alg_bytes(self.handle))

    def alg_bytes_f32(self):
        return int(self._lib.crp_rp_spmm_alg_bytes_f32(self.handle))

    def nnz(self):
        return int(self._lib.crp_rp_spmm_nnz(self.handle))

    def plan_view(self):
        v = L.RpPlanView()
        self._lib.crp_rp_spmm_get_plan(self.handle, C.byref(v))
        return v

    def plan(self):
        """The struct's plan fields (src/rowpara_spmm.h:8-40) as numpy copies."""
        v = self.plan_view()
        P, nnz = v.nproc, self.nnz()

        def arr(p, n, dt):
            return np.ctypeslib.as_array(p, (n,)).astype(dt).copy() if n > 0 else np.zeros(0, dt)
        d = {k: getattr(v, k) for k in ("nproc", "my_rank", "glb_n", "A_nrow", "rB_nrow", "rB_self_src_offset",
                                        "rB_self_dst_offset", "rB_self_nrow", "rB_p2p", "rB_reidx", "rB_recv_size",
                                        "n_exec", "t_init", "t_pack", "t_a2a", "t_unpack", "t_spmm", "t_exec")}
        d["A_rowptr"] = arr(v.A_rowptr, v.A_nrow + 1, np.int32)
        d["A_colidx"] = arr(v.A_colidx, nnz, np.int32)
        d["A_val"] = arr(v.A_val, nnz, np.float64)
        d["rB_self_src_ridxs"] = arr(v.rB_self_src_ridxs, v.rB_self_nrow, np.int32)
        d["rB_scnts"] = arr(v.rB_scnts, P, np.int64)
        d["rB_sdispls"] = arr(v.rB_sdispls, P + 1, np.int64)
        d["rB_rcnts"] = arr(v.rB_rcnts, P, np.int64)
        d["rB_rdispls"] = arr(v.rB_rdispls, P + 1, np.int64)
        n = max(v.glb_n, 1)
        d["rB_sridxs"] = arr(v.rB_sridxs, int(d["rB_sdispls"][P]) // n if v.glb_n else 0, np.int32)
        d["rB_rridxs"] = arr(v.rB_rridxs, int(d["rB_rdispls"][P]) // n if v.glb_n else 0, np.int32)
        p = self._lib.crp_rp_spmm_dev_colidx_host(self.handle)
        d["dev_colidx"] = arr(p, nnz, np.int32)
        return d

    def free(self):
        if getattr(self, "handle", None) is not None and self.handle and self._owned:
            self._lib.crp_rp_spmm_free(C.byref(self.handle))
        self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Para2dSpmm:
    """2D (pm x pn) engine, arguments as para2d_spmm_init (src/para2d_spmm.h:22-47)."""

    def __init__(self, comm, pm, pn, A0_rowptr, B_rowptr, AC_rowptr, BC_colptr, A_rowptr, A_colidx, A_val,
                 plan_only=False):
        lib = L.load()
        self._lib, self.comm = lib, comm
        a0, br, ac, bc = _i32(A0_rowptr), _i32(B_rowptr), _i32(AC_rowptr), _i32(BC_colptr)
        rp, ci, va = _i32(A_rowptr), _i32(A_colidx), _f64(A_val)
        if ci.size == 0:
            ci, va = np.zeros(1, np.int32), np.zeros(1, np.float64)
        self.handle = C.c_void_p()
        fn = lib.crp_para2d_spmm_init_plan_only if plan_only else lib.crp_para2d_spmm_init
        fn(comm.ptr, pm, pn, _ip(a0), _ip(br), _ip(ac), _ip(bc), _ip(rp), _ip(ci), _dp(va),
                                 C.byref(self.handle))
        self.pm, self.pn = pm, pn
        self.pi, self.pj = comm.rank // pn, comm.rank % pn
        self.rp = RpSpmm._wrap(lib.crp_para2d_spmm_rp(self.handle), comm, lib)
        # rows of the B / Y block: the B_rowptr block of grid row pi (the row engine's loc_B_nrow)
        self.loc_B_nrow = int(br[self.pi + 1] - br[self.pi])

    def exec(self, BC_layout, B, C_out, stream=None):
        """float64 operands run the fp64 exec, float32 operands the fp32 exec (crp_para2d_spmm_exec_f32_ex)."""
        f32 = _operands_dtype(B, C_out) == "f32"
        bp, ldb, _kb = _ptr_ld(B, BC_layout, f32)
        cp, ldc, _kc = _ptr_ld(C_out, BC_layout, f32)
        if stream is None:
            stream = _current_stream(C_out)
        fn = self._lib.crp_para2d_spmm_exec_f32_ex if f32 else self._lib.crp_para2d_spmm_exec_ex
        fn(self.handle, BC_layout, bp, ldb, cp, ldc, stream)

    def update_values(self, A_val):
        """New values for the same pattern (crp_para2d_spmm_update_values): this rank's A0 slice values in the order given to
        init.  Collective over the grid row -- the first call of an engine with pn > 1 over the whole grid."""
        va = _f64(A_val).ravel()
        if va.size != self.slice_nnz:
            raise ValueError("A_val has %d entries, this rank's A0 slice %d nonzeros" % (va.size, self.slice_nnz))
        if va.size == 0:
            va = np.zeros(1, np.float64)
        self._lib.crp_para2d_spmm_update_values(self.handle, _dp(va))

    def _exec_t(self, f32, BC_layout, B, C_out, stream):
        bp, ldb, _kb = _ptr_ld(B, BC_layout, f32)
        cp, ldc, _kc = _ptr_ld(C_out, BC_layout, f32)
        _check_blocks(BC_layout, self.rp.glb_n, (("B", B, self.rp.A_nrow), ("C", C_out, self.loc_B_nrow)))
        if stream is None:
            stream = _current_stream(C_out)
        fn = self._lib.crp_para2d_spmm_exec_t_f32_ex if f32 else self._lib.crp_para2d_spmm_exec_t_ex
        fn(self.handle, BC_layout, bp, ldb, cp, ldc, stream)

    def exec_t(self, BC_layout, B, C_out, stream=None):
        """C := A^T * B (crp_para2d_spmm_exec_t_ex), fp64 only: B is this rank's (panel rows) x n_loc block, C_out its
        (B_rowptr block of grid row pi) x n_loc block; layouts and operands as ``exec``."""
        if _operands_dtype(B, C_out) != "f64":
            raise TypeError("exec_t is fp64 only: B and C must be float64")
        self._exec_t(False, BC_layout, B, C_out, stream)

    def exec_t_f32(self, BC_layout, B, C_out, stream=None):
        """C := A^T * B in fp32 (crp_para2d_spmm_exec_t_f32_ex): float32 operands only, blocks and layouts as ``exec_t``."""
        _f32_operands(B, C_out)
        self._exec_t(True, BC_layout, B, C_out, stream)

    def update_values_dev(self, vals, stream=None):
        """New values from device memory (crp_para2d_spmm_update_values_dev): a 1-D contiguous float64 or float32 CUDA tensor of
        ``slice_nnz`` entries, this rank's A0 slice values in the order given to init -- what ``sddmm`` writes.  Collective like
        ``update_values``; every rank of a grid row passes the same dtype."""
        ptr, f32, _keep = _dev_vals(vals, self.slice_nnz)
        if stream is None:
            stream = _current_stream(vals)
        self._lib.crp_para2d_spmm_update_values_dev(self.handle, ptr, f32, stream)

    def row_softmax(self, s, out=None, stream=None):
        """Row softmax over this rank's A0 slice (crp_para2d_spmm_row_softmax_ex): out[p] = exp(s[p] - max) / sum over every row's
        nonzeros.  ``s`` is a 1-D contiguous float64 or float32 CUDA tensor of ``slice_nnz`` entries in the order of the A_val given to
        init -- what ``sddmm`` writes and ``update_values_dev`` takes; ``out`` one like it (allocated when None; ``out is s`` is
        allowed).  Asynchronous on ``stream`` (default: the current torch stream), no communication, not collective; -inf entries
        are masked edges.  Every argument is checked before the library is called.  Returns ``out``."""
        s, out = _softmax_vecs((("s", s),), out, self.slice_nnz)
        if stream is None:
            stream = _current_stream(out)
        f32 = int(s.dtype.itemsize == 4)
        self._lib.crp_para2d_spmm_row_softmax_ex(self.handle, s.data_ptr() or None, out.data_ptr() or None, f32, stream)
        return out

    def row_softmax_bwd(self, y, dy, out=None, stream=None):
        """The Jacobian product of ``row_softmax`` (crp_para2d_spmm_row_softmax_bwd_ex): out[p] = y[p] * (dy[p] - D), D = the row's
        sum of y * dy.  Tensors as in ``row_softmax``, one dtype; ``out`` may be ``dy`` or ``y``.  Returns ``out``."""
        y, dy, out = _softmax_vecs((("y", y), ("dy", dy)), out, self.slice_nnz)
        if stream is None:
            stream = _current_stream(out)
        f32 = int(y.dtype.itemsize == 4)
        self._lib.crp_para2d_spmm_row_softmax_bwd_ex(self.handle, y.data_ptr() or None, dy.data_ptr() or None, out.data_ptr() or None, f32, stream)
        return out

    @property
    def row_softmax_built(self):
        """True once a ``row_softmax`` / ``row_softmax_bwd`` has uploaded the row pointer (crp_para2d_spmm_row_softmax_built); with
        pn > 1 an empty slice uploads nothing and stays False."""
        return bool(self._lib.crp_para2d_spmm_row_softmax_built(self.handle))

    def sddmm(self, BC_layout, X, Y, out, mode=0, stream=None):
        """SDDMM over all n columns (crp_para2d_spmm_sddmm_ex / _f32_ex, by the operands' dtype): out[p] = <X[i], Y[c]> for every
        nonzero p = (i, c) of this rank's A0 slice, in the order of the A_val given to init; mode 1: times the engine's current
        value of p.  X is this rank's (panel rows) x n_loc block, Y its (B_rowptr block) x n_loc block, ``out`` a 1-D array or
        tensor of ``slice_nnz`` entries of the same dtype, on the host or the device.  Collective over the grid row (the first
        call of an engine with pn > 1 over the whole grid).  Mixed dtypes, wrong shapes, a wrong ``out`` length and a wrong
        mode raise before the library is called."""
        f32 = _operands_dtype(X, Y) == "f32"
        if mode not in (0, 1):
            raise ValueError("mode must be 0 or 1, got %r" % (mode,))
        xp, ldx, _kx = _ptr_ld(X, BC_layout, f32)
        yp, ldy, _ky = _ptr_ld(Y, BC_layout, f32)
        _check_blocks(BC_layout, self.rp.glb_n, (("X", X, self.rp.A_nrow), ("Y", Y, self.loc_B_nrow)))
        op, _ko = _out_ptr(out, f32, self.slice_nnz)
        if stream is None:
            stream = _current_stream(out)
        if stream is None:
            stream = _current_stream(X)
        fn = self._lib.crp_para2d_spmm_sddmm_f32_ex if f32 else self._lib.crp_para2d_spmm_sddmm_ex
        fn(self.handle, BC_layout, xp, ldx, yp, ldy, op, int(mode), stream)

    @property
    def slice_nnz(self):
        """Nonzeros of this rank's A0 slice (crp_para2d_spmm_slice_nnz)."""
        return int(self._lib.crp_para2d_spmm_slice_nnz(self.handle))

    @property
    def row_slice_nnz(self):
        """Nonzeros of every A0 slice of this rank's grid row, pn entries (crp_para2d_spmm_row_slice_nnz)."""
        out = np.zeros(self.pn, np.int64)
        self._lib.crp_para2d_spmm_row_slice_nnz(self.handle, out.ctypes.data_as(L.c_ll_p))
        return out

    @property
    def sddmm_built(self):
        """True once a ``sddmm`` on a grid with pn > 1 has allocated the grid-row buffers (crp_para2d_spmm_sddmm_built)."""
        return bool(self._lib.crp_para2d_spmm_sddmm_built(self.handle))

    def print_stat(self):
        self._lib.crp_para2d_spmm_print_stat(self.handle)

    def clear_stat(self):
        self._lib.crp_para2d_spmm_clear_stat(self.handle)

    @property
    def rA_cost(self):
        return int(self._lib.crp_para2d_spmm_rA_cost(self.handle))

    @property
    def replicated_on_device(self):
        """True when init all-gathered the panel's column indices and values between device buffers."""
        return bool(self._lib.crp_para2d_spmm_replicated_on_device(self.handle))

    @property
    def value_uploads(self):
        """Times the panel's values crossed PCIe towards the device: 0 when the engine's matrices were filled from the device
        all-gather (crp_para2d_spmm_value_uploads)."""
        return int(self._lib.crp_para2d_spmm_value_uploads(self.handle))

    @property
    def t_ag_A(self):
        return float(self._lib.crp_para2d_spmm_t_ag_A(self.handle))

    def free(self):
        if getattr(self, "handle", None) is not None and self.handle:
            self._lib.crp_para2d_spmm_free(C.byref(self.handle))
        self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class MatRedist:
    """Generic dense 2D-block redistribution, arguments as mat_redist_engine_init
    (/root/reference/src/mat_redist.h:53-74) with the communicator in place of MPI_Comm / MPI_Datatype.
    dev_type: 0 host, 1 device staged through the host, 2 device to device."""

    def __init__(self, src_srow, src_scol, src_nrow, src_ncol, req_srow, req_scol, req_nrow, req_ncol, comm,
                 dt_size=8, dev_type=0):
        lib = L.load()
        self._lib, self.comm = lib, comm
        self.handle = C.c_void_p()
        lib.crp_mat_redist_init(src_srow, src_scol, src_nrow, src_ncol, req_srow, req_scol, req_nrow, req_ncol,
                                comm.ptr, dt_size, dev_type, C.byref(self.handle), None)
        if not self.handle:
            raise ValueError("mat_redist_engine_init rejected the arguments (invalid dev_type?)")
        self.dt_size, self.dev_type = dt_size, dev_type
        self.req_shape = (req_nrow, req_ncol)

    def exec(self, src_blk, dst_blk):
        """src_blk / dst_blk: 2-D row-major numpy arrays (dev_type 0) or cuda tensors (1, 2)."""
        sp, sld, _a = _ptr_ld_any(src_blk)
        dp, dld, _b = _ptr_ld_any(dst_blk)
        self._lib.crp_mat_redist_exec(self.handle, sp, sld, dp, dld)

    def view(self):
        v = L.MatRedistView()
        self._lib.crp_mat_redist_get_view(self.handle, C.byref(v))

        def arr(p, n):
            return np.ctypeslib.as_array(p, (n,)).copy() if n > 0 else np.zeros(0, np.int32)
        d = {k: getattr(v, k) for k in ("nproc", "rank", "n_proc_send", "n_proc_recv", "send_cnt", "recv_cnt", "hd_trans_ms")}
        d["send_ranks"], d["send_sizes"] = arr(v.send_ranks, v.n_proc_send), arr(v.send_sizes, v.n_proc_send)
        d["send_displs"], d["sblk_sizes"] = arr(v.send_displs, v.n_proc_send + 1), arr(v.sblk_sizes, 4 * v.n_proc_send)
        d["recv_ranks"], d["recv_sizes"] = arr(v.recv_ranks, v.n_proc_recv), arr(v.recv_sizes, v.n_proc_recv)
        d["recv_displs"], d["rblk_sizes"] = arr(v.recv_displs, v.n_proc_recv + 1), arr(v.rblk_sizes, 4 * v.n_proc_recv)
        return d

    def free(self):
        if getattr(self, "handle", None) is not None and self.handle:
            self._lib.crp_mat_redist_free(C.byref(self.handle))
        self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class CrpspmmEngine:
    """The older all-in-one engine, arguments as crpspmm_engine_init / _exec
    (/root/reference/deprecated/src/crpspmm.h:89-122) with the communicator in place of MPI_Comm:
    A in any 1D row distribution (src_A_rowptr holds GLOBAL nonzero offsets), B and C in arbitrary
    2D blocks, all host (numpy) arrays, A's values passed on every exec."""

    def __init__(self, m, n, k, src_A_srow, src_A_nrow, src_A_rowptr, src_A_colidx, src_B_srow, src_B_nrow, src_B_scol,
                 src_B_ncol, dst_C_srow, dst_C_nrow, dst_C_scol, dst_C_ncol, comm, plan_only=False):
        lib = L.load()
        self._lib, self.comm = lib, comm
        self.handle = C.c_void_p()
        self._rowptr, self._colidx = _i32(src_A_rowptr), _i32(src_A_colidx)
        if self._colidx.size == 0:
            self._colidx = np.zeros(1, np.int32)
        fn = lib.crp_crpspmm_init_plan_only if plan_only else lib.crp_crpspmm_init
        fn(m, n, k, src_A_srow, src_A_nrow, _ip(self._rowptr), _ip(self._colidx), src_B_srow, src_B_nrow, src_B_scol,
           src_B_ncol, dst_C_srow, dst_C_nrow, dst_C_scol, dst_C_ncol, comm.ptr, C.byref(self.handle))
        self.dst_shape = (dst_C_nrow, dst_C_ncol)

    def exec(self, src_A_val, src_B, dst_C):
        """src_B / dst_C: 2-D row-major float64 numpy arrays (the caller's blocks)."""
        val = _f64(src_A_val)
        if val.size == 0:
            val = np.zeros(1, np.float64)
        bp, ldb, _a = _ptr_ld_any(src_B)
        cp, ldc, _b = _ptr_ld_any(dst_C)
        self._lib.crp_crpspmm_exec(self.handle, _ip(self._rowptr), _ip(self._colidx), _dp(val), bp, ldb, cp, ldc)

    def view(self):
        v = L.CrpspmmView()
        self._lib.crp_crpspmm_get_view(self.handle, C.byref(v))
        d = {k: getattr(v, k) for k, _t in L.CrpspmmView._fields_ if not k.startswith(("loc_A_rowptr", "loc_A_colidx",
                                                                                     "loc_A_val", "red_B", "loc_C"))}

        def arr(p, n):
            return np.ctypeslib.as_array(p, (n,)).copy() if n > 0 else np.zeros(0)
        d["loc_A_rowptr"] = arr(v.loc_A_rowptr, v.loc_A_nrow + 1)
        d["loc_A_colidx"] = arr(v.loc_A_colidx, v.loc_A_nnz)
        d["loc_A_val"] = arr(v.loc_A_val, v.loc_A_nnz)
        d["red_B"] = arr(v.red_B, (v.rd_B_erow - v.rd_B_srow) * v.loc_B_ncol).reshape(v.rd_B_erow - v.rd_B_srow, v.loc_B_ncol)
        return d

    def print_stat(self):
        self._lib.crp_crpspmm_print_stat(self.handle)

    def clear_stat(self):
        self._lib.crp_crpspmm_clear_stat(self.handle)

    def free(self):
        if getattr(self, "handle", None) is not None and self.handle:
            self._lib.crp_crpspmm_free(C.byref(self.handle))
        self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _ptr_ld_any(x):
    """(address, leading dimension in elements, keepalive) of a 2-D row-major operand of any dtype."""
    try:
        import torch
        if isinstance(x, torch.Tensor):
            assert x.dim() == 2 and (x.shape[1] <= 1 or x.stride(1) == 1)
            return x.data_ptr(), x.stride(0) if x.shape[0] > 1 else max(x.shape[1], 1), x
    except ImportError:
        pass
    assert isinstance(x, np.ndarray) and x.ndim == 2 and (x.shape[1] <= 1 or x.strides[1] == x.itemsize)
    ld = x.strides[0] // x.itemsize if x.shape[0] > 1 else max(x.shape[1], 1)
    return x.ctypes.data, ld, x
