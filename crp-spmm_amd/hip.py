"""Device-level wrappers over include/crpspmm_hip.h for torch tensors
(data_ptr plumbing only; all arithmetic happens in the HIP kernels)."""
import ctypes as C

import numpy as np

from . import _lib as L


# negative return codes of crp_csr_transpose / crp_csr_dev_create_t (include/crpspmm_hip.h, CRP_CSR_T_E*)
T_EARG, T_ECOL, T_EPTR, T_EMIXED = -1, -3, -4, -5
_T_ERRORS = {T_EARG: "bad argument", T_ECOL: "column index out of range", T_EPTR: "rowptr does not start at 0 or decreases",
             T_EMIXED: "host and device pointers mixed"}


class TransposeError(ValueError):
    """A bad input to the CSR transpose (a CRP_CSR_T_E* code); ``code`` holds the code."""

    def __init__(self, what, code):
        super().__init__("%s: %s (code %d)" % (what, _T_ERRORS.get(code, "error"), code))
        self.code = code


class CsrDev:
    """Device-resident CSR (crp_csr_dev_create)."""

    def __init__(self, nrow, ncol, rowptr, colidx, val):
        lib = L.load()
        self._lib = lib
        rp = np.ascontiguousarray(rowptr, dtype=np.int32)
        ci = np.ascontiguousarray(colidx, dtype=np.int32)
        va = np.ascontiguousarray(val, dtype=np.float64)
        if ci.size == 0:
            ci, va = np.zeros(1, np.int32), np.zeros(1, np.float64)
        self.handle = C.c_void_p()
        L.check(lib.crp_csr_dev_create(nrow, ncol, rp.ctypes.data_as(L.c_int_p), ci.ctypes.data_as(L.c_int_p),
                                       va.ctypes.data_as(L.c_dbl_p), C.byref(self.handle)), "crp_csr_dev_create")
        self.nrow, self.ncol = nrow, ncol

    @classmethod
    def from_transpose(cls, nrow, ncol, rowptr, colidx, val):
        """A handle for A^T from the host CSR of the nrow x ncol matrix A (crp_csr_dev_create_t): transposed on the
        device.  ``self.nrow`` is ncol.  ``update_values`` takes values in A's order."""
        lib = L.load()
        rp = np.ascontiguousarray(rowptr, dtype=np.int32)
        ci = np.ascontiguousarray(colidx, dtype=np.int32)
        va = np.ascontiguousarray(val, dtype=np.float64)
        if ci.size == 0:
            ci, va = np.zeros(1, np.int32), np.zeros(1, np.float64)
        self = cls.__new__(cls)
        self._lib = lib
        self.handle = C.c_void_p()
        rc = lib.crp_csr_dev_create_t(nrow, ncol, rp.ctypes.data_as(L.c_int_p), ci.ctypes.data_as(L.c_int_p),
                                      va.ctypes.data_as(L.c_dbl_p), C.byref(self.handle))
        if rc < 0:
            raise TransposeError("crp_csr_dev_create_t", rc)
        L.check(rc, "crp_csr_dev_create_t")
        self.nrow, self.ncol = ncol, nrow
        return self

    @property
    def is_transposed(self):
        return bool(self._lib.crp_csr_dev_is_transposed(self.handle))

    def update_values(self, val, stream=None):
        """crp_csr_dev_update_values: new values in the order given at create (for a ``from_transpose`` handle: A's order);
        a numpy array (host pointer) or a float64 torch tensor on the device."""
        if isinstance(val, np.ndarray):
            keep = np.ascontiguousarray(val, dtype=np.float64)
            ptr, size = keep.ctypes.data, keep.size
        else:
            import torch
            if not (isinstance(val, torch.Tensor) and val.is_cuda and val.dtype == torch.float64 and val.is_contiguous()):
                raise TypeError("val must be a numpy array or a contiguous float64 torch tensor on the device")
            keep, ptr, size = val, val.data_ptr(), val.numel()
            if stream is None:
                stream = _stream(val)
        if size != self.nnz:
            raise ValueError("val has %d entries, the matrix %d nonzeros" % (size, self.nnz))
        L.check(self._lib.crp_csr_dev_update_values(self.handle, C.c_void_p(ptr or None), C.c_void_p(stream)),
                "crp_csr_dev_update_values")
        if isinstance(val, np.ndarray):
            L.check(self._lib.crp_stream_sync(C.c_void_p(stream)), "crp_stream_sync")      # `keep` may go away

    def set_rowmap(self, rowmap, c_nrow):
        """crp_csr_dev_set_rowmap: row t of this (row-subset) matrix writes row rowmap[t] of C and reads row rowmap[t] of
        the X of ``sddmm``, both of c_nrow rows; None restores the identity."""
        if rowmap is None:
            L.check(self._lib.crp_csr_dev_set_rowmap(self.handle, None, 0), "crp_csr_dev_set_rowmap")
            self._x_nrow = self.nrow
            return
        rm = np.ascontiguousarray(rowmap, dtype=np.int32)
        if rm.size != self.nrow:
            raise ValueError("rowmap has %d entries, the matrix %d rows" % (rm.size, self.nrow))
        L.check(self._lib.crp_csr_dev_set_rowmap(self.handle, rm.ctypes.data_as(L.c_int_p), int(c_nrow)), "crp_csr_dev_set_rowmap")
        self._x_nrow = int(c_nrow)

    def sddmm(self, X, Y0, Y1=None, out=None, out_pos=None, mode=0, stream=None):
        """Sampled dense-dense product over this matrix's pattern (crp_sddmm_csr_f64 / _f32, by the operands' dtype):
        out[p] = <X[i], Y[c]> for nonzero p = (i, c), times the matrix's value of p in mode 1; c >= 0 reads row c of Y0,
        c < 0 row ~c of Y1.  X, Y0, Y1 are 2-D row-major float64 or float32 cuda tensors of one dtype and width; ``out`` a
        1-D tensor of that dtype (allocated with nnz entries when None); ``out_pos`` an int32 cuda tensor of nnz entries:
        nonzero p writes out[out_pos[p]] (``out`` is then required and must hold every position named).  Returns ``out``.
        Mixed dtypes, wrong shapes and a short ``out`` raise before the library is called."""
        import torch
        ops = [("X", X), ("Y0", Y0)] + ([("Y1", Y1)] if Y1 is not None else [])
        for name, t in ops:
            if not (isinstance(t, torch.Tensor) and t.dim() == 2):
                raise TypeError("%s must be a 2-D torch tensor on the device" % name)
            if t.dtype not in (torch.float64, torch.float32):
                raise TypeError("%s must be float64 or float32, got %s" % (name, t.dtype))
            if t.dtype != X.dtype:
                raise TypeError("X, Y0 and Y1 must have one dtype (X is %s, %s is %s)" % (X.dtype, name, t.dtype))
            if t.shape[1] > 1 and t.stride(1) != 1:
                raise ValueError("%s must be contiguous along its rows" % name)
        if mode not in (0, 1):
            raise ValueError("mode must be 0 or 1, got %r" % (mode,))
        n = int(X.shape[1])
        if n < 1:
            raise ValueError("the operands need at least one column")
        for name, t in ops[1:]:
            if t.shape[1] != n:
                raise ValueError("%s has %d columns, X has %d" % (name, t.shape[1], n))
        x_nrow = getattr(self, "_x_nrow", self.nrow)
        if X.shape[0] < x_nrow:
            raise ValueError("X has %d rows, the matrix needs %d" % (X.shape[0], x_nrow))
        if Y0.shape[0] < self.ncol:
            raise ValueError("Y0 has %d rows, the matrix has %d columns" % (Y0.shape[0], self.ncol))
        nnz = self.nnz
        if out_pos is not None:
            if not (isinstance(out_pos, torch.Tensor) and out_pos.dtype == torch.int32 and out_pos.dim() == 1
                    and out_pos.is_contiguous()):
                raise TypeError("out_pos must be a contiguous 1-D int32 torch tensor on the device")
            if out_pos.numel() != nnz:
                raise ValueError("out_pos has %d entries, the matrix %d nonzeros" % (out_pos.numel(), nnz))
            if out is None:
                raise ValueError("out_pos needs an out to write into")
        if out is None:
            if not X.is_cuda:
                raise TypeError("X must be on the device")
            out = torch.empty(nnz, dtype=X.dtype, device=X.device)
        if not (isinstance(out, torch.Tensor) and out.dim() == 1 and out.is_contiguous()):
            raise TypeError("out must be a contiguous 1-D torch tensor on the device")
        if out.dtype != X.dtype:
            raise TypeError("out must have the operands' dtype (out is %s, X is %s)" % (out.dtype, X.dtype))
        if out_pos is None and out.numel() < nnz:
            raise ValueError("out has %d entries, the matrix %d nonzeros" % (out.numel(), nnz))
        for name, t in ops + [("out", out)] + ([("out_pos", out_pos)] if out_pos is not None else []):
            if not t.is_cuda or t.device != X.device:
                raise TypeError("%s must be on the device, with X" % name)      # (all pointers are device pointers)
        if nnz == 0:
            return out
        fn = self._lib.crp_sddmm_csr_f64 if X.dtype == torch.float64 else self._lib.crp_sddmm_csr_f32
        y1p, ld1 = (Y1.data_ptr(), Y1.stride(0)) if Y1 is not None else (None, 0)
        L.check(fn(self.handle, n, X.data_ptr(), X.stride(0), Y0.data_ptr(), Y0.stride(0), y1p, ld1, out.data_ptr() or None,
                   out_pos.data_ptr() if out_pos is not None else None, int(mode), _stream(out) if stream is None else stream),
                fn.__name__)
        return out

    def attention(self, Q, K0, V0, K1=None, V1=None, scale=1.0, bias=False, out=None, lse=None, p_out=None, out_pos=None,
                  stream=None, heads=1):
        """Fused sparse attention over this matrix's pattern (crp_attention_csr_f64 / _f32, by the operands' dtype):
        out[i] = sum_p softmax_p(scale * <Q[i], K[c_p]> (+ the matrix's value of p with ``bias``)) * V[c_p] over the nonzeros
        p = (i, c_p) of row i; c >= 0 reads row c of K0 / V0, c < 0 row ~c of K1 / V1.  Q, K0, K1 are 2-D row-major float64 or
        float32 cuda tensors of nk columns, V0, V1 of nv columns, all of one dtype; ``out`` a 2-D tensor of nv columns with a
        row per row of Q (allocated when None).  Optional outputs: ``lse`` a 1-D contiguous tensor with an entry per row of
        ``out``, ``p_out`` a 1-D contiguous tensor of nnz entries for the probabilities -- nonzero p writes p_out[out_pos[p]]
        when ``out_pos`` (int32, nnz entries) is given.  The matrix's values are not changed.  Returns ``out``.  Mixed
        dtypes, wrong shapes and tensors that are not on the device raise before the library is called.
        ``heads`` > 1 (crp_attention_mh_csr_*): the operands hold ``heads`` heads side by side, nk / heads and nv / heads
        columns each (both must divide); head h of ``out`` is bit for bit this call on the column views of head h.  ``lse`` is
        then a contiguous (rows, heads) tensor and ``p_out`` a contiguous (nnz, heads) one -- nonzero p writes row out_pos[p];
        the matrix's value of p (``bias``) is shared by the heads.  ``heads`` = 1 is the call above, unchanged."""
        import torch
        heads = _heads(heads)
        if (K1 is None) != (V1 is None):
            raise ValueError("K1 and V1 come together")
        kops = [("Q", Q), ("K0", K0)] + ([("K1", K1)] if K1 is not None else [])
        vops = [("V0", V0)] + ([("V1", V1)] if V1 is not None else []) + ([("out", out)] if out is not None else [])
        vecs = [(n_, t) for n_, t in (("lse", lse), ("p_out", p_out)) if t is not None]
        nk, nv, scale, bias = _attention_operands(kops, vops, vecs, scale, bias, heads, cap=False, by_operand=True)
        lse, p_out = _mh_flat("lse", lse, heads), _mh_flat("p_out", p_out, heads)
        x_nrow = getattr(self, "_x_nrow", self.nrow)
        if Q.size(0) < x_nrow:
            raise ValueError("Q has %d rows, the matrix needs %d" % (Q.size(0), x_nrow))
        for name, t in (("K0", K0), ("V0", V0)):
            if t.size(0) < self.ncol:
                raise ValueError("%s has %d rows, the matrix has %d columns" % (name, t.size(0), self.ncol))
        if K1 is not None and V1.size(0) != K1.size(0):
            raise ValueError("K1 has %d rows, V1 %d" % (K1.size(0), V1.size(0)))
        if out is not None and out.size(0) < x_nrow:
            raise ValueError("out has %d rows, the matrix needs %d" % (out.size(0), x_nrow))
        nnz = self.nnz
        if lse is not None and (lse.dim() != 1 or not lse.is_contiguous() or lse.numel() < x_nrow * heads):
            raise ValueError("lse must be 1-D and contiguous with %d entries" % x_nrow if heads == 1 else
                             "lse must hold %d rows of %d heads" % (x_nrow, heads))
        if out_pos is not None:
            if not (isinstance(out_pos, torch.Tensor) and out_pos.dtype == torch.int32 and out_pos.dim() == 1
                    and out_pos.is_contiguous()):
                raise TypeError("out_pos must be a contiguous 1-D int32 torch tensor on the device")
            if out_pos.numel() != nnz:
                raise ValueError("out_pos has %d entries, the matrix %d nonzeros" % (out_pos.numel(), nnz))
            if p_out is None:
                raise ValueError("out_pos needs a p_out to write into")
        if p_out is not None:
            if p_out.dim() != 1 or not p_out.is_contiguous():
                raise ValueError("p_out must be 1-D and contiguous")
            if out_pos is None and p_out.numel() < nnz * heads:
                raise ValueError("p_out has %d entries, the matrix %d nonzeros" % (p_out.numel() // heads, nnz))
        _attention_on_device(kops + vops + [(n_, t) for n_, t in (("lse", lse), ("p_out", p_out), ("out_pos", out_pos))
                                            if t is not None])
        if out is None:
            out = torch.empty((x_nrow, nv), dtype=Q.dtype, device=Q.device)
        if self.nrow == 0:
            return out
        fn, widths = L.attention_entry(self._lib, "attention", heads, Q.dtype == torch.float32, nk, nv)
        k1p, ldk1, v1p, ldv1 = (K1.data_ptr(), K1.stride(0), V1.data_ptr(), V1.stride(0)) if K1 is not None else (None, 0, None, 0)
        ptr = lambda t: (t.data_ptr() or None) if t is not None else None
        L.check(fn(self.handle, *widths, scale, bias, Q.data_ptr(), Q.stride(0), ptr(K0), K0.stride(0), k1p, ldk1,
                   ptr(V0), V0.stride(0), v1p, ldv1, out.data_ptr(), out.stride(0), ptr(lse), ptr(p_out), ptr(out_pos),
                   _stream(out) if stream is None else stream), fn.__name__)
        return out

    def attention_bwd_q(self, Q, K0, V0, O, dO, lse, K1=None, V1=None, scale=1.0, bias=False, dQ=None, delta=None, ds_out=None,
                        out_pos=None, stream=None, heads=1):
        """The row side of the fused backward of ``attention`` (crp_attention_bwd_q_csr_f64 / _f32, by the operands' dtype), on
        the handle the forward ran on: with ``O`` and ``lse`` as the forward wrote them and the upstream gradient ``dO``,
        dQ[i] = scale * sum_p dS_p K[c_p] and delta[i] = <dO[i], O[i]> for every row, dS_p = p_p (<dO[i], V[c_p]> - delta[i]),
        p_p = exp(s_p - lse[i]).  Q, K0, K1, dQ have nk columns, V0, V1, O, dO nv; ``lse`` and ``delta`` are 1-D contiguous with
        an entry per row of Q; ``ds_out`` (optional, 1-D contiguous, nnz entries) receives dS_p -- at ds_out[out_pos[p]] when
        ``out_pos`` is given -- the gradient of the bias, in the order ``update_values`` takes.  ``dQ`` and ``delta`` are
        allocated when None.  No output may alias an input.  Widths over 512 (float64) / 1024 (float32) raise ValueError: the
        chain of ``row_softmax_bwd`` and the products serves those.  Returns (dQ, delta).  Every error is raised before the
        library is called.
        ``heads`` > 1 (crp_attention_bwd_q_mh_csr_*): ``heads`` heads side by side as in ``attention``; ``lse`` and ``delta``
        are contiguous (rows, heads) tensors, ``ds_out`` a contiguous (nnz, heads) one whose sum over the heads is the
        gradient of the matrix's values, and the width cap applies to one head.  ``heads`` = 1 is the call above, unchanged."""
        import torch
        heads = _heads(heads)
        delta_given = delta
        lse, delta, ds_out = _mh_flat("lse", lse, heads), _mh_flat("delta", delta, heads), _mh_flat("ds_out", ds_out, heads)
        if (K1 is None) != (V1 is None):
            raise ValueError("K1 and V1 come together")
        kops = [("Q", Q), ("K0", K0)] + ([("K1", K1)] if K1 is not None else []) + ([("dQ", dQ)] if dQ is not None else [])
        vops = [("V0", V0)] + ([("V1", V1)] if V1 is not None else []) + [("O", O), ("dO", dO)]
        vecs = [("lse", lse)] + [(n_, t) for n_, t in (("delta", delta), ("ds_out", ds_out)) if t is not None]
        nk, nv, scale, bias = _attention_operands(kops, vops, vecs, scale, bias, heads)
        x_nrow = getattr(self, "_x_nrow", self.nrow)
        for name, t in (("Q", Q), ("O", O), ("dO", dO), ("dQ", dQ)):
            if t is not None and t.shape[0] < x_nrow:
                raise ValueError("%s has %d rows, the matrix needs %d" % (name, t.shape[0], x_nrow))
        for name, t in (("K0", K0), ("V0", V0)):
            if t.shape[0] < self.ncol:
                raise ValueError("%s has %d rows, the matrix has %d columns" % (name, t.shape[0], self.ncol))
        if K1 is not None and V1.shape[0] != K1.shape[0]:
            raise ValueError("K1 has %d rows, V1 %d" % (K1.shape[0], V1.shape[0]))
        for name, t in (("lse", lse), ("delta", delta)):
            if t is not None and t.numel() < x_nrow * heads:
                raise ValueError("%s must hold %d entries" % (name, x_nrow) if heads == 1 else
                                 "%s must hold %d rows of %d heads" % (name, x_nrow, heads))
        nnz = self.nnz
        if out_pos is not None:
            if not (isinstance(out_pos, torch.Tensor) and out_pos.dtype == torch.int32 and out_pos.dim() == 1
                    and out_pos.is_contiguous()):
                raise TypeError("out_pos must be a contiguous 1-D int32 torch tensor on the device")
            if out_pos.numel() != nnz:
                raise ValueError("out_pos has %d entries, the matrix %d nonzeros" % (out_pos.numel(), nnz))
            if ds_out is None:
                raise ValueError("out_pos needs a ds_out to write into")
        elif ds_out is not None and ds_out.numel() < nnz * heads:
            raise ValueError("ds_out has %d entries, the matrix %d nonzeros" % (ds_out.numel() // heads, nnz))
        _attention_on_device(kops + vops + vecs + ([("out_pos", out_pos)] if out_pos is not None else []))
        if dQ is None:
            dQ = torch.empty((x_nrow, nk), dtype=Q.dtype, device=Q.device)
        if delta is None:
            delta = delta_given = torch.empty((x_nrow,) if heads == 1 else (x_nrow, heads), dtype=Q.dtype, device=Q.device)
        if self.nrow == 0:
            return dQ, delta_given
        fn, widths = L.attention_entry(self._lib, "attention_bwd_q", heads, Q.dtype == torch.float32, nk, nv)
        k1p, ldk1, v1p, ldv1 = (K1.data_ptr(), K1.stride(0), V1.data_ptr(), V1.stride(0)) if K1 is not None else (None, 0, None, 0)
        ptr = lambda t: (t.data_ptr() or None) if t is not None else None
        L.check(fn(self.handle, *widths, scale, bias, Q.data_ptr(), Q.stride(0), ptr(K0), K0.stride(0), k1p, ldk1, ptr(V0), V0.stride(0),
                   v1p, ldv1, O.data_ptr(), O.stride(0), dO.data_ptr(), dO.stride(0), lse.data_ptr(), dQ.data_ptr(), dQ.stride(0),
                   delta.data_ptr(), ptr(ds_out), ptr(out_pos), _stream(dQ) if stream is None else stream), fn.__name__)
        return dQ, delta_given

    def attention_bwd_kv(self, K, V, Q, dO, lse, delta, scale=1.0, bias=False, dK=None, dV=None, stream=None, heads=1):
        """The column side of the fused backward of ``attention`` (crp_attention_bwd_kv_csr_f64 / _f32), on a handle of A^T
        (``from_transpose``): dK[c] = scale * sum_p dS_p Q[i_p] and dV[c] = sum_p p_p dO[i_p] over the entries of column c of A,
        with ``lse`` from the forward and ``delta`` from ``attention_bwd_q``.  K, Q, dK have nk columns, V, dO, dV nv; K, V, dK,
        dV a row per row of this handle, Q, dO, lse, delta one per column.  With ``bias`` the value added to a score is this
        handle's own.  ``dK is K`` and ``dV is V`` are allowed (same tensor); both are allocated when None.  Widths over 512
        (float64) / 1024 (float32) raise ValueError.  Returns (dK, dV).  Every error is raised before the library is called.
        ``heads`` > 1 (crp_attention_bwd_kv_mh_csr_*): ``heads`` heads side by side; ``lse`` and ``delta`` are the contiguous
        (rows of A, heads) tensors of the row side, and the width cap applies to one head."""
        import torch
        heads = _heads(heads)
        lse, delta = _mh_flat("lse", lse, heads), _mh_flat("delta", delta, heads)
        kops = [("K", K), ("Q", Q)] + ([("dK", dK)] if dK is not None else [])
        vops = [("V", V), ("dO", dO)] + ([("dV", dV)] if dV is not None else [])
        nk, nv, scale, bias = _attention_operands(kops, vops, [("lse", lse), ("delta", delta)], scale, bias, heads)
        x_nrow = getattr(self, "_x_nrow", self.nrow)
        for name, t in (("K", K), ("V", V), ("dK", dK), ("dV", dV)):
            if t is not None and t.shape[0] < x_nrow:
                raise ValueError("%s has %d rows, the matrix needs %d" % (name, t.shape[0], x_nrow))
        for name, t in (("Q", Q), ("dO", dO)):
            if t.shape[0] < self.ncol:
                raise ValueError("%s has %d rows, the matrix has %d columns" % (name, t.shape[0], self.ncol))
        for name, t in (("lse", lse), ("delta", delta)):
            if t.numel() < self.ncol * heads:
                raise ValueError("%s must hold %d entries" % (name, self.ncol) if heads == 1 else
                                 "%s must hold %d rows of %d heads" % (name, self.ncol, heads))
        _attention_on_device(kops + vops + [("lse", lse), ("delta", delta)])
        if dK is None:
            dK = torch.empty((x_nrow, nk), dtype=K.dtype, device=K.device)
        if dV is None:
            dV = torch.empty((x_nrow, nv), dtype=K.dtype, device=K.device)
        if self.nrow == 0:
            return dK, dV
        fn, widths = L.attention_entry(self._lib, "attention_bwd_kv", heads, K.dtype == torch.float32, nk, nv)
        L.check(fn(self.handle, *widths, scale, bias, K.data_ptr(), K.stride(0), V.data_ptr(), V.stride(0), Q.data_ptr() or None,
                   Q.stride(0), dO.data_ptr() or None, dO.stride(0), lse.data_ptr() or None, delta.data_ptr() or None, dK.data_ptr(),
                   dK.stride(0), dV.data_ptr(), dV.stride(0), _stream(dK) if stream is None else stream), fn.__name__)
        return dK, dV

    def gat_attention(self, el, er0, V0, er1=None, V1=None, slope=0.2, bias=False, out=None, lse=None, p_out=None, out_pos=None,
                      stream=None, heads=1, dropout=0.0, seed=0):
        """Fused GAT attention over this matrix's pattern (crp_gat_attention_csr_f64 / _f32, by the operands' dtype): for every
        head h, out[i]_h = sum_p softmax_p(leaky_relu(el[i, h] + er[c_p, h], slope) (+ the matrix's value of p with ``bias``))
        * V[c_p]_h over the nonzeros p = (i, c_p) of row i; c >= 0 reads row c of er0 / V0, c < 0 row ~c of er1 / V1.  ``el`` is
        a 2-D (rows, heads) tensor, ``er0`` / ``er1`` (rows of V0 / V1, heads), ``V0`` / ``V1`` have heads * dv columns, all
        row-major float64 or float32 cuda tensors of one dtype; ``out`` has V's width and a row per row of ``el`` (allocated
        when None).  Optional outputs: ``lse`` contiguous (rows, heads), ``p_out`` contiguous (nnz, heads) -- nonzero p writes
        row out_pos[p] when ``out_pos`` (int32, nnz entries) is given; with one head both may be 1-D.  The matrix's values are
        not changed.  ``dropout`` > 0 drops the attention coefficients after the softmax at that rate, by the mask of
        ``dropout_mask(heads, dropout, seed)``, and scales the kept ones by 1 / (1 - dropout) (crp_gat_attention_drop_csr_*);
        ``lse`` and ``p_out`` are those of the call without it.  Returns ``out``.  Every error is raised before the library is
        called."""
        import torch
        heads = _heads(heads)
        dropout, seed = _dropout(dropout, seed)
        if (er1 is None) != (V1 is None):
            raise ValueError("er1 and V1 come together")
        sops = [("el", el), ("er0", er0)] + ([("er1", er1)] if er1 is not None else [])
        vops = [("V0", V0)] + ([("V1", V1)] if V1 is not None else []) + ([("out", out)] if out is not None else [])
        vecs = [(n_, t) for n_, t in (("lse", lse), ("p_out", p_out)) if t is not None]
        nv, slope, bias = _gat_operands(sops, vops, vecs, slope, bias, heads, cap=False)
        lse, p_out = _gat_flat("lse", lse, heads), _gat_flat("p_out", p_out, heads)
        x_nrow = getattr(self, "_x_nrow", self.nrow)
        for name, t in (("el", el), ("out", out)):
            if t is not None and t.size(0) < x_nrow:
                raise ValueError("%s has %d rows, the matrix needs %d" % (name, t.size(0), x_nrow))
        for name, t in (("er0", er0), ("V0", V0)):
            if t.size(0) < self.ncol:
                raise ValueError("%s has %d rows, the matrix has %d columns" % (name, t.size(0), self.ncol))
        if er1 is not None and V1.size(0) != er1.size(0):
            raise ValueError("er1 has %d rows, V1 %d" % (er1.size(0), V1.size(0)))
        nnz = self.nnz
        if lse is not None and lse.numel() < x_nrow * heads:
            raise ValueError("lse must hold %d rows of %d heads" % (x_nrow, heads))
        _gat_out_pos(out_pos, p_out, "p_out", nnz, heads)
        _attention_on_device(sops + vops + [(n_, t) for n_, t in (("lse", lse), ("p_out", p_out), ("out_pos", out_pos))
                                            if t is not None])
        if out is None:
            out = torch.empty((x_nrow, nv), dtype=el.dtype, device=el.device)
        if self.nrow == 0:
            return out
        fn, drop = _drop_entry(self._lib, "gat_attention", "", el.dtype == torch.float32, dropout, seed)
        e1p, lde1, v1p, ldv1 = (er1.data_ptr(), er1.stride(0), V1.data_ptr(), V1.stride(0)) if er1 is not None else (None, 0, None, 0)
        ptr = lambda t: (t.data_ptr() or None) if t is not None else None
        L.check(fn(self.handle, heads, nv // heads, slope, bias, el.data_ptr(), el.stride(0), ptr(er0), er0.stride(0), e1p, lde1,
                   ptr(V0), V0.stride(0), v1p, ldv1, out.data_ptr(), out.stride(0), ptr(lse), ptr(p_out), ptr(out_pos), *drop,
                   _stream(out) if stream is None else stream), fn.__name__)
        return out

    def gat_attention_bwd_row(self, el, er0, V0, O, dO, lse, er1=None, V1=None, slope=0.2, bias=False, d_el=None, delta=None,
                              ds_out=None, out_pos=None, stream=None, heads=1, dropout=0.0, seed=0):
        """The row side of the fused backward of ``gat_attention`` (crp_gat_attention_bwd_row_csr_f64 / _f32), on the handle the
        forward ran on: with ``O`` and ``lse`` as the forward wrote them and the upstream gradient ``dO``, delta[i, h] =
        <dO[i]_h, O[i]_h> and d_el[i, h] = the sum over the row of dZ_p = dS_p * (z_p > 0 ? 1 : slope), dS_p = p_p (<dO[i]_h,
        V[c_p]_h> - delta[i, h]), p_p = exp(s_p - lse[i, h]).  ``d_el`` (rows, heads) and ``delta`` contiguous (rows, heads) are
        allocated when None; ``ds_out`` (optional, contiguous (nnz, heads)) receives dS_p -- at row out_pos[p] when ``out_pos``
        is given -- whose sum over the heads is the gradient of the matrix's values.  No output may alias an input.  A head
        wider than 512 (float64) / 1024 (float32) columns raises ValueError.  ``dropout`` and ``seed``: the forward's (``O`` is the
        dropped output; dP counts as 0 on a dropped edge and as dP / (1 - dropout) on a kept one).  Returns (d_el, delta)."""
        import torch
        heads = _heads(heads)
        dropout, seed = _dropout(dropout, seed)
        if (er1 is None) != (V1 is None):
            raise ValueError("er1 and V1 come together")
        sops = [("el", el), ("er0", er0)] + ([("er1", er1)] if er1 is not None else []) + ([("d_el", d_el)] if d_el is not None else [])
        vops = [("V0", V0)] + ([("V1", V1)] if V1 is not None else []) + [("O", O), ("dO", dO)]
        vecs = [("lse", lse)] + [(n_, t) for n_, t in (("delta", delta), ("ds_out", ds_out)) if t is not None]
        nv, slope, bias = _gat_operands(sops, vops, vecs, slope, bias, heads)
        delta_given = delta
        lse, delta, ds_out = _gat_flat("lse", lse, heads), _gat_flat("delta", delta, heads), _gat_flat("ds_out", ds_out, heads)
        x_nrow = getattr(self, "_x_nrow", self.nrow)
        for name, t in (("el", el), ("O", O), ("dO", dO), ("d_el", d_el)):
            if t is not None and t.size(0) < x_nrow:
                raise ValueError("%s has %d rows, the matrix needs %d" % (name, t.size(0), x_nrow))
        for name, t in (("er0", er0), ("V0", V0)):
            if t.size(0) < self.ncol:
                raise ValueError("%s has %d rows, the matrix has %d columns" % (name, t.size(0), self.ncol))
        if er1 is not None and V1.size(0) != er1.size(0):
            raise ValueError("er1 has %d rows, V1 %d" % (er1.size(0), V1.size(0)))
        for name, t in (("lse", lse), ("delta", delta)):
            if t is not None and t.numel() < x_nrow * heads:
                raise ValueError("%s must hold %d rows of %d heads" % (name, x_nrow, heads))
        _gat_out_pos(out_pos, ds_out, "ds_out", self.nnz, heads)
        _attention_on_device(sops + vops + vecs + ([("out_pos", out_pos)] if out_pos is not None else []))
        if d_el is None:
            d_el = torch.empty((x_nrow, heads), dtype=el.dtype, device=el.device)
        if delta is None:
            delta_given = torch.empty((x_nrow, heads), dtype=el.dtype, device=el.device)
            delta = delta_given.view(-1)
        if self.nrow == 0:
            return d_el, delta_given
        fn, drop = _drop_entry(self._lib, "gat_attention", "_bwd_row", el.dtype == torch.float32, dropout, seed)
        e1p, lde1, v1p, ldv1 = (er1.data_ptr(), er1.stride(0), V1.data_ptr(), V1.stride(0)) if er1 is not None else (None, 0, None, 0)
        ptr = lambda t: (t.data_ptr() or None) if t is not None else None
        L.check(fn(self.handle, heads, nv // heads, slope, bias, el.data_ptr(), el.stride(0), ptr(er0), er0.stride(0), e1p, lde1,
                   ptr(V0), V0.stride(0), v1p, ldv1, O.data_ptr(), O.stride(0), dO.data_ptr(), dO.stride(0), lse.data_ptr(),
                   d_el.data_ptr(), d_el.stride(0), delta.data_ptr(), ptr(ds_out), ptr(out_pos), *drop,
                   _stream(d_el) if stream is None else stream), fn.__name__)
        return d_el, delta_given

    def gat_attention_bwd_col(self, er, V, el, dO, lse, delta, slope=0.2, bias=False, d_er=None, dV=None, stream=None, heads=1,
                              dropout=0.0, seed=0):
        """The column side of the fused backward of ``gat_attention`` (crp_gat_attention_bwd_col_csr_f64 / _f32), on a handle of
        A^T (``from_transpose``): d_er[c, h] = the sum over column c of A of dZ_p and dV[c]_h = sum_p p_p dO[i_p]_h, with ``lse``
        from the forward and ``delta`` from ``gat_attention_bwd_row``.  ``er``, ``d_er`` (rows of this handle, heads) and ``V``,
        ``dV`` have a row per row of this handle; ``el``, ``dO``, ``lse``, ``delta`` one per column.  With ``bias`` the value added
        to a score is this handle's own.  ``dV is V`` is allowed (same tensor); both outputs are allocated when None.  A head wider
        than 512 (float64) / 1024 (float32) columns raises ValueError.  ``dropout`` and ``seed``: the forward's; this handle draws
        the bits the forward's handle drew.  Returns (d_er, dV)."""
        import torch
        heads = _heads(heads)
        dropout, seed = _dropout(dropout, seed)
        sops = [("er", er), ("el", el)] + ([("d_er", d_er)] if d_er is not None else [])
        vops = [("V", V), ("dO", dO)] + ([("dV", dV)] if dV is not None else [])
        nv, slope, bias = _gat_operands(sops, vops, [("lse", lse), ("delta", delta)], slope, bias, heads)
        lse, delta = _gat_flat("lse", lse, heads), _gat_flat("delta", delta, heads)
        x_nrow = getattr(self, "_x_nrow", self.nrow)
        for name, t in (("er", er), ("V", V), ("d_er", d_er), ("dV", dV)):
            if t is not None and t.size(0) < x_nrow:
                raise ValueError("%s has %d rows, the matrix needs %d" % (name, t.size(0), x_nrow))
        for name, t in (("el", el), ("dO", dO)):
            if t.size(0) < self.ncol:
                raise ValueError("%s has %d rows, the matrix has %d columns" % (name, t.size(0), self.ncol))
        for name, t in (("lse", lse), ("delta", delta)):
            if t.numel() < self.ncol * heads:
                raise ValueError("%s must hold %d rows of %d heads" % (name, self.ncol, heads))
        _attention_on_device(sops + vops + [("lse", lse), ("delta", delta)])
        if d_er is None:
            d_er = torch.empty((x_nrow, heads), dtype=er.dtype, device=er.device)
        if dV is None:
            dV = torch.empty((x_nrow, nv), dtype=er.dtype, device=er.device)
        if self.nrow == 0:
            return d_er, dV
        fn, drop = _drop_entry(self._lib, "gat_attention", "_bwd_col", er.dtype == torch.float32, dropout, seed)
        L.check(fn(self.handle, heads, nv // heads, slope, bias, er.data_ptr(), er.stride(0), V.data_ptr(), V.stride(0),
                   el.data_ptr() or None, el.stride(0), dO.data_ptr() or None, dO.stride(0), lse.data_ptr() or None,
                   delta.data_ptr() or None, d_er.data_ptr(), d_er.stride(0), dV.data_ptr(), dV.stride(0), *drop,
                   _stream(dV) if stream is None else stream), fn.__name__)
        return d_er, dV

    def gatv2_attention(self, XT, XS0, a, XS1=None, slope=0.2, bias=False, out=None, lse=None, p_out=None, out_pos=None, stream=None,
                        heads=1, dropout=0.0, seed=0):
        """Fused GATv2 attention over this matrix's pattern (crp_gatv2_attention_csr_f64 / _f32, by the operands' dtype): for every
        head h, s_p = sum_j a[h, j] * leaky_relu(XT[i]_h[j] + XS[c_p]_h[j], slope) (+ the matrix's value of p with ``bias``) and
        out[i]_h = sum_p softmax_p(s) * XS[c_p]_h over the nonzeros p = (i, c_p) of row i; c >= 0 reads row c of XS0, c < 0 row ~c
        of XS1.  ``XT`` (rows, heads * dv) and ``XS0`` / ``XS1`` are 2-D row-major float64 or float32 cuda tensors of one dtype and
        width; ``a`` holds heads * dv contiguous elements (1-D, or (heads, dv)); ``out`` has that width and a row per row of
        ``XT`` (allocated when None).  Optional outputs: ``lse`` contiguous (rows, heads), ``p_out`` contiguous (nnz, heads) --
        nonzero p writes row out_pos[p] when ``out_pos`` (int32, nnz entries) is given; with one head both may be 1-D.  A head
        wider than 512 (float64) / 1024 (float32) columns raises ValueError.  The matrix's values are not changed.  ``dropout`` > 0
        drops the attention coefficients after the softmax at that rate, by the mask of ``dropout_mask(heads, dropout, seed)``,
        and scales the kept ones by 1 / (1 - dropout) (crp_gatv2_attention_drop_csr_*); ``lse`` and ``p_out`` are those of the
        call without it.  Returns ``out``.  Every error is raised before the library is called."""
        import torch
        heads = _heads(heads)
        dropout, seed = _dropout(dropout, seed)
        vops = [("XT", XT), ("XS0", XS0)] + ([("XS1", XS1)] if XS1 is not None else []) + ([("out", out)] if out is not None else [])
        vecs = [(n_, t) for n_, t in (("lse", lse), ("p_out", p_out)) if t is not None]
        nv, slope, bias = _gatv2_operands(vops, vecs, a, slope, bias, heads)
        lse, p_out = _gat_flat("lse", lse, heads), _gat_flat("p_out", p_out, heads)
        x_nrow = getattr(self, "_x_nrow", self.nrow)
        for name, t in (("XT", XT), ("out", out)):
            if t is not None and t.size(0) < x_nrow:
                raise ValueError("%s has %d rows, the matrix needs %d" % (name, t.size(0), x_nrow))
        if XS0.size(0) < self.ncol:
            raise ValueError("XS0 has %d rows, the matrix has %d columns" % (XS0.size(0), self.ncol))
        if lse is not None and lse.numel() < x_nrow * heads:
            raise ValueError("lse must hold %d rows of %d heads" % (x_nrow, heads))
        _gat_out_pos(out_pos, p_out, "p_out", self.nnz, heads)
        _attention_on_device(vops + [("a", a)] + [(n_, t) for n_, t in (("lse", lse), ("p_out", p_out), ("out_pos", out_pos))
                                                  if t is not None])
        if out is None:
            out = torch.empty((x_nrow, nv), dtype=XT.dtype, device=XT.device)
        if self.nrow == 0:
            return out
        fn, drop = _drop_entry(self._lib, "gatv2_attention", "", XT.dtype == torch.float32, dropout, seed)
        x1p, ldx1 = (XS1.data_ptr(), XS1.stride(0)) if XS1 is not None else (None, 0)
        ptr = lambda t: (t.data_ptr() or None) if t is not None else None
        L.check(fn(self.handle, heads, nv // heads, slope, bias, XT.data_ptr(), XT.stride(0), ptr(XS0), XS0.stride(0), x1p, ldx1,
                   a.data_ptr(), out.data_ptr(), out.stride(0), ptr(lse), ptr(p_out), ptr(out_pos), *drop,
                   _stream(out) if stream is None else stream), fn.__name__)
        return out

    def gatv2_attention_bwd_row(self, XT, XS0, a, O, dO, lse, XS1=None, slope=0.2, bias=False, dXT=None, da_part=None, delta=None,
                                ds_out=None, out_pos=None, stream=None, heads=1, dropout=0.0, seed=0):
        """The row side of the fused backward of ``gatv2_attention`` (crp_gatv2_attention_bwd_row_csr_f64 / _f32), on the handle the
        forward ran on: with ``O`` and ``lse`` as the forward wrote them and the upstream gradient ``dO``, delta[i, h] =
        <dO[i]_h, O[i]_h>, dXT[i]_h[j] = sum_p dS_p * (z_pj > 0 ? a[h, j] : a[h, j] * slope) and da_part[i]_h[j] = sum_p dS_p *
        leaky_relu(z_pj) -- the row's share of the gradient of ``a``, which ``col_sum`` adds over the rows -- with dS_p = p_p
        (<dO[i]_h, XS[c_p]_h> - delta[i, h]) and p_p = exp(s_p - lse[i, h]).  ``dXT``, ``da_part`` (rows, heads * dv) and ``delta``
        contiguous (rows, heads) are allocated when None; ``ds_out`` (optional, contiguous (nnz, heads)) receives dS_p -- at row
        out_pos[p] when ``out_pos`` is given.  No output may alias an input.  ``dropout`` and ``seed``: the forward's (``O`` is the
        dropped output; dP counts as 0 on a dropped edge and as dP / (1 - dropout) on a kept one).  Returns (dXT, da_part, delta)."""
        import torch
        heads = _heads(heads)
        dropout, seed = _dropout(dropout, seed)
        vops = ([("XT", XT), ("XS0", XS0)] + ([("XS1", XS1)] if XS1 is not None else []) + [("O", O), ("dO", dO)]
                + [(n_, t) for n_, t in (("dXT", dXT), ("da_part", da_part)) if t is not None])
        vecs = [("lse", lse)] + [(n_, t) for n_, t in (("delta", delta), ("ds_out", ds_out)) if t is not None]
        nv, slope, bias = _gatv2_operands(vops, vecs, a, slope, bias, heads)
        delta_given = delta
        lse, delta, ds_out = _gat_flat("lse", lse, heads), _gat_flat("delta", delta, heads), _gat_flat("ds_out", ds_out, heads)
        x_nrow = getattr(self, "_x_nrow", self.nrow)
        for name, t in (("XT", XT), ("O", O), ("dO", dO), ("dXT", dXT), ("da_part", da_part)):
            if t is not None and t.size(0) < x_nrow:
                raise ValueError("%s has %d rows, the matrix needs %d" % (name, t.size(0), x_nrow))
        if XS0.size(0) < self.ncol:
            raise ValueError("XS0 has %d rows, the matrix has %d columns" % (XS0.size(0), self.ncol))
        for name, t in (("lse", lse), ("delta", delta)):
            if t is not None and t.numel() < x_nrow * heads:
                raise ValueError("%s must hold %d rows of %d heads" % (name, x_nrow, heads))
        _gat_out_pos(out_pos, ds_out, "ds_out", self.nnz, heads)
        _attention_on_device(vops + [("a", a)] + vecs + ([("out_pos", out_pos)] if out_pos is not None else []))
        if dXT is None:
            dXT = torch.empty((x_nrow, nv), dtype=XT.dtype, device=XT.device)
        if da_part is None:
            da_part = torch.empty((x_nrow, nv), dtype=XT.dtype, device=XT.device)
        if delta is None:
            delta_given = torch.empty((x_nrow, heads), dtype=XT.dtype, device=XT.device)
            delta = delta_given.view(-1)
        if self.nrow == 0:
            return dXT, da_part, delta_given
        fn, drop = _drop_entry(self._lib, "gatv2_attention", "_bwd_row", XT.dtype == torch.float32, dropout, seed)
        x1p, ldx1 = (XS1.data_ptr(), XS1.stride(0)) if XS1 is not None else (None, 0)
        ptr = lambda t: (t.data_ptr() or None) if t is not None else None
        L.check(fn(self.handle, heads, nv // heads, slope, bias, XT.data_ptr(), XT.stride(0), ptr(XS0), XS0.stride(0), x1p, ldx1,
                   a.data_ptr(), O.data_ptr(), O.stride(0), dO.data_ptr(), dO.stride(0), lse.data_ptr(), dXT.data_ptr(), dXT.stride(0),
                   da_part.data_ptr(), da_part.stride(0), delta.data_ptr(), ptr(ds_out), ptr(out_pos), *drop,
                   _stream(dXT) if stream is None else stream), fn.__name__)
        return dXT, da_part, delta_given

    def gatv2_attention_bwd_col(self, XS, XT, a, dO, lse, delta, slope=0.2, bias=False, dXS=None, stream=None, heads=1, dropout=0.0,
                                seed=0):
        """The column side of the fused backward of ``gatv2_attention`` (crp_gatv2_attention_bwd_col_csr_f64 / _f32), on a handle of
        A^T (``from_transpose``): dXS[c]_h = sum_p dS_p * (z_p > 0 ? a_h : a_h * slope) + sum_p p_p dO[i_p]_h over column c of A --
        two sums in this handle's order and one addition -- with ``lse`` from the forward and ``delta`` from
        ``gatv2_attention_bwd_row``.  ``XS`` and ``dXS`` have a row per row of this handle; ``XT``, ``dO``, ``lse``, ``delta`` one per
        column.  With ``bias`` the value added to a score is this handle's own.  ``dXS is XS`` is allowed (same tensor); it is
        allocated when None.  ``dropout`` and ``seed``: the forward's; this handle draws the bits the forward's handle drew.
        Returns dXS."""
        import torch
        heads = _heads(heads)
        dropout, seed = _dropout(dropout, seed)
        vops = [("XS", XS), ("XT", XT), ("dO", dO)] + ([("dXS", dXS)] if dXS is not None else [])
        nv, slope, bias = _gatv2_operands(vops, [("lse", lse), ("delta", delta)], a, slope, bias, heads)
        lse, delta = _gat_flat("lse", lse, heads), _gat_flat("delta", delta, heads)
        x_nrow = getattr(self, "_x_nrow", self.nrow)
        for name, t in (("XS", XS), ("dXS", dXS)):
            if t is not None and t.size(0) < x_nrow:
                raise ValueError("%s has %d rows, the matrix needs %d" % (name, t.size(0), x_nrow))
        for name, t in (("XT", XT), ("dO", dO)):
            if t.size(0) < self.ncol:
                raise ValueError("%s has %d rows, the matrix has %d columns" % (name, t.size(0), self.ncol))
        for name, t in (("lse", lse), ("delta", delta)):
            if t.numel() < self.ncol * heads:
                raise ValueError("%s must hold %d rows of %d heads" % (name, self.ncol, heads))
        _attention_on_device(vops + [("a", a), ("lse", lse), ("delta", delta)])
        if dXS is None:
            dXS = torch.empty((x_nrow, nv), dtype=XS.dtype, device=XS.device)
        if self.nrow == 0:
            return dXS
        fn, drop = _drop_entry(self._lib, "gatv2_attention", "_bwd_col", XS.dtype == torch.float32, dropout, seed)
        L.check(fn(self.handle, heads, nv // heads, slope, bias, XS.data_ptr(), XS.stride(0), XT.data_ptr() or None, XT.stride(0),
                   a.data_ptr(), dO.data_ptr() or None, dO.stride(0), lse.data_ptr() or None, delta.data_ptr() or None,
                   dXS.data_ptr(), dXS.stride(0), *drop, _stream(dXS) if stream is None else stream), fn.__name__)
        return dXS

    def dropout_mask(self, heads, dropout, seed, out=None, out_pos=None, stream=None):
        """The attention-dropout mask of the fused GAT / GATv2 calls over this handle (crp_dropout_mask_csr): a uint8 cuda tensor
        (nnz, heads) of keep flags, entry (p, h) -- row out_pos[p] when ``out_pos`` (int32, nnz entries) is given, ``out`` is then
        required -- 1 iff ``dropout_keep(seed, r, c, h, dropout)`` with (r, c) = (the row after the row map, the column code) on a
        handle of A and (the entry's column index, this handle's row after its row map) on a ``from_transpose`` handle, so that
        both handles of a pair flag the same edges.  Duplicate (r, c) entries share a flag.  Returns ``out``."""
        import torch
        heads = _heads(heads)
        dropout, seed = _dropout(dropout, seed)
        nnz = self.nnz
        if out is not None:
            if not (isinstance(out, torch.Tensor) and out.dtype == torch.uint8 and out.is_contiguous()):
                raise TypeError("out must be a contiguous uint8 torch tensor on the device")
            if not out.is_cuda:
                raise TypeError("out must be on the device")
        if out_pos is not None:
            if not (isinstance(out_pos, torch.Tensor) and out_pos.dtype == torch.int32 and out_pos.dim() == 1 and out_pos.is_contiguous()):
                raise TypeError("out_pos must be a contiguous 1-D int32 torch tensor on the device")
            if out_pos.numel() != nnz:
                raise ValueError("out_pos has %d entries, the matrix %d nonzeros" % (out_pos.numel(), nnz))
            if out is None:
                raise ValueError("out_pos needs an out to write into")
            if not out_pos.is_cuda or out_pos.device != out.device:
                raise TypeError("out_pos must be on the device, with out")
        elif out is not None and out.numel() < nnz * heads:
            raise ValueError("out has %d rows, the matrix %d nonzeros" % (out.numel() // heads, nnz))
        if out is None:
            out = torch.empty((nnz, heads), dtype=torch.uint8, device=torch.device("cuda", torch.cuda.current_device()))
        if nnz == 0:
            return out
        L.check(self._lib.crp_dropout_mask_csr(self.handle, heads, dropout, seed, out.data_ptr(),
                                               out_pos.data_ptr() if out_pos is not None else None,
                                               _stream(out) if stream is None else stream), "crp_dropout_mask_csr")
        return out

    def row_softmax(self, s, out=None, stream=None):
        """Row softmax over this matrix's pattern (crp_csr_dev_row_softmax_f64 / _f32, by the dtype of ``s``): for every row,
        out[p] = exp(s[p] - max) / sum over the row's nonzeros p, which count in the handle's CSR order -- what ``sddmm``
        writes.  ``s`` is a 1-D contiguous float64 or float32 cuda tensor of nnz entries; ``out`` one like it (allocated when
        None; ``out is s`` is allowed).  -inf entries are masked edges (exactly 0).  Returns ``out``."""
        s, out = _softmax_vecs((("s", s),), out, self.nnz)
        if self.nnz == 0:
            return out
        import torch
        fn = self._lib.crp_csr_dev_row_softmax_f64 if s.dtype == torch.float64 else self._lib.crp_csr_dev_row_softmax_f32
        L.check(fn(self.handle, s.data_ptr(), out.data_ptr(), _stream(out) if stream is None else stream), fn.__name__)
        return out

    def row_softmax_bwd(self, y, dy, out=None, stream=None):
        """The Jacobian product of ``row_softmax`` (crp_csr_dev_row_softmax_bwd_f64 / _f32): out[p] = y[p] * (dy[p] - D) with
        D = the row's sum of y * dy.  ``y``, ``dy`` and ``out`` as in ``row_softmax``, one dtype; ``out`` may be ``dy`` or ``y``."""
        y, dy, out = _softmax_vecs((("y", y), ("dy", dy)), out, self.nnz)
        if self.nnz == 0:
            return out
        import torch
        fn = self._lib.crp_csr_dev_row_softmax_bwd_f64 if y.dtype == torch.float64 else self._lib.crp_csr_dev_row_softmax_bwd_f32
        L.check(fn(self.handle, y.data_ptr(), dy.data_ptr(), out.data_ptr(), _stream(out) if stream is None else stream), fn.__name__)
        return out

    def resolved_variant(self, n):
        """crp_csr_dev_resolved_variant: what a variant-0 product of n columns launches on this matrix."""
        return int(self._lib.crp_csr_dev_resolved_variant(self.handle, int(n)))

    @property
    def last_kernel(self):
        """crp_csr_dev_last_kernel: the kernel instance the last product on this handle launched, e.g. ``panel<8,2,2,a32,b0>``."""
        return (self._lib.crp_csr_dev_last_kernel(self.handle) or b"").decode()

    @property
    def nnz(self):
        return int(self._lib.crp_csr_dev_nnz(self.handle))

    def row_part_comm_size(self, rblk_ptr, x_displs):
        """csr_mat_row_part_comm_size (src/spmat_part.c:38-64) evaluated on the device-resident CSR -> (sizes, total)."""
        rb = np.ascontiguousarray(rblk_ptr, dtype=np.int32)
        xd = np.ascontiguousarray(x_displs, dtype=np.int32)
        nblk = rb.size - 1
        sizes = np.zeros(nblk, dtype=np.int32)
        tot = C.c_int()
        L.check(self._lib.crp_csr_dev_row_part_comm_size(self.handle, nblk, rb.ctypes.data_as(L.c_int_p), xd.ctypes.data_as(L.c_int_p),
                                                         sizes.ctypes.data_as(L.c_int_p), C.byref(tot)), "crp_csr_dev_row_part_comm_size")
        return sizes, tot.value

    def free(self):
        if self.handle:
            self._lib.crp_csr_dev_destroy(C.byref(self.handle))
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _stream(t):
    import torch
    return torch.cuda.current_stream(t.device).cuda_stream


def _check_dev_vectors(named, nnz):
    """The one checker of value vectors that live on the device (``update_values_dev``, the row softmax), run before any
    library call: every (name, tensor) of ``named`` a 1-D contiguous float64 / float32 CUDA tensor of nnz entries (nnz None: as
    many as the first holds), all of one dtype and device.  TypeError for anything that is not a torch tensor, for another
    dtype and for mixed dtypes; then ValueError for a wrong dimension, strides or length; then TypeError for a tensor that is
    not on the device."""
    import torch
    head, first = named[0]
    for name, t in named:
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s must be a torch tensor on the device (host values go to update_values)" % name)
        if t.dtype not in (torch.float64, torch.float32):
            raise TypeError("%s must be float64 or float32, got %s" % (name, t.dtype))
        if t.dtype != first.dtype:
            raise TypeError("%s and %s must share one dtype (%s, %s)" % (head, name, first.dtype, t.dtype))
    for name, t in named:
        if t.dim() != 1 or not t.is_contiguous():
            raise ValueError("%s must be 1-D and contiguous" % name)
        want = first.numel() if nnz is None else nnz
        if t.numel() != want:
            raise ValueError("%s has %d entries, the call needs %d" % (name, t.numel(), want))
    for name, t in named:
        if not t.is_cuda or t.device != first.device:
            raise TypeError("%s must be on the device%s (host values go to update_values)" % (name, "" if t is first else ", with " + head))


BWD_WIDTH_CAP = {8: 512, 4: 1024}       # widest nk / nv of the fused attention backward, by the element size


def _heads(heads):
    """``heads`` of the attention calls as an int >= 1, checked before any library call"""
    if isinstance(heads, bool) or not isinstance(heads, (int, np.integer)):
        raise TypeError("heads must be an int, got %r" % (heads,))
    if heads < 1:
        raise ValueError("heads must be at least 1, got %d" % heads)
    return int(heads)


def _mh_widths(nk, nv, heads):
    if nk % heads or nv % heads:
        raise ValueError("%d heads do not divide the widths (nk = %d, nv = %d)" % (heads, nk, nv))


def _mh_flat(name, t, heads):
    """A per-row or per-nonzero tensor of a multi-head call -- contiguous, (rows, heads) -- as the flat view the single-head
    checks take; ``heads`` = 1, None and anything that is not a tensor pass through to those checks."""
    import torch
    if heads == 1 or not isinstance(t, torch.Tensor):
        return t
    if t.dim() != 2 or t.shape[1] != heads or not t.is_contiguous():
        raise ValueError("%s must be a contiguous 2-D tensor with %d columns (one per head)" % (name, heads))
    return t.view(-1)


def _attention_operands(kops, vops, vecs, scale, bias, heads=1, cap=True, by_operand=False):
    """The operands of the three attention wrappers, checked before any library call: kops 2-D of one width nk, vops 2-D of one
    width nv, all float64 or float32 of the first's dtype, their rows contiguous; ``heads`` must divide both widths.  Returns
    (nk, nv, scale, bias) as the C call takes them; the device is checked by _attention_on_device.  ``cap`` (the backward): one
    head's widths are held to BWD_WIDTH_CAP.  The order decides which error an input with two faults gets, and each wrapper keeps
    its own: by default (the backward) every type comes first and vecs are then held to 1-D and contiguous; ``by_operand`` (the
    forward) judges an operand's rows before the next one's type and leaves the shapes of vecs to the caller."""
    import torch
    head, first = kops[0]
    ops = kops + vops
    rows_now = len(ops) if by_operand else 0
    floats, dtype = (torch.float64, torch.float32), getattr(first, "dtype", None)
    for i, (name, t) in enumerate(ops + vecs):
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s must be a torch tensor on the device" % name)
        if t.dtype not in floats:
            raise TypeError("%s must be float64 or float32, got %s" % (name, t.dtype))
        if t.dtype != dtype:
            raise TypeError("the operands must have one dtype (%s is %s, %s is %s)" % (head, dtype, name, t.dtype))
        if i < rows_now:
            if t.dim() != 2:
                raise TypeError("%s must be a 2-D torch tensor on the device" % name)
            if t.size(1) > 1 and t.stride(1) != 1:
                raise ValueError("%s must be contiguous along its rows" % name)
    if not by_operand:
        for name, t in ops:
            if t.dim() != 2:
                raise TypeError("%s must be a 2-D torch tensor on the device" % name)
            if t.size(1) > 1 and t.stride(1) != 1:
                raise ValueError("%s must be contiguous along its rows" % name)
        for name, t in vecs:
            if t.dim() != 1 or not t.is_contiguous():
                raise ValueError("%s must be 1-D and contiguous" % name)
    if bias not in (False, True, 0, 1):
        raise ValueError("bias must be a bool, got %r" % (bias,))
    scale = float(scale)
    if not np.isfinite(scale):
        raise ValueError("scale must be finite, got %r" % (scale,))
    nk, nv = first.size(1), vops[0][1].size(1)
    if nk < 1 or nv < 1:
        raise ValueError("the operands need at least one column")
    for (side, n) in ((kops, nk), (vops, nv)):
        for name, t in side[1:]:
            if t.size(1) != n:
                raise ValueError("%s has %d columns, %s has %d" % (name, t.size(1), side[0][0], n))
    _mh_widths(nk, nv, heads)
    if cap:
        cap = BWD_WIDTH_CAP[first.element_size()]
        if nk // heads > cap or nv // heads > cap:
            raise ValueError("the fused backward takes at most %d columns%s in %s (nk = %d, nv = %d)"
                             % (cap, "" if heads == 1 else " per head", first.dtype, nk // heads, nv // heads))
    return nk, nv, scale, int(bool(bias))


def _gat_operands(sops, vops, vecs, slope, bias, heads, cap=True):
    """The operands of the three GAT wrappers, checked before any library call: sops 2-D with ``heads`` columns (el, er, their
    gradients), vops 2-D of one width that ``heads`` divides, vecs per-row or per-nonzero tensors, all float64 or float32 of the
    first's dtype, rows contiguous.  Returns (nv, slope, bias) as the C call takes them -- nv the whole width of V; the device is
    checked by _attention_on_device.  ``cap`` (the backward): one head's width is held to BWD_WIDTH_CAP."""
    import torch
    head, first = sops[0]
    floats, dtype = (torch.float64, torch.float32), getattr(first, "dtype", None)
    for name, t in sops + vops + vecs:
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s must be a torch tensor on the device" % name)
        if t.dtype not in floats:
            raise TypeError("%s must be float64 or float32, got %s" % (name, t.dtype))
        if t.dtype != dtype:
            raise TypeError("the operands must have one dtype (%s is %s, %s is %s)" % (head, dtype, name, t.dtype))
    for name, t in sops + vops:
        if t.dim() != 2:
            raise TypeError("%s must be a 2-D torch tensor on the device" % name)
        if t.size(1) > 1 and t.stride(1) != 1:
            raise ValueError("%s must be contiguous along its rows" % name)
    if bias not in (False, True, 0, 1):
        raise ValueError("bias must be a bool, got %r" % (bias,))
    slope = float(slope)
    if not np.isfinite(slope):
        raise ValueError("slope must be finite, got %r" % (slope,))
    for name, t in sops:
        if t.size(1) != heads:
            raise ValueError("%s has %d columns, the call %d heads" % (name, t.size(1), heads))
    nv = vops[0][1].size(1)
    if nv < 1:
        raise ValueError("the operands need at least one column")
    for name, t in vops[1:]:
        if t.size(1) != nv:
            raise ValueError("%s has %d columns, %s has %d" % (name, t.size(1), vops[0][0], nv))
    if nv % heads:
        raise ValueError("%d heads do not divide the width (nv = %d)" % (heads, nv))
    if cap:
        cap = BWD_WIDTH_CAP[first.element_size()]
        if nv // heads > cap:
            raise ValueError("the fused backward takes at most %d columns per head in %s (dv = %d)" % (cap, first.dtype, nv // heads))
    return nv, slope, int(bool(bias))


def _dropout(dropout, seed):
    """(rate, seed) of the attention dropout as the C calls take them, checked before any library call: a rate in [0, 1), a seed
    of 64 bits"""
    try:
        rate = float(dropout)
    except (TypeError, ValueError):
        raise TypeError("dropout must be a number, got %r" % (dropout,))
    if not (0.0 <= rate < 1.0):
        raise ValueError("dropout must lie in [0, 1), got %r" % (dropout,))
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)):
        raise TypeError("seed must be an integer, got %r" % (seed,))
    if not (0 <= int(seed) < 1 << 64):
        raise ValueError("seed must lie in [0, 2^64), got %r" % (seed,))
    return rate, int(seed)


def _drop_entry(lib, family, side, f32, dropout, seed):
    """(entry point, the arguments it takes before the stream) of a GAT / GATv2 call: the plain one for dropout == 0"""
    dt = "f32" if f32 else "f64"
    if dropout == 0.0:
        return getattr(lib, "crp_%s%s_csr_%s" % (family, side, dt)), ()
    return getattr(lib, "crp_%s_drop%s_csr_%s" % (family, side, dt)), (dropout, seed)


def dropout_keep(seed, r, c, h, dropout):
    """crp_dropout_keep_host: whether the attention dropout of the fused GAT / GATv2 calls keeps edge (r, c) in head h -- word 0
    of Philox4x32-10 with key = the seed's two words and counter (r, c, h, 0), held against floor(dropout * 2^32).  ``r``: the row
    of the output; ``c``: the 32-bit column code (a negative code counts as its bit pattern).  Host code: needs no device."""
    dropout, seed = _dropout(dropout, seed)
    rc = L.load().crp_dropout_keep_host(seed, int(r) & 0xFFFFFFFF, int(c) & 0xFFFFFFFF, int(h) & 0xFFFFFFFF, dropout)
    if rc < 0:
        raise ValueError("crp_dropout_keep_host refused its arguments")
    return bool(rc)


def _gat_flat(name, t, heads):
    """A per-row or per-nonzero tensor of a GAT call -- contiguous (rows, heads), or 1-D with one head -- as a flat view"""
    if t is None:
        return t
    if t.dim() == 1 and heads == 1 and t.is_contiguous():
        return t
    if t.dim() != 2 or t.shape[1] != heads or not t.is_contiguous():
        raise ValueError("%s must be a contiguous 2-D tensor with %d columns (one per head)" % (name, heads))
    return t.view(-1)


def _gat_out_pos(out_pos, out, name, nnz, heads):
    """``out_pos`` and the per-nonzero output (flat) it indexes, as the attention wrappers check them"""
    import torch
    if out_pos is not None:
        if not (isinstance(out_pos, torch.Tensor) and out_pos.dtype == torch.int32 and out_pos.dim() == 1 and out_pos.is_contiguous()):
            raise TypeError("out_pos must be a contiguous 1-D int32 torch tensor on the device")
        if out_pos.numel() != nnz:
            raise ValueError("out_pos has %d entries, the matrix %d nonzeros" % (out_pos.numel(), nnz))
        if out is None:
            raise ValueError("out_pos needs a %s to write into" % name)
    elif out is not None and out.numel() < nnz * heads:
        raise ValueError("%s has %d rows, the matrix %d nonzeros" % (name, out.numel() // heads, nnz))


def _gatv2_operands(vops, vecs, a, slope, bias, heads):
    """The operands of the three GATv2 wrappers, checked before any library call: vops 2-D of one width that ``heads`` divides,
    vecs per-row or per-nonzero tensors, ``a`` that many contiguous elements, all float64 or float32 of the first's dtype, rows
    contiguous; one head's width is held to BWD_WIDTH_CAP in both directions.  Returns (nv, slope, bias) as the C call takes them
    -- nv the whole width; the device is checked by _attention_on_device."""
    import torch
    head, first = vops[0]
    floats, dtype = (torch.float64, torch.float32), getattr(first, "dtype", None)
    for name, t in vops + [("a", a)] + vecs:
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s must be a torch tensor on the device" % name)
        if t.dtype not in floats:
            raise TypeError("%s must be float64 or float32, got %s" % (name, t.dtype))
        if t.dtype != dtype:
            raise TypeError("the operands must have one dtype (%s is %s, %s is %s)" % (head, dtype, name, t.dtype))
    for name, t in vops:
        if t.dim() != 2:
            raise TypeError("%s must be a 2-D torch tensor on the device" % name)
        if t.size(1) > 1 and t.stride(1) != 1:
            raise ValueError("%s must be contiguous along its rows" % name)
    if bias not in (False, True, 0, 1):
        raise ValueError("bias must be a bool, got %r" % (bias,))
    slope = float(slope)
    if not np.isfinite(slope):
        raise ValueError("slope must be finite, got %r" % (slope,))
    nv = first.size(1)
    if nv < 1:
        raise ValueError("the operands need at least one column")
    for name, t in vops[1:]:
        if t.size(1) != nv:
            raise ValueError("%s has %d columns, %s has %d" % (name, t.size(1), head, nv))
    if nv % heads:
        raise ValueError("%d heads do not divide the width (nv = %d)" % (heads, nv))
    if a.dim() not in (1, 2) or a.numel() != nv or not a.is_contiguous() or (a.dim() == 2 and a.size(0) != heads):
        raise ValueError("a must hold heads * dv = %d contiguous elements, 1-D or (heads, dv); it is %s" % (nv, tuple(a.shape)))
    cap = BWD_WIDTH_CAP[first.element_size()]
    if nv // heads > cap:
        raise ValueError("the fused GATv2 attention takes at most %d columns per head in %s (dv = %d)" % (cap, first.dtype, nv // heads))
    return nv, slope, int(bool(bias))


def _attention_on_device(named):
    """... and, after every shape check, all of them on the first's device (all pointers are device pointers)"""
    head, first = named[0]
    for name, t in named:
        if not t.is_cuda or t.device != first.device:
            raise TypeError("%s must be on the device, with %s" % (name, head))


def _softmax_vecs(named, out, nnz):
    """The value tensors of a row softmax call through ``_check_dev_vectors``; ``out`` is allocated like the first when None.
    Returns the tensors, out last."""
    import torch
    _check_dev_vectors(tuple(named) + ((("out", out),) if out is not None else ()), nnz)
    if out is None:
        out = torch.empty_like(named[0][1])
    return tuple(t for _, t in named) + (out,)


def _softmax_rowptr(rowptr, like):
    import torch
    if not isinstance(rowptr, torch.Tensor) or rowptr.dtype != torch.int32:
        raise TypeError("rowptr must be an int32 torch tensor on the device")
    if rowptr.dim() != 1 or not rowptr.is_contiguous() or rowptr.numel() < 1:
        raise ValueError("rowptr must be 1-D and contiguous, with nrow + 1 entries")
    if not rowptr.is_cuda or rowptr.device != like.device:
        raise TypeError("rowptr must be on the device, with the values")
    return rowptr.numel() - 1


def row_softmax(rowptr, s, out=None, stream=None):
    """Row softmax over a CSR pattern (crp_row_softmax_f64 / _f32, by the dtype of ``s``): ``rowptr`` is an int32 cuda tensor
    of nrow + 1 non-decreasing entries that index ``s`` and ``out`` directly (rowptr[0] need not be 0: a slice ``rowptr[r0:r1]``
    addresses a row subset of the same tensors; the entries must lie inside ``s``, which cannot be checked without a
    download).  ``s`` is a 1-D contiguous float64 or float32 cuda tensor, ``out`` one of the same length (allocated when None;
    only the entries the rows name are written; ``out is s`` is allowed).  Returns ``out``."""
    import torch
    s, out = _softmax_vecs((("s", s),), out, None)
    nrow = _softmax_rowptr(rowptr, s)
    if nrow == 0 or s.numel() == 0:
        return out
    fn = L.load().crp_row_softmax_f64 if s.dtype == torch.float64 else L.load().crp_row_softmax_f32
    L.check(fn(nrow, rowptr.data_ptr(), s.data_ptr(), out.data_ptr(), _stream(out) if stream is None else stream), fn.__name__)
    return out


def row_softmax_bwd(rowptr, y, dy, out=None, stream=None):
    """The Jacobian product of ``row_softmax`` (crp_row_softmax_bwd_f64 / _f32): out[p] = y[p] * (dy[p] - D), D = the row's sum
    of y * dy.  Arguments as ``row_softmax``; ``out`` may be ``dy`` or ``y``."""
    import torch
    y, dy, out = _softmax_vecs((("y", y), ("dy", dy)), out, None)
    nrow = _softmax_rowptr(rowptr, y)
    if nrow == 0 or y.numel() == 0:
        return out
    fn = L.load().crp_row_softmax_bwd_f64 if y.dtype == torch.float64 else L.load().crp_row_softmax_bwd_f32
    L.check(fn(nrow, rowptr.data_ptr(), y.data_ptr(), dy.data_ptr(), out.data_ptr(), _stream(out) if stream is None else stream),
            fn.__name__)
    return out


def sparse_attention(A, At, Q, K, V, scale=1.0, bias=False, heads=1):
    """softmax_row(scale * (Q K^T)|pattern(A) (+ A's values with ``bias``)) V as a differentiable function of Q, K and V: ``A`` is
    the ``CsrDev`` of the pattern, ``At`` the ``CsrDev.from_transpose`` of the same CSR (with ``bias`` both hold the same
    values).  The forward is ``A.attention``, which keeps O and lse; the backward is ``A.attention_bwd_q`` and
    ``At.attention_bwd_kv``.  Nothing nnz-sized is stored between the two.  2-D row-major cuda tensors of one dtype.  The
    matrix's values are constants here: with ``bias`` they enter the scores and get no gradient (``attention_bwd_q`` with
    ``ds_out`` forms it).  ``At`` must be the transpose of ``A``: its shape and nonzero count are checked, its pattern is not.
    ``heads`` > 1: Q, K, V hold ``heads`` heads side by side (the widths must divide); the result and the gradients are, bit for
    bit, the per-head single-head results side by side."""
    heads = _heads(heads)
    _mh_widths(int(Q.shape[-1]), int(V.shape[-1]), heads)
    if At.nrow != A.ncol or At.ncol != A.nrow or At.nnz != A.nnz:
        raise ValueError("At is %d x %d with %d nonzeros: not the transpose of A (%d x %d, %d)"
                         % (At.nrow, At.ncol, At.nnz, A.nrow, A.ncol, A.nnz))
    return _sparse_attention_fn().apply(Q, K, V, A, At, float(scale), bool(bias), heads)


_SPARSE_ATTENTION_FN = None


def _sparse_attention_fn():
    """the autograd.Function behind ``sparse_attention``, made on first use (this module imports torch only where it is used)"""
    global _SPARSE_ATTENTION_FN
    if _SPARSE_ATTENTION_FN is not None:
        return _SPARSE_ATTENTION_FN
    import torch

    class SparseAttention(torch.autograd.Function):
        @staticmethod
        def forward(ctx, Q, K, V, A, At, scale, bias, heads=1):
            Q, K, V = (t if t.stride(-1) == 1 else t.contiguous() for t in (Q.detach(), K.detach(), V.detach()))
            lse = torch.empty((Q.shape[0],) if heads == 1 else (Q.shape[0], heads), dtype=Q.dtype, device=Q.device)
            O = A.attention(Q, K, V, scale=scale, bias=bias, lse=lse, heads=heads)
            ctx.save_for_backward(Q, K, V, O, lse)
            ctx.handles = (A, At, scale, bias, heads)
            return O

        @staticmethod
        def backward(ctx, dO):
            Q, K, V, O, lse = ctx.saved_tensors
            A, At, scale, bias, heads = ctx.handles
            dO = dO if dO.stride(-1) == 1 else dO.contiguous()
            dQ, delta = A.attention_bwd_q(Q, K, V, O, dO, lse, scale=scale, bias=bias, heads=heads)
            dK, dV = At.attention_bwd_kv(K, V, Q, dO, lse, delta, scale=scale, bias=bias, heads=heads)
            return dQ, dK, dV, None, None, None, None, None

    _SPARSE_ATTENTION_FN = SparseAttention
    return SparseAttention


def gat_attention(A, At, el, er, V, slope=0.2, bias=False, heads=1, dropout=0.0, seed=None):
    """The GAT layer's attention, out[i]_h = sum_p softmax_p(leaky_relu(el[i, h] + er[c_p, h], slope) (+ A's values with ``bias``))
    V[c_p]_h, as a differentiable function of el, er and V: ``A`` is the ``CsrDev`` of the pattern, ``At`` the
    ``CsrDev.from_transpose`` of the same CSR (with ``bias`` both hold the same values).  The forward is ``A.gat_attention``,
    which keeps O and lse; the backward is ``A.gat_attention_bwd_row`` and ``At.gat_attention_bwd_col``.  Nothing nnz-sized is
    stored between the two.  ``el`` (rows, heads), ``er`` (columns, heads) and ``V`` (columns, heads * dv) are 2-D row-major cuda
    tensors of one dtype.  The matrix's values are constants here.  ``At`` must be the transpose of ``A``: its shape and nonzero
    count are checked, its pattern is not.  ``dropout`` > 0 (training; evaluation passes 0) drops the attention coefficients
    after the softmax and scales the kept ones by 1 / (1 - dropout); no mask is stored, the backward re-forms it from ``seed``,
    which is kept beside O and lse.  ``seed`` None draws 64 bits from torch's default host generator once per call, so that
    ``torch.manual_seed`` reproduces a run."""
    heads = _heads(heads)
    if At.nrow != A.ncol or At.ncol != A.nrow or At.nnz != A.nnz:
        raise ValueError("At is %d x %d with %d nonzeros: not the transpose of A (%d x %d, %d)"
                         % (At.nrow, At.ncol, At.nnz, A.nrow, A.ncol, A.nnz))
    dropout, seed = _autograd_dropout(dropout, seed)
    return _gat_attention_fn().apply(el, er, V, A, At, float(slope), bool(bias), heads, dropout, seed)


def _autograd_dropout(dropout, seed):
    """(rate, seed) of a differentiable GAT / GATv2 call: without a seed, 64 bits from torch's default host generator"""
    rate, _ = _dropout(dropout, 0)
    if seed is None:
        if rate == 0.0:
            return rate, 0
        import torch
        hi, lo = (int(x) for x in torch.randint(0, 1 << 32, (2,), dtype=torch.int64))
        return rate, (hi << 32) | lo
    return _dropout(rate, seed)


_GAT_ATTENTION_FN = None


def _gat_attention_fn():
    """the autograd.Function behind ``gat_attention``, made on first use"""
    global _GAT_ATTENTION_FN
    if _GAT_ATTENTION_FN is not None:
        return _GAT_ATTENTION_FN
    import torch

    class GatAttention(torch.autograd.Function):
        @staticmethod
        def forward(ctx, el, er, V, A, At, slope, bias, heads, dropout=0.0, seed=0):
            el, er, V = (t if t.dim() != 2 or t.stride(-1) == 1 else t.contiguous() for t in (el.detach(), er.detach(), V.detach()))
            lse = torch.empty((el.shape[0], heads), dtype=el.dtype, device=el.device)
            O = A.gat_attention(el, er, V, slope=slope, bias=bias, lse=lse, heads=heads, dropout=dropout, seed=seed)
            ctx.save_for_backward(el, er, V, O, lse)
            ctx.handles = (A, At, slope, bias, heads, dropout, seed)
            return O

        @staticmethod
        def backward(ctx, dO):
            el, er, V, O, lse = ctx.saved_tensors
            A, At, slope, bias, heads, dropout, seed = ctx.handles
            dO = dO if dO.stride(-1) == 1 else dO.contiguous()
            d_el, delta = A.gat_attention_bwd_row(el, er, V, O, dO, lse, slope=slope, bias=bias, heads=heads, dropout=dropout, seed=seed)
            d_er, dV = At.gat_attention_bwd_col(er, V, el, dO, lse, delta, slope=slope, bias=bias, heads=heads, dropout=dropout,
                                                seed=seed)
            return d_el, d_er, dV, None, None, None, None, None, None, None

    _GAT_ATTENTION_FN = GatAttention
    return GatAttention


def col_sum(src, out=None, stream=None):
    """Column sums of a 2-D row-major float64 or float32 cuda tensor (crp_col_sum_f64 / _f32): blocks of 256 consecutive rows
    are summed per column from +0 in ascending row, and the block sums are added left to right -- a fixed order, no atomics,
    so the bits depend on the dtype, the shape and the data only.  ``out`` (contiguous, one element per column) is allocated
    when None.  Returns ``out``.  Every error is raised before the library is called."""
    import torch
    if not isinstance(src, torch.Tensor) or src.dim() != 2:
        raise TypeError("src must be a 2-D torch tensor on the device")
    if src.dtype not in (torch.float64, torch.float32):
        raise TypeError("src must be float64 or float32, got %s" % (src.dtype,))
    if src.size(0) > 0 and src.size(1) > 1 and src.stride(1) != 1:
        raise ValueError("src must be contiguous along its rows")
    nrow, n = src.shape
    if out is not None:
        if not isinstance(out, torch.Tensor) or out.dtype != src.dtype:
            raise TypeError("out must be a torch tensor of src's dtype")
        if out.numel() != n or not out.is_contiguous():
            raise ValueError("out must hold %d contiguous elements" % n)
    _attention_on_device([("src", src)] + ([("out", out)] if out is not None else []))
    if out is None:
        out = torch.empty((n,), dtype=src.dtype, device=src.device)
    if n == 0:
        return out
    work = torch.empty((max(1, (nrow + 255) // 256) * n,), dtype=src.dtype, device=src.device)
    lib = L.load()
    fn = lib.crp_col_sum_f32 if src.dtype == torch.float32 else lib.crp_col_sum_f64
    L.check(fn(nrow, n, src.data_ptr() or None, max(src.stride(0), n), work.data_ptr(), out.data_ptr(),
               _stream(out) if stream is None else stream), fn.__name__)
    return out


def gatv2_attention(A, At, XT, XS, a, slope=0.2, bias=False, heads=1, dropout=0.0, seed=None):
    """The GATv2 layer's attention, out[i]_h = sum_p softmax_p(sum_j a[h, j] leaky_relu(XT[i]_h[j] + XS[c_p]_h[j], slope) (+ A's
    values with ``bias``)) XS[c_p]_h, as a differentiable function of XT, XS and a: ``A`` is the ``CsrDev`` of the pattern, ``At``
    the ``CsrDev.from_transpose`` of the same CSR (with ``bias`` both hold the same values).  The forward is
    ``A.gatv2_attention``, which keeps O and lse; the backward is ``A.gatv2_attention_bwd_row``, ``At.gatv2_attention_bwd_col`` and
    ``col_sum`` of the rows' shares of the gradient of ``a``.  Nothing nnz-sized is stored.  ``XT`` (rows, heads * dv) and ``XS``
    (columns, heads * dv) are 2-D row-major cuda tensors of one dtype, ``a`` holds heads * dv elements (1-D or (heads, dv)).  One
    tensor may be passed as XT and XS (shared weights): its gradient is the sum of both.  The matrix's values are constants here.
    ``At`` must be the transpose of ``A``: its shape and nonzero count are checked, its pattern is not.  ``dropout`` and ``seed``
    as in ``gat_attention``."""
    heads = _heads(heads)
    if At.nrow != A.ncol or At.ncol != A.nrow or At.nnz != A.nnz:
        raise ValueError("At is %d x %d with %d nonzeros: not the transpose of A (%d x %d, %d)"
                         % (At.nrow, At.ncol, At.nnz, A.nrow, A.ncol, A.nnz))
    dropout, seed = _autograd_dropout(dropout, seed)
    return _gatv2_attention_fn().apply(XT, XS, a, A, At, float(slope), bool(bias), heads, dropout, seed)


_GATV2_ATTENTION_FN = None


def _gatv2_attention_fn():
    """the autograd.Function behind ``gatv2_attention``, made on first use"""
    global _GATV2_ATTENTION_FN
    if _GATV2_ATTENTION_FN is not None:
        return _GATV2_ATTENTION_FN
    import torch

    class Gatv2Attention(torch.autograd.Function):
        @staticmethod
        def forward(ctx, XT, XS, a, A, At, slope, bias, heads, dropout=0.0, seed=0):
            XT, XS = (t if t.dim() != 2 or t.stride(-1) == 1 else t.contiguous() for t in (XT.detach(), XS.detach()))
            a = a.detach().contiguous()
            lse = torch.empty((XT.shape[0], heads), dtype=XT.dtype, device=XT.device)
            O = A.gatv2_attention(XT, XS, a, slope=slope, bias=bias, lse=lse, heads=heads, dropout=dropout, seed=seed)
            ctx.save_for_backward(XT, XS, a, O, lse)
            ctx.handles = (A, At, slope, bias, heads, dropout, seed)
            return O

        @staticmethod
        def backward(ctx, dO):
            XT, XS, a, O, lse = ctx.saved_tensors
            A, At, slope, bias, heads, dropout, seed = ctx.handles
            dO = dO if dO.stride(-1) == 1 else dO.contiguous()
            dXT = da_part = None
            if getattr(A, "_x_nrow", A.nrow) != A.nrow:         # a row subset writes the rows it names: the others are zero
                dXT, da_part = torch.zeros_like(XT), torch.zeros_like(XT)
            dXT, da_part, delta = A.gatv2_attention_bwd_row(XT, XS, a, O, dO, lse, slope=slope, bias=bias, dXT=dXT, da_part=da_part,
                                                            heads=heads, dropout=dropout, seed=seed)
            dXS = At.gatv2_attention_bwd_col(XS, XT, a, dO, lse, delta, slope=slope, bias=bias, heads=heads, dropout=dropout, seed=seed)
            da = col_sum(da_part).view(a.shape)
            return dXT, dXS, da, None, None, None, None, None, None, None

    _GATV2_ATTENTION_FN = Gatv2Attention
    return Gatv2Attention


def spmm_csr(A, B0, C_out, n=None, layout=0, B1=None, variant=0, stream=None):
    """C_out := A * B (crp_spmm_csr_f64). B0 / B1 / C_out are 2-D float64 cuda tensors;
    layout 1 operands are passed as (n, ld) tensors holding the column-major data."""
    lib = L.load()
    if layout == 0:
        n = C_out.shape[1] if n is None else n
    else:
        n = C_out.shape[0] if n is None else n
    b1p, ld1 = (B1.data_ptr(), B1.stride(0)) if B1 is not None else (None, 0)
    L.check(lib.crp_spmm_csr_f64(A.handle, layout, n, B0.data_ptr() if B0 is not None else None,
                                 B0.stride(0) if B0 is not None else 0, b1p, ld1, C_out.data_ptr(),
                                 C_out.stride(0), variant, _stream(C_out) if stream is None else stream),
            "crp_spmm_csr_f64")


def csr_transpose(rowptr, colidx, val, ncol, stream=None):
    """crp_csr_transpose -> (rowptr_t, colidx_t, val_t, tmap): A^T of the CSR (rowptr, colidx, val) with ncol columns;
    tmap[q] = position in the input of output entry q.  numpy arrays: host code; torch tensors on the GPU (int32 rowptr /
    colidx, float64 val): the HIP kernels on `stream` (default: the current torch stream), results as tensors on the same
    device.  A bad input raises TransposeError with the C code."""
    lib = L.load()
    try:
        import torch
        tensors = [isinstance(t, torch.Tensor) and t.is_cuda for t in (rowptr, colidx, val)]
    except ImportError:
        tensors = [False] * 3
    ncol = int(ncol)
    if any(tensors):
        import torch
        if not all(tensors):
            raise TransposeError("csr_transpose", T_EMIXED)
        for t, dt in ((rowptr, torch.int32), (colidx, torch.int32), (val, torch.float64)):
            if t.dtype != dt or not t.is_contiguous():
                raise TransposeError("csr_transpose", T_EARG)
        nrow, nnz = rowptr.numel() - 1, colidx.numel()
        if nrow < 0 or ncol < 0 or val.numel() != nnz:
            raise TransposeError("csr_transpose", T_EARG)
        dev = rowptr.device
        rowptr_t = torch.empty(ncol + 1, dtype=torch.int32, device=dev)
        colidx_t = torch.empty(max(nnz, 1), dtype=torch.int32, device=dev)
        val_t = torch.empty(max(nnz, 1), dtype=torch.float64, device=dev)
        tmap = torch.empty(max(nnz, 1), dtype=torch.int32, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
        rc = lib.crp_csr_transpose(nrow, ncol, C.c_void_p(rowptr.data_ptr()), C.c_void_p(colidx.data_ptr() or None),
                                   C.c_void_p(val.data_ptr() or None), C.c_void_p(rowptr_t.data_ptr()),
                                   C.c_void_p(colidx_t.data_ptr()), C.c_void_p(val_t.data_ptr()), C.c_void_p(tmap.data_ptr()),
                                   C.c_void_p(st))
    else:
        rowptr = np.ascontiguousarray(rowptr, dtype=np.int32)
        colidx = np.ascontiguousarray(colidx, dtype=np.int32)
        val = np.ascontiguousarray(val, dtype=np.float64)
        nrow, nnz = rowptr.size - 1, colidx.size
        if nrow < 0 or ncol < 0 or val.size != nnz:
            raise TransposeError("csr_transpose", T_EARG)
        rowptr_t = np.zeros(ncol + 1, np.int32)
        colidx_t = np.zeros(max(nnz, 1), np.int32)
        val_t = np.zeros(max(nnz, 1), np.float64)
        tmap = np.zeros(max(nnz, 1), np.int32)
        ci = colidx if nnz else np.zeros(1, np.int32)
        va = val if nnz else np.zeros(1, np.float64)
        rc = lib.crp_csr_transpose(nrow, ncol, rowptr.ctypes.data, ci.ctypes.data, va.ctypes.data, rowptr_t.ctypes.data,
                                   colidx_t.ctypes.data, val_t.ctypes.data, tmap.ctypes.data, None)
    if rc < 0:
        raise TransposeError("crp_csr_transpose", rc)
    L.check(rc, "crp_csr_transpose")
    return rowptr_t, colidx_t[:nnz], val_t[:nnz], tmap[:nnz]


def gather_rows(ridx, src, dst, layout=0, scatter=False, stream=None):
    lib = L.load()
    fn = lib.crp_scatter_rows_f64 if scatter else lib.crp_gather_rows_f64
    if layout == 0:
        n = (src if scatter else dst).shape[1]
    else:
        n = (src if scatter else dst).shape[0]
    L.check(fn(layout, ridx.numel(), n, ridx.data_ptr(), src.data_ptr(), src.stride(0), dst.data_ptr(),
               dst.stride(0), _stream(dst) if stream is None else stream), "crp_gather/scatter_rows_f64")


def transpose(src, dst, stream=None):
    lib = L.load()
    L.check(lib.crp_transpose_f64(src.shape[0], src.shape[1], src.data_ptr(), src.stride(0), dst.data_ptr(),
                                  dst.stride(0), _stream(dst) if stream is None else stream), "crp_transpose_f64")


def gather_rows_f32(ridx, src, dst, layout=0, stream=None):
    """crp_gather_rows_f32: dst[i] = src[ridx[i]] (rows; layout 1: columns of (n, ld) tensors) on float32 cuda tensors."""
    _move_rows_f32(ridx, src, dst, layout, False, stream)


def scatter_rows_f32(ridx, src, dst, layout=0, stream=None):
    """crp_scatter_rows_f32: dst[ridx[i]] = src[i]."""
    _move_rows_f32(ridx, src, dst, layout, True, stream)


def _move_rows_f32(ridx, src, dst, layout, scatter, stream):
    lib = L.load()
    fn = lib.crp_scatter_rows_f32 if scatter else lib.crp_gather_rows_f32
    n = (src if scatter else dst).shape[1 if layout == 0 else 0]
    L.check(fn(layout, ridx.numel(), n, ridx.data_ptr(), src.data_ptr(), src.stride(0), dst.data_ptr(),
               dst.stride(0), _stream(dst) if stream is None else stream), "crp_gather/scatter_rows_f32")


def transpose_f32(src, dst, stream=None):
    """crp_transpose_f32: dst[c][r] = src[r][c] on float32 cuda tensors."""
    lib = L.load()
    L.check(lib.crp_transpose_f32(src.shape[0], src.shape[1], src.data_ptr(), src.stride(0), dst.data_ptr(),
                                  dst.stride(0), _stream(dst) if stream is None else stream), "crp_transpose_f32")


def device_info(dev=0):
    lib = L.load()
    name = C.create_string_buffer(256)
    cu, mem = C.c_int(), C.c_size_t()
    L.check(lib.crp_hip_device_info(dev, name, C.byref(cu), C.byref(mem)), "crp_hip_device_info")
    return name.value.decode(), cu.value, mem.value


def panel_format_host(rowptr, colidx, val, R):
    """Host-only view of the row-panel format (crp_panel_format_host) as numpy arrays."""
    lib = L.load()
    rp = np.ascontiguousarray(rowptr, dtype=np.int32)
    ci = np.ascontiguousarray(colidx, dtype=np.int32)
    va = np.ascontiguousarray(val, dtype=np.float64)
    if ci.size == 0:
        ci, va = np.zeros(1, np.int32), np.zeros(1, np.float64)
    npanel, ent, nord = C.c_int(), C.c_longlong(), C.c_int()
    pptr, pcol, pmask, pval, pord = L.c_int_p(), L.c_int_p(), C.POINTER(C.c_uint)(), L.c_dbl_p(), L.c_int_p()
    L.check(lib.crp_panel_format_host(rp.size - 1, rp.ctypes.data_as(L.c_int_p), ci.ctypes.data_as(L.c_int_p),
                                      va.ctypes.data_as(L.c_dbl_p), R, C.byref(npanel), C.byref(pptr), C.byref(pcol),
                                      C.byref(pmask), C.byref(pval), C.byref(ent), C.byref(pord), C.byref(nord)),
            "crp_panel_format_host")
    P = npanel.value
    pp = np.ctypeslib.as_array(pptr, (P + 1,)).copy()
    tot = int(pp[P])
    out = dict(R=R, npanel=P, pptr=pp, real_entries=ent.value,
               porder=np.ctypeslib.as_array(pord, (max(nord.value, 1),))[:nord.value].copy(),
               pcol=np.ctypeslib.as_array(pcol, (max(tot, 1),))[:tot].copy(),
               pmask4=np.ctypeslib.as_array(pmask, (tot // 4 + 2,)).copy(),
               pval=np.ctypeslib.as_array(pval, (max(tot * R, 1),))[:tot * R].copy().reshape(tot, R))
    for p in (pptr, pcol, pmask, pval, pord):
        L.c_free(C.cast(p, C.c_void_p))
    return out


def team_format_host(rowptr, colidx, val):
    """crp_team_format_host -> dict(nteam, lattice, tpanel, tptr, tcol, tmask, torder)."""
    lib = L.load()
    rp = np.ascontiguousarray(rowptr, dtype=np.int32)
    ci = np.ascontiguousarray(colidx, dtype=np.int32)
    va = np.ascontiguousarray(val, dtype=np.float64)
    if ci.size == 0:
        ci, va = np.zeros(1, np.int32), np.zeros(1)
    nteam, lat = C.c_int(), C.c_int()
    tp, tt, tc, to = L.c_int_p(), L.c_int_p(), L.c_int_p(), L.c_int_p()
    tm = C.POINTER(C.c_uint)()
    L.check(lib.crp_team_format_host(rp.size - 1, rp.ctypes.data_as(L.c_int_p), ci.ctypes.data_as(L.c_int_p),
                                     va.ctypes.data_as(L.c_dbl_p), C.byref(nteam), C.byref(lat), C.byref(tp), C.byref(tt),
                                     C.byref(tc), C.byref(tm), C.byref(to)), "crp_team_format_host")
    nt = nteam.value

    def take(ptr, cnt, dt):
        out = np.ctypeslib.as_array(ptr, (max(cnt, 1),))[:cnt].astype(dt).copy()
        L.c_free(C.cast(ptr, C.c_void_p))
        return out
    tptr = take(tt, nt + 1, np.int32)
    tot = int(tptr[-1]) if nt else 0
    return dict(nteam=nt, lattice=bool(lat.value), tpanel=take(tp, 4 * nt, np.int32).reshape(nt, 4), tptr=tptr,
                tcol=take(tc, tot, np.int32), tmask=take(tm, tot, np.uint32), torder=take(to, nt, np.int32))


def team2_format_host(rowptr, colidx, val):
    """crp_team2_format_host -> dict(nteam, waves W = 8, lattice, tpanel[nteam, 8], tinfo[nteam, 4], tpro[nteam, 3, 8, 2],
    trec (uint32 words), tvoff (units of 4 values), tval (the value streams), torder, vmap, tgrid[8, entries per XCD])."""
    lib = L.load()
    rp = np.ascontiguousarray(rowptr, dtype=np.int32)
    ci = np.ascontiguousarray(colidx, dtype=np.int32)
    va = np.ascontiguousarray(val, dtype=np.float64)
    nnz = int(rp[-1])
    if ci.size == 0:
        ci, va = np.zeros(1, np.int32), np.zeros(1)
    nteam, lat = C.c_int(), C.c_int()
    tp, ti, tpr, to = L.c_int_p(), L.c_int_p(), L.c_int_p(), L.c_int_p()
    tr, vm = C.POINTER(C.c_uint)(), C.POINTER(C.c_uint)()
    tv = C.POINTER(C.c_longlong)()
    tval = L.c_dbl_p()
    nrw, nve = C.c_longlong(), C.c_longlong()
    L.check(lib.crp_team2_format_host(rp.size - 1, rp.ctypes.data_as(L.c_int_p), ci.ctypes.data_as(L.c_int_p),
                                      va.ctypes.data_as(L.c_dbl_p), C.byref(nteam), C.byref(lat), C.byref(tp), C.byref(ti),
                                      C.byref(tpr), C.byref(tr), C.byref(nrw), C.byref(tv), C.byref(tval), C.byref(nve),
                                      C.byref(to), C.byref(vm)), "crp_team2_format_host")
    nt = nteam.value
    P, W = 1, 8
    tg, ng = L.c_int_p(), C.c_int()
    L.check(lib.crp_team2_format_host_grid(C.byref(tg), C.byref(ng)), "crp_team2_format_host_grid")

    def take(ptr, cnt, dt):
        out = np.ctypeslib.as_array(ptr, (max(cnt, 1),))[:cnt].astype(dt).copy()
        L.c_free(C.cast(ptr, C.c_void_p))
        return out
    return dict(nteam=nt, waves=W, panels_per_wave=P, compact=bool(lib.crp_team2_format_host_compact()), lattice=bool(lat.value), tpanel=take(tp, W * P * nt, np.int32).reshape(nt, W * P),
                tinfo=take(ti, 4 * nt, np.int32).reshape(nt, 4), tpro=take(tpr, 6 * W * nt, np.int32).reshape(nt, 3, W, 2),
                trec=take(tr, nrw.value, np.uint32), tvoff=take(tv, W * nt + 1, np.int64),
                tval=take(tval, nve.value, np.float64), torder=take(to, nt, np.int32),
                vmap=take(vm, nnz, np.uint32), tgrid=take(tg, ng.value, np.int32).reshape(8, -1))


def team2r_format_host(rowptr, colidx, val, G=4):
    """crp_team2r_format_host -> dict(G, nteam, lattice, tpanel[nteam, 8], tinfo[nteam, 2], trec[rounds, 8, 16] (uint32), tvoff (units
    of 16 bytes), tval (the streams as float64 words; view as uint16 for the offsets), tgrid[8, -1], vmap, rounds, steps, slots_filled, nnz)."""
    lib = L.load()
    rp = np.ascontiguousarray(rowptr, dtype=np.int32)
    ci = np.ascontiguousarray(colidx, dtype=np.int32)
    va = np.ascontiguousarray(val, dtype=np.float64)
    nnz = int(rp[-1])
    if ci.size == 0:
        ci, va = np.zeros(1, np.int32), np.zeros(1)
    nteam, lat, ng = C.c_int(), C.c_int(), C.c_int()
    tp, ti, tg = L.c_int_p(), L.c_int_p(), L.c_int_p()
    tr, vm, te = C.POINTER(C.c_uint)(), C.POINTER(C.c_uint)(), C.POINTER(C.c_uint)()
    tv = C.POINTER(C.c_longlong)()
    tval = L.c_dbl_p()
    nrw, nwd = C.c_longlong(), C.c_longlong()
    stats = (C.c_longlong * 4)()
    L.check(lib.crp_team2r_format_host(rp.size - 1, rp.ctypes.data_as(L.c_int_p), ci.ctypes.data_as(L.c_int_p), va.ctypes.data_as(L.c_dbl_p),
                                       int(G), C.byref(nteam), C.byref(lat), C.byref(tp), C.byref(ti), C.byref(tr), C.byref(nrw), C.byref(tv),
                                       C.byref(tval), C.byref(nwd), C.byref(tg), C.byref(ng), C.byref(vm), stats, C.byref(te)), "crp_team2r_format_host")
    nt = nteam.value

    def take(ptr, cnt, dt):
        out = np.ctypeslib.as_array(ptr, (max(cnt, 1),))[:cnt].astype(dt).copy()
        L.c_free(C.cast(ptr, C.c_void_p))
        return out
    return dict(G=int(G), rowdma=2, nteam=nt, lattice=bool(lat.value), tpanel=take(tp, 8 * nt, np.int32).reshape(nt, 8),
                tinfo=take(ti, 2 * nt, np.int32).reshape(nt, 2), trec=take(tr, nrw.value, np.uint32).reshape(-1, 8, 16),
                tvoff=take(tv, 8 * nt + 1, np.int64), tval=take(tval, nwd.value, np.float64),
                tgrid=take(tg, ng.value, np.int32).reshape(8, -1), vmap=take(vm, nnz, np.uint32),
                tent=take(te, 256 * ng.value, np.uint32).reshape(-1, 8, 32), rounds=int(stats[0]), steps=int(stats[1]), slots_filled=int(stats[2]), nnz=int(stats[3]))


def locality_order_host(rowptr, colidx, ncol=None, nparts=8):
    """crp_locality_order_host -> (perm, info dict or None when the matrix does not qualify)."""
    lib = L.load()
    rp = np.ascontiguousarray(rowptr, dtype=np.int32)
    ci = np.ascontiguousarray(colidx, dtype=np.int32)
    if ci.size == 0:
        ci = np.zeros(1, np.int32)
    m = rp.size - 1
    perm = np.zeros(max(m, 1), dtype=np.int32)
    info = np.zeros(4)
    rc = lib.crp_locality_order_host(m, m if ncol is None else int(ncol), rp.ctypes.data_as(L.c_int_p), ci.ctypes.data_as(L.c_int_p),
                                     int(nparts), perm.ctypes.data_as(L.c_int_p), info.ctypes.data_as(L.c_dbl_p))
    if rc < 0:
        raise RuntimeError("crp_locality_order_host failed: %d" % rc)
    if rc == 1:
        return perm[:m], None
    return perm[:m], dict(groups=int(info[0]), parts=int(info[1]), mean_dist_before=info[2], mean_dist_after=info[3])


SHAPES = ("aligned", "ld+1", "b1", "misaligned")      # operand shapes of crp_spmm_plan_host


def spmm_plan_host(rowptr, colidx, widths, variant=0, dtype="f64", shape="aligned", ncol=None):
    """crp_spmm_plan_host -> (info dict, resolved variants as a list, one per width): the kernel choice of the device path, on the host."""
    lib = L.load()
    rp = np.ascontiguousarray(rowptr, dtype=np.int32)
    ci = np.ascontiguousarray(colidx, dtype=np.int32)
    if ci.size == 0:
        ci = np.zeros(1, np.int32)
    m = rp.size - 1
    w = np.ascontiguousarray(widths, dtype=np.int32)
    res = np.zeros(max(w.size, 1), dtype=np.int32)
    info = np.zeros(5, dtype=np.int32)
    L.check(lib.crp_spmm_plan_host(m, m if ncol is None else int(ncol), rp.ctypes.data_as(L.c_int_p), ci.ctypes.data_as(L.c_int_p),
                                   w.size, w.ctypes.data_as(L.c_int_p), int(variant), int(dtype == "f32"), SHAPES.index(shape),
                                   res.ctypes.data_as(L.c_int_p), info.ctypes.data_as(L.c_int_p)), "crp_spmm_plan_host")
    return (dict(auto_variant=int(info[0]), reordered=int(info[1]), team2_min_n=int(info[2]), team2_pays=int(info[3]),
                 panels_sparse=int(info[4])), [int(x) for x in res[:w.size]])


def spmm_csr_f32(A, B0, C_out, n=None, B1=None, variant=0, stream=None):
    """crp_spmm_csr_f32: C := A * B with values, B and C in fp32 (row-major float32 torch tensors on the device).
    B0 = None: every column index is a receive-buffer one (B1 rows only)."""
    lib = L.load()
    if n is None:
        n = C_out.shape[1]
    b0p, ldb0 = (B0.data_ptr(), B0.stride(0)) if B0 is not None else (None, 0)
    b1p, ldb1 = (B1.data_ptr(), B1.stride(0)) if B1 is not None else (None, 0)
    L.check(lib.crp_spmm_csr_f32(A.handle, n, b0p, ldb0, b1p, ldb1, C_out.data_ptr(), C_out.stride(0), variant,
                                 _stream(C_out) if stream is None else stream), "crp_spmm_csr_f32")
