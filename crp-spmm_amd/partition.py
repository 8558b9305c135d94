"""Graph-based 1D row partitioning and the symmetric permutation P A P^T -- Python view of include/crp_part.h.

``graph_row_order`` is part-method 1 of the example programs without METIS: recursive breadth-first bisection of
the graph of A + A^T (row groups as vertices, row nonzeros as weights); ``permute_sym`` applies the partition's
permutation on the host (numpy arrays) or on the device (torch tensors on the GPU, HIP kernels in
csrc/permute_kernels.hip); ``graph_row_partition`` does both in place, like the reference's METIS_row_partition."""
import ctypes as C

import numpy as np

from . import _lib as L

# rows up to this many entries are sorted in LDS by one workgroup; longer rows go through a device scratch buffer
# (LDS_PAIRS in csrc/permute_kernels.hip); rows up to 64 entries are sorted by one wave in registers
PERMUTE_WAVE_PAIRS = 64
PERMUTE_LDS_PAIRS = 4096

# negative return codes (include/crp_part.h)
EARG, EPERM, ECOL, EPTR, EMIXED = -1, -2, -3, -4, -5
_ERRORS = {EARG: "bad argument", EPERM: "perm is not a bijection", ECOL: "column index out of range",
           EPTR: "rowptr does not start at 0 or decreases", EMIXED: "host and device pointers mixed"}


class PartitionError(ValueError):
    """A bad input (negative code of include/crp_part.h); ``code`` holds the code."""

    def __init__(self, what, code):
        super().__init__("%s: %s (code %d)" % (what, _ERRORS.get(code, "error"), code))
        self.code = code


def _check(rc, what):
    if rc < 0:
        raise PartitionError(what, rc)
    L.check(rc, what)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _ip(a):
    return a.ctypes.data_as(L.c_int_p)


def graph_row_order(rowptr, colidx, nproc):
    """-> (perm, row_displs): perm[i] = new index of original row i, row_displs = nproc + 1 cuts of the new rows."""
    rowptr, colidx = _i32(rowptr), _i32(colidx)
    nrow = rowptr.size - 1
    if nrow < 0 or nproc < 1 or rowptr[-1] != colidx.size:
        raise PartitionError("graph_row_order", EARG)
    perm = np.zeros(max(nrow, 1), np.int32)
    displs = np.zeros(nproc + 1, np.int32)
    _check(L.load().crp_graph_row_order(nrow, nproc, _ip(rowptr), _ip(colidx if colidx.size else np.zeros(1, np.int32)),
                                        _ip(perm), _ip(displs)), "crp_graph_row_order")
    return perm[:nrow], displs


def permute_sym(rowptr, colidx, val, perm, stream=None):
    """P A P^T -> (rowptr1, colidx1, val1).  numpy arrays: host threads; torch tensors on the GPU (int32 rowptr /
    colidx / perm, float64 val): the HIP kernels on `stream` (default: the current torch stream), results as tensors
    on the same device."""
    lib = L.load()
    try:
        import torch
        on_dev = isinstance(rowptr, torch.Tensor) and rowptr.is_cuda
    except ImportError:
        on_dev = False
    if on_dev:
        import torch
        for t, dt in ((rowptr, torch.int32), (colidx, torch.int32), (val, torch.float64), (perm, torch.int32)):
            if not isinstance(t, torch.Tensor) or t.dtype != dt or not t.is_contiguous() or not t.is_cuda:
                raise PartitionError("permute_sym", EMIXED if not (isinstance(t, torch.Tensor) and t.is_cuda) else EARG)
        nrow = rowptr.numel() - 1
        if nrow < 0 or perm.numel() != nrow or int(rowptr[-1]) != colidx.numel() or val.numel() != colidx.numel():
            raise PartitionError("permute_sym", EARG)
        dev = rowptr.device
        rowptr1 = torch.empty(nrow + 1, dtype=torch.int32, device=dev)
        colidx1 = torch.empty(max(colidx.numel(), 1), dtype=torch.int32, device=dev)
        val1 = torch.empty(max(val.numel(), 1), dtype=torch.float64, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
        _check(lib.crp_csr_permute_sym(nrow, C.c_void_p(rowptr.data_ptr()), C.c_void_p(colidx.data_ptr() or None),
                                       C.c_void_p(val.data_ptr() or None), C.c_void_p(perm.data_ptr()),
                                       C.c_void_p(rowptr1.data_ptr()), C.c_void_p(colidx1.data_ptr()),
                                       C.c_void_p(val1.data_ptr()), C.c_void_p(st)), "crp_csr_permute_sym")
        nnz = colidx.numel()
        return rowptr1, colidx1[:nnz], val1[:nnz]
    rowptr, colidx, perm = _i32(rowptr), _i32(colidx), _i32(perm)
    val = np.ascontiguousarray(val, dtype=np.float64)
    nrow = rowptr.size - 1
    nnz = colidx.size
    if nrow < 0 or perm.size != nrow or rowptr[-1] != nnz or val.size != nnz:
        raise PartitionError("permute_sym", EARG)
    rowptr1 = np.zeros(nrow + 1, np.int32)
    colidx1 = np.zeros(max(nnz, 1), np.int32)
    val1 = np.zeros(max(nnz, 1), np.float64)
    ci = colidx if nnz else np.zeros(1, np.int32)
    va = val if nnz else np.zeros(1, np.float64)
    pm = perm if perm.size else np.zeros(1, np.int32)
    _check(lib.crp_csr_permute_sym(nrow, rowptr.ctypes.data, ci.ctypes.data, va.ctypes.data, pm.ctypes.data,
                                   rowptr1.ctypes.data, colidx1.ctypes.data, val1.ctypes.data, None), "crp_csr_permute_sym")
    return rowptr1, colidx1[:nnz], val1[:nnz]


def graph_row_partition(rowptr, colidx, val, nproc, where=-1):
    """crp_graph_row_partition on copies of the host arrays -> (rowptr1, colidx1, val1, perm, row_displs).
    where = 0: host, 1: device (staged through the current HIP device), -1: the device when there is one."""
    rowptr, colidx = _i32(rowptr).copy(), _i32(colidx).copy()
    val = np.ascontiguousarray(val, dtype=np.float64).copy()
    nrow = rowptr.size - 1
    if nrow < 0 or nproc < 1 or rowptr[-1] != colidx.size or val.size != colidx.size:
        raise PartitionError("graph_row_partition", EARG)
    perm = np.zeros(max(nrow, 1), np.int32)
    displs = np.zeros(nproc + 1, np.int32)
    ci = colidx if colidx.size else np.zeros(1, np.int32)
    va = val if val.size else np.zeros(1, np.float64)
    _check(L.load().crp_graph_row_partition(nrow, nproc, _ip(rowptr), _ip(ci), va.ctypes.data_as(L.c_dbl_p), _ip(perm),
                                            _ip(displs), where), "crp_graph_row_partition")
    return rowptr, colidx, val, perm[:nrow], displs
