"""CPU: the fp32 transposed product and the device-resident value updates, without a device.  The new entry points exist with
the documented prototypes, are bound in _lib.SIGNATURES with matching ctypes and are exported; NULL engines are no-ops; the
kernel entry points refuse NULL and negative arguments before anything touches a device; and on plan-only 1 x 1 engines the
Python wrappers refuse wrong dtypes, wrong shapes, host values and a wrong length before any library call (a plan-only
engine would abort in the library, a wrong shape would be an out-of-bounds device access).  exec_t still refuses float32."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

SYMBOLS = {
    # name -> (header, the prototype as documented)
    "crp_scatter_add_rows_f32": ("crpspmm_hip.h",
                                 "int crp_scatter_add_rows_f32(int nseg, int n, const int *seg_row, const int *seg_ptr, const int *seg_pos, "
                                 "const float *src, long long lds, float *dst, long long ldd, void *stream);"),
    "crp_gather_vals_f64": ("crpspmm_hip.h",
                            "int crp_gather_vals_f64(long long n, const int *map, const double *src, double *dst, void *stream);"),
    "crp_gather_vals_f32_f64": ("crpspmm_hip.h",
                                "int crp_gather_vals_f32_f64(long long n, const int *map, const float *src, double *dst, void *stream);"),
    "crp_rp_spmm_exec_t_f32_ex": ("crp_engine.h",
                                  "void crp_rp_spmm_exec_t_f32_ex(crp_rp_spmm_p rp_spmm, int BC_layout, const float *B, long long ldB, "
                                  "float *C, long long ldC, void *stream);"),
    "crp_rp_spmm_update_values_dev": ("crp_engine.h",
                                      "void crp_rp_spmm_update_values_dev(crp_rp_spmm_p rp_spmm, const void *A_val_dev, int f32, void *stream);"),
    "crp_rp_spmm_host_values_stale": ("crp_engine.h", "int crp_rp_spmm_host_values_stale(crp_rp_spmm_p rp_spmm);"),
    "crp_para2d_spmm_exec_t_f32_ex": ("crp_engine.h",
                                      "void crp_para2d_spmm_exec_t_f32_ex(crp_para2d_spmm_p e, int BC_layout, const float *B, long long ldB, "
                                      "float *C, long long ldC, void *stream);"),
    "crp_para2d_spmm_update_values_dev": ("crp_engine.h",
                                          "void crp_para2d_spmm_update_values_dev(crp_para2d_spmm_p e, const void *A_val_dev, int f32, "
                                          "void *stream);"),
}


def _ctype_of(arg):
    arg = arg.strip()
    if "*" in arg or arg.split()[0].endswith("_p"):
        return C.c_void_p
    return {"int": C.c_int, "long long": C.c_longlong}[" ".join(arg.split()[:-1])]


@pytest.mark.parametrize("name", sorted(SYMBOLS))
def test_symbol_is_exported_declared_and_bound(crp, name):
    from crp_spmm_amd import _lib
    header, proto = SYMBOLS[name]
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert any(ln.split()[-1] == name and " T " in ln for ln in out.splitlines()), "%s is not exported" % name
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", header)).read())
    assert proto in text, "%s is not declared in include/%s as documented" % (name, header)
    assert name in _lib.SIGNATURES, "%s is not bound in _lib.SIGNATURES" % name
    res, args = _lib.SIGNATURES[name]
    want = [_ctype_of(a) for a in proto[proto.index("(") + 1:proto.rindex(")")].split(",")]
    want_res = {"int": C.c_int, "void": None}[proto[:proto.index(" crp_")]]
    assert res == want_res, name
    assert list(args) == want, (name, args, want)
    fn = getattr(crp.load(), name)
    assert fn.restype == res and list(fn.argtypes) == want


def test_null_engine_is_a_no_op(crp):
    lib = crp.load()
    lib.crp_rp_spmm_exec_t_f32_ex(None, 0, None, 0, None, 0, None)
    lib.crp_para2d_spmm_exec_t_f32_ex(None, 0, None, 0, None, 0, None)
    for f32 in (0, 1):
        lib.crp_rp_spmm_update_values_dev(None, None, f32, None)
        lib.crp_para2d_spmm_update_values_dev(None, None, f32, None)
    assert lib.crp_rp_spmm_host_values_stale(None) == 0


def test_kernel_entry_points_refuse_bad_arguments_without_a_device(crp):
    """The argument checks come before anything touches a device: the pointers below are never dereferenced."""
    lib = crp.load()
    buf = (C.c_double * 8)()
    p = C.addressof(buf)
    fn = lib.crp_scatter_add_rows_f32
    assert fn(-1, 4, p, p, p, p, 4, p, 4, None) == -1
    assert fn(2, -1, p, p, p, p, 4, p, 4, None) == -1
    for hole in range(5):
        a = [p] * 5
        a[hole] = None
        assert fn(2, 4, a[0], a[1], a[2], a[3], 4, a[4], 4, None) == -1, hole
    assert fn(0, 4, None, None, None, None, 4, None, 4, None) == 0          # nothing to do: nothing is launched
    assert fn(2, 0, None, None, None, None, 0, None, 0, None) == 0
    for fn in (lib.crp_gather_vals_f64, lib.crp_gather_vals_f32_f64):
        assert fn(-1, None, p, p, None) == -1
        assert fn(4, None, None, p, None) == -1
        assert fn(4, p, p, None, None) == -1
        assert fn(0, None, None, None, None) == 0


NEW_CALLS = tuple(n for n in SYMBOLS if "spmm" in n) + ("crp_rp_spmm_exec_t_ex", "crp_para2d_spmm_exec_t_ex", "crp_rp_spmm_update_values",
                                                        "crp_para2d_spmm_update_values")


class _Spy:
    """Stands in for the library on one object: records every entry point of the operations under test fetched for a call
    (as tests/test_para2d_ops.py does)."""

    def __init__(self, lib, called):
        self._lib, self._called = lib, called

    def __getattr__(self, name):
        if name in NEW_CALLS:
            self._called.append(name)
        return getattr(self._lib, name)


M, K, N = 40, 36, 8


def _engines(crp):
    """plan-only engines of one rank: the 2D engine (with its inner row engine) and a row engine of its own"""
    from crp_spmm_amd import comm, engine, gen
    rp, ci, va = gen.random_csr(M, K, 6, seed=3)
    sc = comm.SelfComm()
    e2 = engine.Para2dSpmm(sc, 1, 1, [0, M], [0, K], [0, M], [0, N], rp, ci, va, plan_only=True)
    e1 = engine.RpSpmm(0, M, rp, ci, va, [0, K], N, sc, plan_only=True)
    return e1, e2, sc, int(rp[-1])


def _refused(crp, monkeypatch, exc, call):
    e1, e2, sc, nnz = _engines(crp)
    called = []
    for e in (e1, e2, e2.rp):
        monkeypatch.setattr(e, "_lib", _Spy(e._lib, called))
    for e in (e1, e2):
        with pytest.raises(exc):
            call(e, nnz)
    assert called == []
    monkeypatch.undo()
    e1.free()
    e2.free()
    sc.free()


@pytest.mark.parametrize("layout", [0, 1])
def test_exec_t_f32_refuses_every_dtype_but_float32(crp, monkeypatch, layout):
    import torch
    sb, sc_ = ((M, N), (K, N)) if layout == 0 else ((N, M), (N, K))
    for b, c in (("f8", "f8"), ("f8", "f4"), ("f4", "f8"), ("f2", "f2"), ("i4", "i4")):
        _refused(crp, monkeypatch, TypeError, lambda e, nnz: e.exec_t_f32(layout, np.zeros(sb, b), np.zeros(sc_, c)))
    for b, c in ((torch.float64, torch.float64), (torch.float32, torch.float64), (torch.float16, torch.float16)):
        _refused(crp, monkeypatch, TypeError, lambda e, nnz: e.exec_t_f32(layout, torch.zeros(sb, dtype=b), torch.zeros(sc_, dtype=c)))


def test_exec_t_f32_refuses_wrong_shapes(crp, monkeypatch):
    z = lambda shape: np.zeros(shape, np.float32)
    bad = [
        lambda e, nnz: e.exec_t_f32(0, z((M - 1, N)), z((K, N))),        # B a row short
        lambda e, nnz: e.exec_t_f32(0, z((M, N + 1)), z((K, N))),        # B a column wide
        lambda e, nnz: e.exec_t_f32(0, z((M, N)), z((K - 1, N))),        # C a row short
        lambda e, nnz: e.exec_t_f32(0, z((M, N)), z((K, N - 1))),        # C a column short
        lambda e, nnz: e.exec_t_f32(0, z((K, N)), z((M, N))[:K]),        # B and C swapped (B has K < M rows)
        lambda e, nnz: e.exec_t_f32(1, z((N, M - 1)), z((N, K))),        # column-major B a row short
        lambda e, nnz: e.exec_t_f32(1, z((N + 1, M)), z((N, K))),
        lambda e, nnz: e.exec_t_f32(1, z((N, M)), z((N, K - 1))),        # column-major C a row short
        lambda e, nnz: e.exec_t_f32(1, z((N, M)), z((N - 1, K))),
    ]
    for call in bad:
        _refused(crp, monkeypatch, ValueError, call)


def test_update_values_dev_refuses_host_values_and_wrong_lengths(crp, monkeypatch):
    import torch
    for dt, tdt in ((np.float64, torch.float64), (np.float32, torch.float32)):
        _refused(crp, monkeypatch, TypeError, lambda e, nnz: e.update_values_dev(np.ones(nnz, dt)))                   # numpy
        _refused(crp, monkeypatch, TypeError, lambda e, nnz: e.update_values_dev(torch.ones(nnz, dtype=tdt)))         # a CPU tensor
    _refused(crp, monkeypatch, TypeError, lambda e, nnz: e.update_values_dev(list(range(nnz))))
    _refused(crp, monkeypatch, TypeError, lambda e, nnz: e.update_values_dev(torch.ones(nnz, dtype=torch.float16)))
    _refused(crp, monkeypatch, TypeError, lambda e, nnz: e.update_values_dev(torch.ones(nnz, dtype=torch.int32)))
    for d in (-1, 1):
        _refused(crp, monkeypatch, ValueError, lambda e, nnz: e.update_values_dev(torch.ones(nnz + d, dtype=torch.float64)))
    _refused(crp, monkeypatch, ValueError, lambda e, nnz: e.update_values_dev(torch.ones(0, dtype=torch.float32)))
    _refused(crp, monkeypatch, ValueError, lambda e, nnz: e.update_values_dev(torch.ones(2 * nnz, dtype=torch.float64)[::2]))   # strided
    _refused(crp, monkeypatch, ValueError, lambda e, nnz: e.update_values_dev(torch.ones((nnz, 1), dtype=torch.float64)))       # 2-D


@pytest.mark.parametrize("layout", [0, 1])
def test_exec_t_still_refuses_float32(crp, monkeypatch, layout):
    """The existing contract, restated next to the new methods: exec_t is fp64 only."""
    sb, sc_ = ((M, N), (K, N)) if layout == 0 else ((N, M), (N, K))
    for b, c in (("f4", "f4"), ("f8", "f4"), ("f4", "f8")):
        _refused(crp, monkeypatch, TypeError, lambda e, nnz: e.exec_t(layout, np.zeros(sb, b), np.zeros(sc_, c)))


def test_host_values_stale_is_false_on_a_fresh_engine_and_after_a_host_update(crp):
    e1, e2, sc, nnz = _engines(crp)
    assert e1.host_values_stale is False and e2.rp.host_values_stale is False
    e1.update_values(np.full(nnz, 2.0))
    assert e1.host_values_stale is False and np.array_equal(e1.plan()["A_val"], np.full(nnz, 2.0))
    e1.free()
    e2.free()
    sc.free()
