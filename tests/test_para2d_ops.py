"""CPU: value updates, A^T*B and SDDMM on the 2D engine, without a device.  The nine entry points exist with the documented
prototypes; the Python wrappers refuse mixed dtypes, float32 to exec_t, wrong shapes, a wrong `out` length, a wrong mode and
a wrong-length value update before any of the new library calls (a plan-only engine would abort in the library, a wrong
shape would be an out-of-bounds device access); update_values on a plan-only 1 x 1 engine replaces the inner plan's values;
and at 2 and 4 ranks (tests/dist_para2d_ops_worker.py) the slice counts, the value update in panel order and the numpy
replay of the SDDMM data flow hold on every grid, a grid row with an empty A0 slice included."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

SYMBOLS = {
    # name -> (header, the prototype as documented)
    "crp_sum_segments_f64": ("crpspmm_hip.h",
                             "int crp_sum_segments_f64(int nseg, long long len, const double *src, long long seg_stride, double *out, "
                             "void *stream);"),
    "crp_sum_segments_f32": ("crpspmm_hip.h",
                             "int crp_sum_segments_f32(int nseg, long long len, const float *src, long long seg_stride, float *out, "
                             "void *stream);"),
    "crp_para2d_spmm_update_values": ("crp_engine.h", "void crp_para2d_spmm_update_values(crp_para2d_spmm_p e, const double *A_val);"),
    "crp_para2d_spmm_exec_t_ex": ("crp_engine.h",
                                  "void crp_para2d_spmm_exec_t_ex(crp_para2d_spmm_p e, int BC_layout, const double *B, long long ldB, "
                                  "double *C, long long ldC, void *stream);"),
    "crp_para2d_spmm_sddmm_ex": ("crp_engine.h",
                                 "void crp_para2d_spmm_sddmm_ex(crp_para2d_spmm_p e, int layout, const double *X, long long ldX, "
                                 "const double *Y, long long ldY, double *out, int mode, void *stream);"),
    "crp_para2d_spmm_sddmm_f32_ex": ("crp_engine.h",
                                     "void crp_para2d_spmm_sddmm_f32_ex(crp_para2d_spmm_p e, int layout, const float *X, long long ldX, "
                                     "const float *Y, long long ldY, float *out, int mode, void *stream);"),
    "crp_para2d_spmm_sddmm_built": ("crp_engine.h", "int crp_para2d_spmm_sddmm_built(crp_para2d_spmm_p e);"),
    "crp_para2d_spmm_slice_nnz": ("crp_engine.h", "long long crp_para2d_spmm_slice_nnz(crp_para2d_spmm_p e);"),
    "crp_para2d_spmm_row_slice_nnz": ("crp_engine.h", "int crp_para2d_spmm_row_slice_nnz(crp_para2d_spmm_p e, long long *nnz_of_pj);"),
}
# the pointer arguments _lib binds with a type of their own (everything else that is a pointer or a handle: void *)
TYPED = {("crp_para2d_spmm_update_values", 1): C.POINTER(C.c_double), ("crp_para2d_spmm_row_slice_nnz", 1): C.POINTER(C.c_longlong)}


def _ctype_of(name, i, arg):
    arg = arg.strip()
    if (name, i) in TYPED:
        return TYPED[(name, i)]
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
    res, args = _lib.SIGNATURES[name]
    want = [_ctype_of(name, i, a) for i, a in enumerate(proto[proto.index("(") + 1:proto.rindex(")")].split(","))]
    want_res = {"int": C.c_int, "long long": C.c_longlong, "void": None}[proto[:proto.index(" crp_")]]
    assert res == want_res, name
    assert list(args) == want, (name, args, want)
    fn = getattr(crp.load(), name)
    assert fn.restype == res and list(fn.argtypes) == want


NEW_CALLS = ("crp_para2d_spmm_update_values", "crp_para2d_spmm_exec_t_ex", "crp_para2d_spmm_sddmm_ex", "crp_para2d_spmm_sddmm_f32_ex",
             "crp_rp_spmm_update_values", "crp_rp_spmm_exec_t_ex", "crp_rp_spmm_sddmm_ex", "crp_rp_spmm_sddmm_f32_ex")


class _Spy:
    """Stands in for the library on one object: records every entry point of the new operations fetched for a call."""

    def __init__(self, lib, called):
        self._lib, self._called = lib, called

    def __getattr__(self, name):
        if name in NEW_CALLS:
            self._called.append(name)
        return getattr(self._lib, name)


M, K, N = 40, 40, 8


def _plan_only(crp):
    from crp_spmm_amd import comm, engine, gen
    rp, ci, va = gen.random_csr(M, K, 6, seed=3)
    sc = comm.SelfComm()
    e2 = engine.Para2dSpmm(sc, 1, 1, [0, M], [0, K], [0, M], [0, N], rp, ci, va, plan_only=True)
    return e2, sc, int(rp[-1]), va


def _refused(crp, monkeypatch, exc, call):
    e2, sc, nnz, _va = _plan_only(crp)
    called = []
    monkeypatch.setattr(e2, "_lib", _Spy(e2._lib, called))
    monkeypatch.setattr(e2.rp, "_lib", _Spy(e2.rp._lib, called))
    with pytest.raises(exc):
        call(e2, nnz)
    assert called == []
    monkeypatch.undo()
    e2.free()
    sc.free()


def test_properties_of_a_one_by_one_engine(crp):
    e2, sc, nnz, _va = _plan_only(crp)
    assert e2.slice_nnz == nnz and e2.loc_B_nrow == K
    row = e2.row_slice_nnz
    assert row.dtype == np.int64 and row.tolist() == [nnz]
    assert e2.sddmm_built is False
    e2.free()
    sc.free()


@pytest.mark.parametrize("x, y, o", [("f8", "f4", "f8"), ("f4", "f8", "f4"), ("f8", "f8", "f4"), ("f4", "f4", "f8"),
                                     ("f2", "f2", "f2"), ("i4", "i4", "i4")])
@pytest.mark.parametrize("layout", [0, 1])
def test_sddmm_refuses_mixed_or_unsupported_dtypes(crp, monkeypatch, x, y, o, layout):
    shape = (M, N) if layout == 0 else (N, M)
    _refused(crp, monkeypatch, TypeError,
             lambda e, nnz: e.sddmm(layout, np.zeros(shape, x), np.zeros(shape, y), np.zeros(nnz, o)))


@pytest.mark.parametrize("layout", [0, 1])
def test_exec_t_refuses_float32_and_mixed_dtypes(crp, monkeypatch, layout):
    shape = (M, N) if layout == 0 else (N, M)
    for b, c in (("f4", "f4"), ("f8", "f4"), ("f4", "f8"), ("i4", "i4")):
        _refused(crp, monkeypatch, TypeError, lambda e, nnz: e.exec_t(layout, np.zeros(shape, b), np.zeros(shape, c)))


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_sddmm_refuses_wrong_shapes_out_length_and_mode(crp, monkeypatch, dt):
    bad = [
        lambda e, nnz: e.sddmm(0, np.zeros((M, N - 1), dt), np.zeros((K, N), dt), np.zeros(nnz, dt)),      # X a column short
        lambda e, nnz: e.sddmm(0, np.zeros((M - 1, N), dt), np.zeros((K, N), dt), np.zeros(nnz, dt)),      # X a row short
        lambda e, nnz: e.sddmm(0, np.zeros((M, N), dt), np.zeros((K - 1, N), dt), np.zeros(nnz, dt)),      # Y a row short
        lambda e, nnz: e.sddmm(0, np.zeros((M, N), dt), np.zeros((K, N + 1), dt), np.zeros(nnz, dt)),      # Y a column wide
        lambda e, nnz: e.sddmm(1, np.zeros((N, M - 1), dt), np.zeros((N, K), dt), np.zeros(nnz, dt)),      # column-major X a row short
        lambda e, nnz: e.sddmm(1, np.zeros((N, M), dt), np.zeros((N + 1, K), dt), np.zeros(nnz, dt)),      # column-major Y a column wide
        lambda e, nnz: e.sddmm(1, np.zeros((N, M), dt), np.zeros((N, K - 1), dt), np.zeros(nnz, dt)),      # column-major Y a row short
        lambda e, nnz: e.sddmm(0, np.zeros((M, N), dt), np.zeros((K, N), dt), np.zeros(nnz - 1, dt)),      # out short
        lambda e, nnz: e.sddmm(0, np.zeros((M, N), dt), np.zeros((K, N), dt), np.zeros(nnz + 1, dt)),      # out long
        lambda e, nnz: e.sddmm(0, np.zeros((M, N), dt), np.zeros((K, N), dt), np.zeros(2 * nnz, dt)[::2]),  # out strided
        lambda e, nnz: e.sddmm(0, np.zeros((M, N), dt), np.zeros((K, N), dt), np.zeros(nnz, dt), mode=2),
    ]
    for call in bad:
        _refused(crp, monkeypatch, ValueError, call)


def test_exec_t_refuses_wrong_shapes(crp, monkeypatch):
    z = np.zeros
    bad = [
        lambda e, nnz: e.exec_t(0, z((M - 1, N)), z((K, N))),        # B a row short
        lambda e, nnz: e.exec_t(0, z((M, N + 1)), z((K, N))),        # B a column wide
        lambda e, nnz: e.exec_t(0, z((M, N)), z((K - 1, N))),        # C a row short
        lambda e, nnz: e.exec_t(0, z((M, N)), z((K, N - 1))),        # C a column short
        lambda e, nnz: e.exec_t(1, z((N, M - 1)), z((N, K))),        # column-major B a row short
        lambda e, nnz: e.exec_t(1, z((N + 1, M)), z((N, K))),
        lambda e, nnz: e.exec_t(1, z((N, M)), z((N, K - 1))),        # column-major C a row short
        lambda e, nnz: e.exec_t(1, z((N, M)), z((N - 1, K))),
    ]
    for call in bad:
        _refused(crp, monkeypatch, ValueError, call)


def test_update_values_refuses_a_wrong_length(crp, monkeypatch):
    for d in (-1, 1):
        _refused(crp, monkeypatch, ValueError, lambda e, nnz: e.update_values(np.ones(nnz + d)))
    _refused(crp, monkeypatch, ValueError, lambda e, nnz: e.update_values(np.ones(0)))


def test_update_values_replaces_the_plan_values(crp):
    e2, sc, nnz, va = _plan_only(crp)
    assert np.array_equal(e2.rp.plan()["A_val"], va)
    new = 3.0 * va + 1.0
    e2.update_values(new)
    assert np.array_equal(e2.rp.plan()["A_val"], new)
    assert not e2.sddmm_built
    e2.free()
    sc.free()


def test_null_engine_is_a_no_op(crp):
    lib = crp.load()
    lib.crp_para2d_spmm_update_values(None, None)
    lib.crp_para2d_spmm_exec_t_ex(None, 0, None, 0, None, 0, None)
    lib.crp_para2d_spmm_sddmm_ex(None, 0, None, 0, None, 0, None, 0, None)
    lib.crp_para2d_spmm_sddmm_f32_ex(None, 0, None, 0, None, 0, None, 0, None)
    assert lib.crp_para2d_spmm_sddmm_built(None) == 0
    assert lib.crp_para2d_spmm_slice_nnz(None) == -1
    assert lib.crp_para2d_spmm_row_slice_nnz(None, None) == 0


def test_sum_segments_refuses_bad_arguments_without_a_device(crp):
    """The argument checks come before anything touches a device: the pointers below are never dereferenced."""
    lib = crp.load()
    buf = (C.c_double * 8)()
    p = C.addressof(buf)
    for fn in (lib.crp_sum_segments_f64, lib.crp_sum_segments_f32):
        assert fn(2, 4, None, 4, p, None) == -1
        assert fn(2, 4, p, 4, None, None) == -1
        assert fn(0, 4, p, 4, p, None) == -1
        assert fn(2, -1, p, 4, p, None) == -1
        assert fn(2, 4, p, 3, p, None) == -4
        assert fn(2, 0, p, 0, p, None) == 0
        assert fn(1, 0, p, -5, p, None) == 0


@pytest.mark.parametrize("world", [2, 4])
def test_slices_update_and_sddmm_data_flow_on_every_grid(world):
    env = dict(os.environ)
    env.pop("RP_SPMM_REIDX", None)
    env["OMP_NUM_THREADS"] = "1"
    # the ranks neither see nor open a GPU, also on a machine that has one (tests/test_dist_cpu.py)
    env["HIP_VISIBLE_DEVICES"] = "-1"
    env["GPU_ENABLE_PAL"] = "1"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world),
           "--master-addr", "127.0.0.1", "--master-port", str(29660 + world), os.path.join(ROOT, "tests", "dist_para2d_ops_worker.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "DIST_PARA2D_OPS_WORKER_OK world=%d" % world in r.stdout
