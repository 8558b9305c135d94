"""CPU: the row softmax over A's pattern, without a device.  The fourteen entry points exist with the documented prototypes,
are bound in _lib.SIGNATURES with matching ctypes and are exported; NULL engines are no-ops and read "not built"; the raw
entry points refuse a negative row count and NULL pointers before anything touches a device and accept nrow == 0; and on
plan-only 1 x 1 engines the Python wrappers refuse host values, wrong dtypes, mixed dtypes, wrong lengths, dimensions and
strides before any library call (a plan-only engine would abort in the library)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

_RAW = "int crp_row_softmax_%s(int nrow, const int *rowptr, const %s *s, %s *y, void *stream);"
_RAW_B = "int crp_row_softmax_bwd_%s(int nrow, const int *rowptr, const %s *y, const %s *dy, %s *ds, void *stream);"
_HND = "int crp_csr_dev_row_softmax_%s(crp_csr_dev_p A, const %s *s, %s *y, void *stream);"
_HND_B = "int crp_csr_dev_row_softmax_bwd_%s(crp_csr_dev_p A, const %s *y, const %s *dy, %s *ds, void *stream);"
SYMBOLS = {}
for _sfx, _t in (("f64", "double"), ("f32", "float")):
    SYMBOLS["crp_row_softmax_" + _sfx] = ("crpspmm_hip.h", _RAW % (_sfx, _t, _t))
    SYMBOLS["crp_row_softmax_bwd_" + _sfx] = ("crpspmm_hip.h", _RAW_B % (_sfx, _t, _t, _t))
    SYMBOLS["crp_csr_dev_row_softmax_" + _sfx] = ("crpspmm_hip.h", _HND % (_sfx, _t, _t))
    SYMBOLS["crp_csr_dev_row_softmax_bwd_" + _sfx] = ("crpspmm_hip.h", _HND_B % (_sfx, _t, _t, _t))
for _eng in ("rp", "para2d"):
    _p = "crp_%s_spmm" % _eng
    SYMBOLS[_p + "_row_softmax_ex"] = ("crp_engine.h", "void %s_row_softmax_ex(%s_p e, const void *s, void *y, int f32, void *stream);" % (_p, _p))
    SYMBOLS[_p + "_row_softmax_bwd_ex"] = ("crp_engine.h", "void %s_row_softmax_bwd_ex(%s_p e, const void *y, const void *dy, void *ds, int f32, "
                                                           "void *stream);" % (_p, _p))
    SYMBOLS[_p + "_row_softmax_built"] = ("crp_engine.h", "int %s_row_softmax_built(%s_p e);" % (_p, _p))


def _ctype_of(arg):
    arg = arg.strip()
    if "*" in arg or arg.split()[0].endswith("_p"):
        return C.c_void_p
    return {"int": C.c_int, "long long": C.c_longlong}[" ".join(arg.split()[:-1])]


@pytest.mark.parametrize("name", sorted(SYMBOLS))
def test_symbol_is_exported_declared_and_bound(crp, name):
    from crp_spmm_amd import _lib
    assert len(SYMBOLS) == 14
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


def test_null_engine_is_a_no_op_and_reads_not_built(crp):
    lib = crp.load()
    for f32 in (0, 1):
        lib.crp_rp_spmm_row_softmax_ex(None, None, None, f32, None)
        lib.crp_rp_spmm_row_softmax_bwd_ex(None, None, None, None, f32, None)
        lib.crp_para2d_spmm_row_softmax_ex(None, None, None, f32, None)
        lib.crp_para2d_spmm_row_softmax_bwd_ex(None, None, None, None, f32, None)
    assert lib.crp_rp_spmm_row_softmax_built(None) == 0
    assert lib.crp_para2d_spmm_row_softmax_built(None) == 0


def test_raw_entry_points_refuse_bad_arguments_without_a_device(crp):
    """The argument checks come before anything touches a device: the pointers below are never dereferenced."""
    lib = crp.load()
    buf = (C.c_double * 8)()
    p = C.addressof(buf)
    for fn in (lib.crp_row_softmax_f64, lib.crp_row_softmax_f32):
        assert fn(-1, p, p, p, None) == -1
        for hole in range(3):
            a = [p] * 3
            a[hole] = None
            assert fn(2, a[0], a[1], a[2], None) == -1, hole
        assert fn(0, None, None, None, None) == 0          # nothing to do: nothing is launched
        assert fn(0, p, p, p, None) == 0
    for fn in (lib.crp_row_softmax_bwd_f64, lib.crp_row_softmax_bwd_f32):
        assert fn(-1, p, p, p, p, None) == -1
        for hole in range(4):
            a = [p] * 4
            a[hole] = None
            assert fn(2, a[0], a[1], a[2], a[3], None) == -1, hole
        assert fn(0, None, None, None, None, None) == 0
    assert lib.crp_csr_dev_row_softmax_f64(None, p, p, None) == -1
    assert lib.crp_csr_dev_row_softmax_f32(None, p, p, None) == -1
    assert lib.crp_csr_dev_row_softmax_bwd_f64(None, p, p, p, None) == -1
    assert lib.crp_csr_dev_row_softmax_bwd_f32(None, p, p, p, None) == -1
    assert bytes(buf) == bytes(64)


NEW_CALLS = tuple(n for n in SYMBOLS)


class _Spy:
    """Stands in for the library on one object: records every entry point of the operations under test fetched for a call
    (as tests/test_f32_backward_args.py does)."""

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


def _calls(bad, good):
    """every way of putting the bad argument into a forward or a backward call, the other arguments being good ones"""
    return [lambda e, nnz: e.row_softmax(bad(nnz)),
            lambda e, nnz: e.row_softmax(good(nnz), out=bad(nnz)),
            lambda e, nnz: e.row_softmax_bwd(bad(nnz), good(nnz)),
            lambda e, nnz: e.row_softmax_bwd(good(nnz), bad(nnz)),
            lambda e, nnz: e.row_softmax_bwd(good(nnz), good(nnz), out=bad(nnz))]


def test_wrappers_refuse_what_is_not_a_float_tensor(crp, monkeypatch):
    """TypeError before any library call: numpy arrays, lists, other dtypes.  (A well-formed host tensor, which is refused for
    being on the host, stands in for the device tensor no CPU test can make: the bad argument is always met first or alone.)"""
    import torch
    good = lambda nnz: torch.ones(nnz, dtype=torch.float64)
    for bad in (lambda nnz: np.ones(nnz, np.float64), lambda nnz: np.ones(nnz, np.float32), lambda nnz: [0.0] * nnz,
                lambda nnz: torch.ones(nnz, dtype=torch.float16), lambda nnz: torch.ones(nnz, dtype=torch.int32)):
        for call in _calls(bad, good):
            _refused(crp, monkeypatch, TypeError, call)


def test_wrappers_refuse_host_tensors_and_mixed_dtypes(crp, monkeypatch):
    import torch
    for tdt in (torch.float64, torch.float32):
        _refused(crp, monkeypatch, TypeError, lambda e, nnz: e.row_softmax(torch.ones(nnz, dtype=tdt)))
        _refused(crp, monkeypatch, TypeError, lambda e, nnz: e.row_softmax_bwd(torch.ones(nnz, dtype=tdt), torch.ones(nnz, dtype=tdt)))
    a, b = torch.float64, torch.float32
    _refused(crp, monkeypatch, TypeError, lambda e, nnz: e.row_softmax(torch.ones(nnz, dtype=a), out=torch.ones(nnz, dtype=b)))
    _refused(crp, monkeypatch, TypeError, lambda e, nnz: e.row_softmax_bwd(torch.ones(nnz, dtype=a), torch.ones(nnz, dtype=b)))
    _refused(crp, monkeypatch, TypeError, lambda e, nnz: e.row_softmax_bwd(torch.ones(nnz, dtype=b), torch.ones(nnz, dtype=b),
                                                                              out=torch.ones(nnz, dtype=a)))


def test_wrappers_refuse_wrong_lengths_dimensions_and_strides(crp, monkeypatch):
    import torch
    good = lambda nnz: torch.ones(nnz, dtype=torch.float32)
    bads = [lambda nnz: torch.ones(nnz - 1, dtype=torch.float32), lambda nnz: torch.ones(nnz + 1, dtype=torch.float32),
            lambda nnz: torch.ones(0, dtype=torch.float32), lambda nnz: torch.ones(2 * nnz, dtype=torch.float32)[::2],
            lambda nnz: torch.ones((nnz, 1), dtype=torch.float32), lambda nnz: torch.ones((1, nnz), dtype=torch.float32)]
    for bad in bads:
        for call in _calls(bad, good):         # (shapes are checked before the tensors' device: the host stand-ins pass that far)
            _refused(crp, monkeypatch, ValueError, call)


def test_device_level_wrappers_refuse_before_any_library_call(crp, monkeypatch):
    """hip.row_softmax / _bwd: the same rules, and an int32 device row pointer"""
    import torch
    from crp_spmm_amd import _lib, hip
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was reached"))
    rp = torch.zeros(5, dtype=torch.int32)
    v = torch.ones(7, dtype=torch.float64)
    with pytest.raises(TypeError):
        hip.row_softmax(rp, np.ones(7))
    with pytest.raises(TypeError):
        hip.row_softmax(rp, v)                                   # on the host
    with pytest.raises(TypeError):
        hip.row_softmax_bwd(rp, v, v.float())
    with pytest.raises(ValueError):
        hip.row_softmax(rp, v.reshape(7, 1))
    with pytest.raises(ValueError):
        hip.row_softmax(rp, v, out=torch.ones(8, dtype=torch.float64))
    with pytest.raises(ValueError):
        hip.row_softmax_bwd(rp, v, torch.ones(6, dtype=torch.float64))
    with pytest.raises(ValueError):
        hip.row_softmax_bwd(rp, torch.ones(14, dtype=torch.float64)[::2], v)


def test_built_reads_false_on_plan_only_engines(crp):
    e1, e2, sc, nnz = _engines(crp)
    assert e1.row_softmax_built is False and e2.row_softmax_built is False and e2.rp.row_softmax_built is False
    e1.free()
    e2.free()
    sc.free()
