"""CPU: the fused attention over A's pattern, without a device.  The five entry points exist with the documented prototypes, are
bound in _lib.SIGNATURES with matching ctypes and are exported; a NULL engine is a no-op and reads "not built"; the device
entry points refuse every bad argument with the documented code before anything touches a device; and the Python wrappers
refuse mixed dtypes, wrong shapes and tensors that are not on the device before any library call."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

_DEV = ("int crp_attention_csr_%s(crp_csr_dev_p A, int nk, int nv, double scale, int bias, const %s *Q, long long ldQ, "
        "const %s *K0, long long ldK0, const %s *K1, long long ldK1, const %s *V0, long long ldV0, const %s *V1, long long ldV1, "
        "%s *O, long long ldO, %s *lse, %s *p_out, const int *out_pos, void *stream);")
_ENG = ("void crp_rp_spmm_attention%s_ex(crp_rp_spmm_p rp_spmm, int layout, double scale, int bias, const %s *Q, long long ldQ, "
        "const %s *K, long long ldK, const %s *V, long long ldV, %s *O, long long ldO, %s *lse, %s *p_out, void *stream);")
SYMBOLS = {
    "crp_attention_csr_f64": ("crpspmm_hip.h", _DEV % (("f64",) + ("double",) * 8)),
    "crp_attention_csr_f32": ("crpspmm_hip.h", _DEV % (("f32",) + ("float",) * 8)),
    "crp_rp_spmm_attention_ex": ("crp_engine.h", _ENG % (("",) + ("double",) * 6)),
    "crp_rp_spmm_attention_f32_ex": ("crp_engine.h", _ENG % (("_f32",) + ("float",) * 6)),
    "crp_rp_spmm_attention_built": ("crp_engine.h", "int crp_rp_spmm_attention_built(crp_rp_spmm_p rp_spmm);"),
}


def _ctype_of(arg):
    arg = arg.strip()
    if "*" in arg or arg.split()[0].endswith("_p"):
        return C.c_void_p
    return {"int": C.c_int, "long long": C.c_longlong, "double": C.c_double}[" ".join(arg.split()[:-1])]


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
    assert res == {"int": C.c_int, "void": None}[proto[:proto.index(" crp_")]], name
    assert list(args) == want, (name, args, want)
    fn = getattr(crp.load(), name)
    assert fn.restype == res and list(fn.argtypes) == want


def test_null_engine_is_a_no_op_and_reads_not_built(crp):
    lib = crp.load()
    buf = (C.c_double * 8)()
    p = C.addressof(buf)
    for fn in (lib.crp_rp_spmm_attention_ex, lib.crp_rp_spmm_attention_f32_ex):
        fn(None, 0, 1.0, 0, None, 0, None, 0, None, 0, None, 0, None, None, None)
        fn(None, 1, 0.5, 1, p, 1, p, 1, p, 1, p, 1, p, p, None)
    assert lib.crp_rp_spmm_attention_built(None) == 0
    assert bytes(buf) == bytes(64)


def test_device_entry_points_refuse_bad_arguments_without_a_device(crp):
    """A NULL handle is refused first, so no pointer below is ever dereferenced and every call returns -1 without a device; the
    codes that need a live handle (-4 for the leading dimensions, -1 for a missing source) are pinned in
    tests/test_gpu_attention.py::test_argument_errors_write_nothing."""
    lib = crp.load()
    buf = (C.c_double * 8)()
    p = C.addressof(buf)
    for fn in (lib.crp_attention_csr_f64, lib.crp_attention_csr_f32):
        assert fn(None, 4, 4, 1.0, 0, p, 4, p, 4, None, 0, p, 4, None, 0, p, 4, p, p, None, None) == -1
        assert fn(None, 0, 0, float("nan"), 7, None, 0, None, 0, None, 0, None, 0, None, 0, None, 0, None, None, None, None) == -1
    assert bytes(buf) == bytes(64)


M, K, N = 40, 36, 8


def _plan_only(crp):
    from crp_spmm_amd import comm, engine, gen
    rp, ci, va = gen.random_csr(M, K, 6, seed=3)
    sc = comm.SelfComm()
    return engine.RpSpmm(0, M, rp, ci, va, [0, K], N, sc, plan_only=True), sc, int(rp[-1])


class _Spy:
    def __init__(self, lib, called):
        self._lib, self._called = lib, called

    def __getattr__(self, name):
        if name in SYMBOLS:
            self._called.append(name)
        return getattr(self._lib, name)


def _refused(crp, monkeypatch, exc, call):
    e, sc, nnz = _plan_only(crp)
    called = []
    monkeypatch.setattr(e, "_lib", _Spy(e._lib, called))
    with pytest.raises(exc):
        call(e, nnz)
    assert called == []                         # (a plan-only engine would abort in the library)
    monkeypatch.undo()
    e.free()
    sc.free()


def test_engine_wrapper_refuses_before_any_library_call(crp, monkeypatch):
    f8, f4 = np.float64, np.float32
    z = lambda r, c, dt=f8: np.zeros((r, c), dt)
    good = lambda **kw: dict(dict(layout=0, Q=z(M, N), K=z(K, N), V=z(K, N), out=z(M, N)), **kw)

    def call(**kw):
        a = good(**kw)
        extra = {k: a.pop(k) for k in list(a) if k in ("scale", "bias", "lse", "p_out")}
        return lambda e, nnz: e.attention(a["layout"], a["Q"], a["K"], a["V"], a["out"],
                                          **{k: (v(nnz) if callable(v) else v) for k, v in extra.items()})
    for kw in (dict(Q=z(M, N, f4)), dict(K=z(K, N, f4)), dict(V=z(K, N, f4)), dict(out=z(M, N, f4)), dict(Q=[[0.0] * N] * M),
               dict(V=z(K, N).astype(np.int32)), dict(lse=np.zeros(M, f4)), dict(p_out=lambda nnz: np.zeros(nnz, f4)),
               dict(lse=[0.0] * M), dict(lse=np.zeros((M, 1)))):
        _refused(crp, monkeypatch, TypeError, call(**kw))
    for kw in (dict(Q=z(M - 1, N)), dict(K=z(K - 1, N)), dict(V=z(K - 1, N)), dict(V=z(K, N + 1)), dict(out=z(M, N - 1)),
               dict(Q=z(M, N + 1)), dict(lse=np.zeros(M - 1)), dict(lse=np.zeros(M + 1)), dict(p_out=lambda nnz: np.zeros(nnz - 1)),
               dict(p_out=lambda nnz: np.zeros(2 * nnz)[::2]), dict(bias=2), dict(scale=float("inf")), dict(scale=float("nan"))):
        _refused(crp, monkeypatch, ValueError, call(**kw))
    e, sc, nnz = _plan_only(crp)
    assert e.attention_built() is False
    e.free()
    sc.free()


class _Handle:
    """CsrDev.attention on an object that has the attributes the checks read and a library that fails the test when reached"""
    nrow, ncol, nnz = M, K, 50

    class _Lib:
        def __getattr__(self, name):
            pytest.fail("the library was reached (%s)" % name)
    _lib = _Lib()
    handle = None


def test_csrdev_attention_refuses_before_the_library(crp):
    import torch
    from crp_spmm_amd import hip
    h = _Handle()
    att = lambda *a, **kw: hip.CsrDev.attention(h, *a, **kw)
    t = lambda r, c, dt=torch.float64: torch.zeros((r, c), dtype=dt)
    Q, Kt, V = t(M, N), t(K, N), t(K, 5)
    with pytest.raises(TypeError):
        att(np.zeros((M, N)), Kt, V)
    with pytest.raises(TypeError):
        att(Q, Kt.float(), V)
    with pytest.raises(TypeError):
        att(Q, Kt, V.float())
    with pytest.raises(TypeError):
        att(Q, Kt, V, out=t(M, 5, torch.float32))
    with pytest.raises(TypeError):
        att(Q, Kt, V, lse=torch.zeros(M, dtype=torch.float32))
    with pytest.raises(TypeError):
        att(Q, Kt, V, p_out=np.zeros(50))
    with pytest.raises(TypeError):
        att(Q, Kt, V)                                           # well-formed, but on the host
    with pytest.raises(TypeError):
        att(Q, Kt, V, p_out=torch.zeros(50, dtype=torch.float64), out_pos=torch.zeros(50, dtype=torch.int64))
    for bad in (dict(K1=t(4, N)), dict(V1=t(4, 5)), dict(K1=t(4, N + 1), V1=t(4, 5)), dict(K1=t(4, N), V1=t(4, 6)),
                dict(K1=t(4, N), V1=t(3, 5)), dict(out=t(M, 6)), dict(out=t(M - 1, 5)), dict(lse=torch.zeros(M - 1, dtype=torch.float64)),
                dict(lse=torch.zeros((M, 1), dtype=torch.float64)), dict(p_out=torch.zeros(49, dtype=torch.float64)),
                dict(out_pos=torch.zeros(50, dtype=torch.int32)), dict(p_out=torch.zeros(50, dtype=torch.float64),
                                                                       out_pos=torch.zeros(49, dtype=torch.int32)),
                dict(bias=3), dict(scale=float("inf"))):
        with pytest.raises(ValueError):
            att(Q, Kt, V, **bad)
    for Qb, Kb, Vb in ((t(M - 1, N), Kt, V), (Q, t(K - 1, N), V), (Q, Kt, t(K - 1, 5)), (Q, t(K, N + 1), V), (t(M, 0), t(K, 0), V),
                       (torch.zeros((M, 2 * N), dtype=torch.float64)[:, ::2], Kt, V)):
        with pytest.raises(ValueError):
            att(Qb, Kb, Vb)
