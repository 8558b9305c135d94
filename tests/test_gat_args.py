"""CPU: the fused GAT attention without a device.  The new entry points exist with the documented prototypes, are bound in
_lib.SIGNATURES with matching ctypes and are exported; a NULL handle returns -1 and a NULL engine is a no-op; and every wrapper
error -- dtypes, shapes of el / er / V, heads, slope, bias, the per-row and per-nonzero tensors, the width cap of the backward -- is
raised before any library call.  In the style of tests/test_attention_mh_args.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

_SRC = ("const %s *el, long long ldel, const %s *er0, long long lder0, const %s *er1, long long lder1, const %s *V0, long long ldV0, "
        "const %s *V1, long long ldV1, ")
_FWD = ("int crp_gat_attention_csr_%s(crp_csr_dev_p A, int heads, int dv, double slope, int bias, " + _SRC +
        "%s *O, long long ldO, %s *lse, %s *p_out, const int *out_pos, void *stream);")
_ROW = ("int crp_gat_attention_bwd_row_csr_%s(crp_csr_dev_p A, int heads, int dv, double slope, int bias, " + _SRC +
        "const %s *O, long long ldO, const %s *dO, long long lddO, const %s *lse, %s *d_el, long long ldd_el, %s *delta, %s *ds_out, "
        "const int *out_pos, void *stream);")
_COL = ("int crp_gat_attention_bwd_col_csr_%s(crp_csr_dev_p At, int heads, int dv, double slope, int bias, const %s *er, long long lder, "
        "const %s *V, long long ldV, const %s *el, long long ldel, const %s *dO, long long lddO, const %s *lse, const %s *delta, "
        "%s *d_er, long long ldd_er, %s *dV, long long lddV, void *stream);")
_ENG = ("void crp_rp_spmm_gat%s_ex(crp_rp_spmm_p rp_spmm, int layout, int heads, double slope, int bias, const %s *el, long long ldel, "
        "const %s *er, long long lder, const %s *V, long long ldV, %s *O, long long ldO, %s *lse, %s *p_out, void *stream);")
SYMBOLS = {"crp_rp_spmm_gat_built": ("crp_engine.h", "int crp_rp_spmm_gat_built(crp_rp_spmm_p rp_spmm);")}
for _sfx, _t_ in (("f64", "double"), ("f32", "float")):
    SYMBOLS["crp_gat_attention_csr_" + _sfx] = ("crpspmm_hip.h", _FWD % ((_sfx,) + (_t_,) * 8))
    SYMBOLS["crp_gat_attention_bwd_row_csr_" + _sfx] = ("crpspmm_hip.h", _ROW % ((_sfx,) + (_t_,) * 11))
    SYMBOLS["crp_gat_attention_bwd_col_csr_" + _sfx] = ("crpspmm_hip.h", _COL % ((_sfx,) + (_t_,) * 8))
    _e = "" if _sfx == "f64" else "_f32"
    SYMBOLS["crp_rp_spmm_gat%s_ex" % _e] = ("crp_engine.h", _ENG % ((_e,) + (_t_,) * 6))


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


def test_a_null_handle_returns_minus_one_and_a_null_engine_is_a_no_op(crp):
    """A NULL handle is refused first, so no pointer is dereferenced and no device is needed; the codes that need a live handle are
    pinned in tests/test_gpu_gat.py."""
    lib = crp.load()
    buf = (C.c_double * 8)()
    p = C.addressof(buf)
    for sfx in ("f64", "f32"):
        fn = getattr(lib, "crp_gat_attention_csr_" + sfx)
        assert fn(None, 2, 4, 0.2, 0, p, 2, p, 2, None, 0, p, 8, None, 0, p, 8, p, p, None, None) == -1
        assert fn(None, 0, 0, float("nan"), 7, None, 0, None, 0, None, 0, None, 0, None, 0, None, 0, None, None, None, None) == -1
        fn = getattr(lib, "crp_gat_attention_bwd_row_csr_" + sfx)
        assert fn(None, 2, 4, 0.2, 0, p, 2, p, 2, None, 0, p, 8, None, 0, p, 8, p, 8, p, p, 2, p, p, None, None) == -1
        assert fn(None, -1, 9999, 0.2, 0, None, 0, None, 0, None, 0, None, 0, None, 0, None, 0, None, 0, None, None, 0, None, None, None,
                  None) == -1
        fn = getattr(lib, "crp_gat_attention_bwd_col_csr_" + sfx)
        assert fn(None, 2, 4, 0.2, 0, p, 2, p, 8, p, 2, p, 8, p, p, p, 2, p, 8, None) == -1
        assert fn(None, 0, 9999, float("inf"), 0, None, 0, None, 0, None, 0, None, 0, None, None, None, 0, None, 0, None) == -1
    for fn in (lib.crp_rp_spmm_gat_ex, lib.crp_rp_spmm_gat_f32_ex):
        fn(None, 0, 2, 0.2, 0, None, 0, None, 0, None, 0, None, 0, None, None, None)
        fn(None, 1, 0, float("nan"), 1, p, 1, p, 1, p, 1, p, 1, p, p, None)          # (not even heads is looked at)
    assert lib.crp_rp_spmm_gat_built(None) == 0
    assert bytes(buf) == bytes(64)


M, K, H, DV = 40, 36, 2, 3
NV, NNZ = H * DV, 50


class _Handle:
    """the wrappers on an object that has the attributes the checks read and a library that fails the test when reached"""
    nrow, ncol, nnz = M, K, NNZ

    class _Lib:
        def __getattr__(self, name):
            pytest.fail("the library was reached (%s)" % name)
    _lib = _Lib()
    handle = None


def _t(r, c, dt=None):
    import torch
    return torch.zeros((r, c), dtype=dt or torch.float64)


def _common(call):
    """what the three wrappers refuse alike; `call` fills in well-formed host operands"""
    import torch
    for heads in (0, -1):
        with pytest.raises(ValueError):
            call(heads=heads)
    for heads in (2.0, "2", None, True):
        with pytest.raises(TypeError):
            call(heads=heads)
    with pytest.raises(TypeError):
        call(heads=H)                                                           # well-formed, but on the host
    for kw in (dict(slope=float("nan")), dict(slope=float("inf")), dict(bias=2), dict(bias="yes")):
        with pytest.raises(ValueError):
            call(heads=H, **kw)
    with pytest.raises(ValueError):
        call(heads=3)                                                           # el and er have H columns
    with pytest.raises(TypeError):
        call(heads=H, el=_t(M, H, torch.float32))
    with pytest.raises(TypeError):
        call(heads=H, el=np.zeros((M, H)))
    with pytest.raises(TypeError):
        call(heads=H, el=torch.zeros(M * H, dtype=torch.float64))
    with pytest.raises(ValueError):
        call(heads=H, el=_t(H, M).t())


def test_gat_attention_refuses_before_the_library(crp):
    import torch
    from crp_spmm_amd import hip
    h = _Handle()
    good = dict(el=_t(M, H), er0=_t(K, H), V0=_t(K, NV))

    def call(**kw):
        a = dict(good, **kw)
        pos = [a.pop(k) for k in ("el", "er0", "V0")]
        return hip.CsrDev.gat_attention(h, *pos, **a)
    _common(call)
    v = lambda n: torch.zeros(n, dtype=torch.float64)
    for kw in (dict(V0=_t(K, NV + 1)), dict(er0=_t(K, H + 1)), dict(er0=_t(K - 1, H)), dict(V0=_t(K - 1, NV)), dict(el=_t(M - 1, H)),
               dict(out=_t(M, NV + H)), dict(out=_t(M - 1, NV)), dict(er1=_t(5, H)), dict(er1=_t(5, H), V1=_t(6, NV)),
               dict(er1=_t(5, H), V1=_t(5, NV + H)), dict(lse=v(M * H)), dict(lse=_t(M, H + 1)), dict(lse=_t(M - 1, H)), dict(lse=_t(H, M).t()),
               dict(p_out=v(NNZ * H)), dict(p_out=_t(NNZ, H + 1)), dict(p_out=_t(NNZ - 1, H)), dict(p_out=_t(NNZ, 2 * H)[:, ::2]),
               dict(p_out=_t(NNZ, H), out_pos=torch.zeros(NNZ - 1, dtype=torch.int32)), dict(out_pos=torch.zeros(NNZ, dtype=torch.int32))):
        with pytest.raises(ValueError):
            call(heads=H, **kw)
    with pytest.raises(TypeError):
        call(heads=H, p_out=_t(NNZ, H), out_pos=torch.zeros(NNZ, dtype=torch.int64))
    with pytest.raises(TypeError):
        call(heads=H, lse=_t(M, H, torch.float32))
    # one head: 1-D and (n, 1) per-row tensors are both taken (and then found on the host); the forward has no width cap
    for lse in (v(M), _t(M, 1)):
        with pytest.raises(TypeError):
            call(heads=1, el=_t(M, 1), er0=_t(K, 1), V0=_t(K, 1100), lse=lse)


def test_bwd_row_refuses_before_the_library(crp):
    import torch
    from crp_spmm_amd import hip
    h = _Handle()
    good = dict(el=_t(M, H), er0=_t(K, H), V0=_t(K, NV), O=_t(M, NV), dO=_t(M, NV), lse=_t(M, H))

    def call(**kw):
        a = dict(good, **kw)
        pos = [a.pop(k) for k in ("el", "er0", "V0", "O", "dO", "lse")]
        return hip.CsrDev.gat_attention_bwd_row(h, *pos, **a)
    _common(call)
    v = lambda n: torch.zeros(n, dtype=torch.float64)
    for kw in (dict(lse=v(M * H)), dict(lse=_t(M, H + 1)), dict(lse=_t(M - 1, H)), dict(delta=v(M * H)), dict(delta=_t(M - 1, H)),
               dict(d_el=_t(M, H + 1)), dict(d_el=_t(M - 1, H)), dict(dO=_t(M, NV + H)), dict(O=_t(M - 1, NV)),
               dict(ds_out=v(NNZ * H)), dict(ds_out=_t(NNZ - 1, H)), dict(ds_out=_t(NNZ, H + 1)),
               dict(out_pos=torch.zeros(NNZ, dtype=torch.int32)), dict(ds_out=_t(NNZ, H), out_pos=torch.zeros(NNZ + 1, dtype=torch.int32)),
               # the cap is per head: 2 x 513 columns are refused, 2 x 512 pass the checks and end at the host tensors
               dict(V0=_t(K, 1026), O=_t(M, 1026), dO=_t(M, 1026))):
        with pytest.raises(ValueError):
            call(heads=H, **kw)
    with pytest.raises(TypeError):
        call(heads=H, V0=_t(K, 1024), O=_t(M, 1024), dO=_t(M, 1024))


def test_bwd_col_refuses_before_the_library(crp):
    import torch
    from crp_spmm_amd import hip
    h = _Handle()                                               # as a handle of A^T: M rows (er, V), K columns (el, dO)
    good = dict(er=_t(M, H), V=_t(M, NV), el=_t(K, H), dO=_t(K, NV), lse=_t(K, H), delta=_t(K, H))

    def call(**kw):
        a = dict(good, **kw)
        if "el" in kw and kw["el"] is not good["el"] and "er" not in kw:            # (_common varies the first operand: here er)
            a["er"], a["el"] = kw["el"], good["el"]
        pos = [a.pop(k) for k in ("er", "V", "el", "dO", "lse", "delta")]
        return hip.CsrDev.gat_attention_bwd_col(h, *pos, **a)
    _common(call)
    v = lambda n: torch.zeros(n, dtype=torch.float64)
    for kw in (dict(lse=v(K * H)), dict(lse=_t(K, H + 1)), dict(lse=_t(K - 1, H)), dict(delta=v(K * H)), dict(delta=_t(K - 1, H)),
               dict(delta=_t(H, K).t()), dict(el=_t(K - 1, H), er=good["er"]), dict(dO=_t(K - 1, NV)), dict(er=_t(M - 1, H)),
               dict(d_er=_t(M, H + 1)), dict(dV=_t(M - 1, NV)), dict(dV=_t(M, NV + H)), dict(V=_t(M, 1026), dO=_t(K, 1026))):
        with pytest.raises(ValueError):
            call(heads=H, **kw)


def test_gat_attention_function_refuses_a_wrong_transpose(crp):
    from crp_spmm_amd import hip

    class At(_Handle):
        nrow, ncol = K, M
    for heads, exc in ((0, ValueError), (-2, ValueError), (1.5, TypeError)):
        with pytest.raises(exc):
            hip.gat_attention(_Handle(), At(), _t(M, H), _t(K, H), _t(K, NV), heads=heads)
    with pytest.raises(ValueError):
        hip.gat_attention(_Handle(), _Handle(), _t(M, H), _t(K, H), _t(K, NV), heads=H)


def test_engine_wrapper_refuses_before_any_library_call(crp, monkeypatch):
    """a plan-only engine would abort in the library: every refusal below comes from the wrapper"""
    import torch
    from test_attention_args import _plan_only, M as EM, K as EK, N as EN           # (EN = 8 columns: 2 heads of 4)

    class Spy:
        def __init__(self, lib, called):
            self._lib, self._called = lib, called

        def __getattr__(self, name):
            self._called.append(name)
            return getattr(self._lib, name)

    def refused(exc, call):
        e, sc, nnz = _plan_only(crp)
        called = []
        monkeypatch.setattr(e, "_lib", Spy(e._lib, called))
        with pytest.raises(exc):
            call(e, nnz)
        assert not [c for c in called if c.startswith("crp_rp_spmm_gat")], called
        monkeypatch.undo()
        assert e.gat_built() is False
        e.free()
        sc.free()
    z = lambda r, c: np.zeros((r, c))
    t = lambda r, c, dt=torch.float64: torch.zeros((r, c), dtype=dt)

    def fwd(**kw):
        a = dict(dict(el=t(EM, 2), er=t(EK, 2), V=z(EK, EN), out=z(EM, EN), heads=2), **kw)
        pos = [a.pop(k) for k in ("el", "er", "V", "out")]
        return lambda e, nnz: e.gat_attention(0, *pos, **{k: (v(nnz) if callable(v) else v) for k, v in a.items()})
    for exc, kw in ((ValueError, dict(heads=0)), (ValueError, dict(heads=3)), (ValueError, dict(heads=16)), (TypeError, dict(heads=2.0)),
                    (TypeError, dict(heads=True)), (TypeError, dict(el=z(EM, 2))), (TypeError, dict(er=z(EK, 2))),
                    (TypeError, dict(el=t(EM, 2, torch.float32))), (TypeError, dict(el=torch.zeros(EM * 2, dtype=torch.float64))),
                    (ValueError, dict(el=t(EM, 3))), (ValueError, dict(er=t(EK - 1, 2))), (ValueError, dict(el=t(2, EM).t())),
                    (ValueError, dict(heads=4)),                                 # (el and er have two columns)
                    (ValueError, dict(slope=float("nan"))), (ValueError, dict(bias=3)),
                    (ValueError, dict(V=z(EK, EN + 1))), (ValueError, dict(out=z(EM - 1, EN))), (TypeError, dict(V=z(EK, EN).astype(np.float32))),
                    (ValueError, dict(lse=np.zeros(EM * 2))), (ValueError, dict(lse=z(EM, 3))), (ValueError, dict(lse=z(EM - 1, 2))),
                    (TypeError, dict(lse=z(EM, 2).astype(np.float32))),
                    (ValueError, dict(p_out=lambda nnz: np.zeros(nnz * 2))), (ValueError, dict(p_out=lambda nnz: z(nnz - 1, 2))),
                    (TypeError, dict())):                                        # (last: well-formed, but el and er are on the host)
        refused(exc, fwd(**kw))
