"""CPU: the fused GATv2 attention without a device.  The new entry points exist with the documented prototypes, are bound in
_lib.SIGNATURES with matching ctypes and are exported; a NULL handle returns -1 and a NULL engine is a no-op; and every wrapper
error -- dtypes, shapes of XT / XS / a, heads, slope, bias, the per-row and per-nonzero tensors, the width cap of both directions --
is raised before any library call.  In the style of tests/test_gat_args.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

_SRC = "const %s *XT, long long ldXT, const %s *XS0, long long ldXS0, const %s *XS1, long long ldXS1, const %s *a, "
_FWD = ("int crp_gatv2_attention_csr_%s(crp_csr_dev_p A, int heads, int dv, double slope, int bias, " + _SRC +
        "%s *O, long long ldO, %s *lse, %s *p_out, const int *out_pos, void *stream);")
_ROW = ("int crp_gatv2_attention_bwd_row_csr_%s(crp_csr_dev_p A, int heads, int dv, double slope, int bias, " + _SRC +
        "const %s *O, long long ldO, const %s *dO, long long lddO, const %s *lse, %s *dXT, long long lddXT, %s *da_part, long long ldda, "
        "%s *delta, %s *ds_out, const int *out_pos, void *stream);")
_COL = ("int crp_gatv2_attention_bwd_col_csr_%s(crp_csr_dev_p At, int heads, int dv, double slope, int bias, const %s *XS, long long ldXS, "
        "const %s *XT, long long ldXT, const %s *a, const %s *dO, long long lddO, const %s *lse, const %s *delta, "
        "%s *dXS, long long lddXS, void *stream);")
_SUM = "int crp_col_sum_%s(int nrow, int n, const %s *src, long long lds, %s *work, %s *out, void *stream);"
_ENG = ("void crp_rp_spmm_gatv2%s_ex(crp_rp_spmm_p rp_spmm, int layout, int heads, double slope, int bias, const %s *XT, long long ldXT, "
        "const %s *a, const %s *XS, long long ldXS, %s *O, long long ldO, %s *lse, %s *p_out, void *stream);")
SYMBOLS = {"crp_rp_spmm_gatv2_built": ("crp_engine.h", "int crp_rp_spmm_gatv2_built(crp_rp_spmm_p rp_spmm);")}
for _sfx, _t_ in (("f64", "double"), ("f32", "float")):
    SYMBOLS["crp_gatv2_attention_csr_" + _sfx] = ("crpspmm_hip.h", _FWD % ((_sfx,) + (_t_,) * 7))
    SYMBOLS["crp_gatv2_attention_bwd_row_csr_" + _sfx] = ("crpspmm_hip.h", _ROW % ((_sfx,) + (_t_,) * 11))
    SYMBOLS["crp_gatv2_attention_bwd_col_csr_" + _sfx] = ("crpspmm_hip.h", _COL % ((_sfx,) + (_t_,) * 7))
    SYMBOLS["crp_col_sum_" + _sfx] = ("crpspmm_hip.h", _SUM % ((_sfx,) + (_t_,) * 3))
    _e = "" if _sfx == "f64" else "_f32"
    SYMBOLS["crp_rp_spmm_gatv2%s_ex" % _e] = ("crp_engine.h", _ENG % ((_e,) + (_t_,) * 6))


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


def test_the_width_error_is_the_attention_backwards(crp):
    text = open(os.path.join(ROOT, "include", "crpspmm_hip.h")).read()
    assert re.search(r"#define CRP_GATV2_EWIDTH \(-6\)", text) and re.search(r"#define CRP_ATTN_BWD_EWIDTH \(-6\)", text)


def test_a_null_handle_returns_minus_one_and_a_null_engine_is_a_no_op(crp):
    """A NULL handle is refused first, so no pointer is dereferenced and no device is needed; col_sum refuses its arguments before it
    launches; the codes that need a live handle are pinned in tests/test_gpu_gatv2.py."""
    lib = crp.load()
    buf = (C.c_double * 8)()
    p = C.addressof(buf)
    for sfx in ("f64", "f32"):
        fn = getattr(lib, "crp_gatv2_attention_csr_" + sfx)
        assert fn(None, 2, 4, 0.2, 0, p, 8, p, 8, None, 0, p, p, 8, p, p, None, None) == -1
        assert fn(None, 0, 0, float("nan"), 7, None, 0, None, 0, None, 0, None, None, 0, None, None, None, None) == -1
        fn = getattr(lib, "crp_gatv2_attention_bwd_row_csr_" + sfx)
        assert fn(None, 2, 4, 0.2, 0, p, 8, p, 8, None, 0, p, p, 8, p, 8, p, p, 8, p, 8, p, p, None, None) == -1
        assert fn(None, -1, 9999, 0.2, 0, None, 0, None, 0, None, 0, None, None, 0, None, 0, None, None, 0, None, 0, None, None, None, None) == -1
        fn = getattr(lib, "crp_gatv2_attention_bwd_col_csr_" + sfx)
        assert fn(None, 2, 4, 0.2, 0, p, 8, p, 8, p, p, 8, p, p, p, 8, None) == -1
        assert fn(None, 0, 9999, float("inf"), 0, None, 0, None, 0, None, None, 0, None, None, None, 0, None) == -1
        fn = getattr(lib, "crp_col_sum_" + sfx)
        assert fn(-1, 2, p, 2, p, p, None) == -1 and fn(2, -1, p, 2, p, p, None) == -1
        assert fn(2, 2, None, 2, p, p, None) == -1 and fn(2, 2, p, 2, None, p, None) == -1 and fn(2, 2, p, 2, p, None, None) == -1
        assert fn(2, 3, p, 2, p, p, None) == -4
    for fn in (lib.crp_rp_spmm_gatv2_ex, lib.crp_rp_spmm_gatv2_f32_ex):
        fn(None, 0, 2, 0.2, 0, None, 0, None, None, 0, None, 0, None, None, None)
        fn(None, 1, 0, float("nan"), 1, p, 1, p, p, 1, p, 1, p, p, None)             # (not even heads is looked at)
    assert lib.crp_rp_spmm_gatv2_built(None) == 0
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


def _common(call, first, rows):
    """what the three wrappers refuse alike; `call` fills in well-formed host operands; `first`: the name of the first operand"""
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
        call(heads=4)                                                           # 4 heads do not divide 6 columns
    for a in (torch.zeros(NV + 1, dtype=torch.float64), _t(H + 1, DV), _t(DV, H), _t(H, 2 * DV)[:, ::2], _t(1, NV)):
        with pytest.raises(ValueError):
            call(heads=H, a=a)
    for a in (np.zeros(NV), torch.zeros(NV, dtype=torch.float32)):
        with pytest.raises(TypeError):
            call(heads=H, a=a)
    with pytest.raises(TypeError):
        call(heads=H, **{first: _t(rows, NV, torch.float32)})
    with pytest.raises(TypeError):
        call(heads=H, **{first: np.zeros((rows, NV))})
    with pytest.raises(TypeError):
        call(heads=H, **{first: torch.zeros(rows * NV, dtype=torch.float64)})
    with pytest.raises(ValueError):
        call(heads=H, **{first: _t(NV, rows).t()})


def test_gatv2_attention_refuses_before_the_library(crp):
    import torch
    from crp_spmm_amd import hip
    h = _Handle()
    good = dict(XT=_t(M, NV), XS0=_t(K, NV), a=_t(H, DV))

    def call(**kw):
        a = dict(good, **kw)
        pos = [a.pop(k) for k in ("XT", "XS0", "a")]
        return hip.CsrDev.gatv2_attention(h, *pos, **a)
    _common(call, "XT", M)
    v = lambda n: torch.zeros(n, dtype=torch.float64)
    for kw in (dict(XS0=_t(K, NV + 1)), dict(XS0=_t(K - 1, NV)), dict(XT=_t(M - 1, NV)), dict(out=_t(M, NV + H)), dict(out=_t(M - 1, NV)),
               dict(XS1=_t(5, NV + H)), dict(lse=v(M * H)), dict(lse=_t(M, H + 1)), dict(lse=_t(M - 1, H)), dict(lse=_t(H, M).t()),
               dict(p_out=v(NNZ * H)), dict(p_out=_t(NNZ, H + 1)), dict(p_out=_t(NNZ - 1, H)), dict(p_out=_t(NNZ, 2 * H)[:, ::2]),
               dict(p_out=_t(NNZ, H), out_pos=torch.zeros(NNZ - 1, dtype=torch.int32)), dict(out_pos=torch.zeros(NNZ, dtype=torch.int32)),
               # the cap is per head and holds in the forward too: 2 x 513 columns are refused
               dict(XT=_t(M, 1026), XS0=_t(K, 1026), a=_t(2, 513))):
        with pytest.raises(ValueError):
            call(heads=H, **kw)
    with pytest.raises(TypeError):
        call(heads=H, p_out=_t(NNZ, H), out_pos=torch.zeros(NNZ, dtype=torch.int64))
    with pytest.raises(TypeError):
        call(heads=H, lse=_t(M, H, torch.float32))
    # 2 x 512 pass the checks and end at the host tensors; one head: 1-D and (n, 1) per-row tensors are both taken, a 1-D or (1, dv)
    with pytest.raises(TypeError):
        call(heads=H, XT=_t(M, 1024), XS0=_t(K, 1024), a=_t(2, 512))
    for lse, a in ((v(M), v(5)), (_t(M, 1), _t(1, 5))):
        with pytest.raises(TypeError):
            call(heads=1, XT=_t(M, 5), XS0=_t(K, 5), a=a, lse=lse)


def test_bwd_row_refuses_before_the_library(crp):
    import torch
    from crp_spmm_amd import hip
    h = _Handle()
    good = dict(XT=_t(M, NV), XS0=_t(K, NV), a=_t(H, DV), O=_t(M, NV), dO=_t(M, NV), lse=_t(M, H))

    def call(**kw):
        a = dict(good, **kw)
        pos = [a.pop(k) for k in ("XT", "XS0", "a", "O", "dO", "lse")]
        return hip.CsrDev.gatv2_attention_bwd_row(h, *pos, **a)
    _common(call, "XT", M)
    v = lambda n: torch.zeros(n, dtype=torch.float64)
    for kw in (dict(lse=v(M * H)), dict(lse=_t(M, H + 1)), dict(lse=_t(M - 1, H)), dict(delta=v(M * H)), dict(delta=_t(M - 1, H)),
               dict(dXT=_t(M, NV + 1)), dict(dXT=_t(M - 1, NV)), dict(da_part=_t(M, NV + 1)), dict(da_part=_t(M - 1, NV)),
               dict(dO=_t(M, NV + H)), dict(O=_t(M - 1, NV)), dict(ds_out=v(NNZ * H)), dict(ds_out=_t(NNZ - 1, H)), dict(ds_out=_t(NNZ, H + 1)),
               dict(out_pos=torch.zeros(NNZ, dtype=torch.int32)), dict(ds_out=_t(NNZ, H), out_pos=torch.zeros(NNZ + 1, dtype=torch.int32)),
               dict(XT=_t(M, 1026), XS0=_t(K, 1026), a=_t(2, 513), O=_t(M, 1026), dO=_t(M, 1026))):
        with pytest.raises(ValueError):
            call(heads=H, **kw)
    with pytest.raises(TypeError):
        call(heads=H, XT=_t(M, 1024), XS0=_t(K, 1024), a=_t(2, 512), O=_t(M, 1024), dO=_t(M, 1024))


def test_bwd_col_refuses_before_the_library(crp):
    import torch
    from crp_spmm_amd import hip
    h = _Handle()                                               # as a handle of A^T: M rows (XS), K columns (XT, dO)
    good = dict(XS=_t(M, NV), XT=_t(K, NV), a=_t(H, DV), dO=_t(K, NV), lse=_t(K, H), delta=_t(K, H))

    def call(**kw):
        a = dict(good, **kw)
        pos = [a.pop(k) for k in ("XS", "XT", "a", "dO", "lse", "delta")]
        return hip.CsrDev.gatv2_attention_bwd_col(h, *pos, **a)
    _common(call, "XS", M)
    v = lambda n: torch.zeros(n, dtype=torch.float64)
    for kw in (dict(lse=v(K * H)), dict(lse=_t(K, H + 1)), dict(lse=_t(K - 1, H)), dict(delta=v(K * H)), dict(delta=_t(K - 1, H)),
               dict(delta=_t(H, K).t()), dict(XT=_t(K - 1, NV)), dict(dO=_t(K - 1, NV)), dict(XS=_t(M - 1, NV)), dict(dXS=_t(M - 1, NV)),
               dict(dXS=_t(M, NV + H)), dict(XS=_t(M, 1026), XT=_t(K, 1026), a=_t(2, 513), dO=_t(K, 1026))):
        with pytest.raises(ValueError):
            call(heads=H, **kw)


def test_col_sum_refuses_before_the_library(crp, monkeypatch):
    import torch
    from crp_spmm_amd import hip, _lib
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was reached"))
    for src in (np.zeros((4, 3)), torch.zeros(12, dtype=torch.float64), torch.zeros((4, 3), dtype=torch.int32)):
        with pytest.raises(TypeError):
            hip.col_sum(src)
    with pytest.raises(ValueError):
        hip.col_sum(_t(3, 4).t())
    for out in (torch.zeros(4, dtype=torch.float64), _t(1, 6)[0, ::2]):
        with pytest.raises(ValueError):
            hip.col_sum(_t(4, 3), out=out)
    with pytest.raises(TypeError):
        hip.col_sum(_t(4, 3), out=torch.zeros(3, dtype=torch.float32))
    with pytest.raises(TypeError):
        hip.col_sum(_t(4, 3))                                                   # well-formed, but on the host


def test_gatv2_attention_function_refuses_a_wrong_transpose(crp):
    from crp_spmm_amd import hip

    class At(_Handle):
        nrow, ncol = K, M
    for heads, exc in ((0, ValueError), (-2, ValueError), (1.5, TypeError)):
        with pytest.raises(exc):
            hip.gatv2_attention(_Handle(), At(), _t(M, NV), _t(K, NV), _t(H, DV), heads=heads)
    with pytest.raises(ValueError):
        hip.gatv2_attention(_Handle(), _Handle(), _t(M, NV), _t(K, NV), _t(H, DV), heads=H)


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
        assert not [c for c in called if c.startswith("crp_rp_spmm_gatv2")], called
        monkeypatch.undo()
        assert e.gatv2_built() is False
        e.free()
        sc.free()
    z = lambda r, c: np.zeros((r, c))
    t = lambda r, c, dt=torch.float64: torch.zeros((r, c), dtype=dt)

    def fwd(**kw):
        a = dict(dict(XT=t(EM, EN), a=t(2, 4), XS=z(EK, EN), out=z(EM, EN), heads=2), **kw)
        pos = [a.pop(k) for k in ("XT", "a", "XS", "out")]
        return lambda e, nnz: e.gatv2_attention(0, *pos, **{k: (v(nnz) if callable(v) else v) for k, v in a.items()})
    for exc, kw in ((ValueError, dict(heads=0)), (ValueError, dict(heads=3)), (ValueError, dict(heads=16)), (TypeError, dict(heads=2.0)),
                    (TypeError, dict(heads=True)), (TypeError, dict(XT=z(EM, EN))), (TypeError, dict(a=z(2, 4))),
                    (TypeError, dict(XT=t(EM, EN, torch.float32))), (TypeError, dict(XT=torch.zeros(EM * EN, dtype=torch.float64))),
                    (ValueError, dict(XT=t(EM, EN + 1))), (ValueError, dict(XT=t(EM - 1, EN))), (ValueError, dict(XT=t(EN, EM).t())),
                    (ValueError, dict(a=t(4, 2))), (ValueError, dict(a=torch.zeros(EN + 1, dtype=torch.float64))),
                    (ValueError, dict(slope=float("nan"))), (ValueError, dict(bias=3)),
                    (ValueError, dict(XS=z(EK, EN + 1))), (ValueError, dict(out=z(EM - 1, EN))), (TypeError, dict(XS=z(EK, EN).astype(np.float32))),
                    (ValueError, dict(lse=np.zeros(EM * 2))), (ValueError, dict(lse=z(EM, 3))), (ValueError, dict(lse=z(EM - 1, 2))),
                    (TypeError, dict(lse=z(EM, 2).astype(np.float32))),
                    (ValueError, dict(p_out=lambda nnz: np.zeros(nnz * 2))), (ValueError, dict(p_out=lambda nnz: z(nnz - 1, 2))),
                    (TypeError, dict())):                                        # (last: well-formed, but XT and a are on the host)
        refused(exc, fwd(**kw))
