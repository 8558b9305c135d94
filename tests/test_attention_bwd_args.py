"""CPU: the fused attention backward, without a device.  The device entry points exist with the documented prototypes, are bound
in _lib.SIGNATURES with matching ctypes and are exported; they refuse a NULL handle before anything touches a device; and the
Python wrappers refuse mixed dtypes, wrong shapes, widths over the cap and tensors that are not on the device before any library
call."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_attention_args import _ctype_of

_Q = ("int crp_attention_bwd_q_csr_%s(crp_csr_dev_p A, int nk, int nv, double scale, int bias, const %s *Q, long long ldQ, "
      "const %s *K0, long long ldK0, const %s *K1, long long ldK1, const %s *V0, long long ldV0, const %s *V1, long long ldV1, "
      "const %s *O, long long ldO, const %s *dO, long long lddO, const %s *lse, %s *dQ, long long lddQ, %s *delta, %s *ds_out, "
      "const int *out_pos, void *stream);")
_KV = ("int crp_attention_bwd_kv_csr_%s(crp_csr_dev_p At, int nk, int nv, double scale, int bias, const %s *K, long long ldK, "
       "const %s *V, long long ldV, const %s *Q, long long ldQ, const %s *dO, long long lddO, const %s *lse, const %s *delta, "
       "%s *dK, long long lddK, %s *dV, long long lddV, void *stream);")
_ENG = ("void crp_rp_spmm_attention_bwd%s_ex(crp_rp_spmm_p rp_spmm, double scale, int bias, const %s *Q, long long ldQ, "
        "const %s *K, long long ldK, const %s *V, long long ldV, const %s *O, long long ldO, const %s *dO, long long lddO, "
        "const %s *lse, %s *dQ, long long lddQ, %s *dK, long long lddK, %s *dV, long long lddV, %s *ds_out, void *stream);")
SYMBOLS = {
    "crp_attention_bwd_q_csr_f64": ("crpspmm_hip.h", _Q % (("f64",) + ("double",) * 11)),
    "crp_attention_bwd_q_csr_f32": ("crpspmm_hip.h", _Q % (("f32",) + ("float",) * 11)),
    "crp_attention_bwd_kv_csr_f64": ("crpspmm_hip.h", _KV % (("f64",) + ("double",) * 8)),
    "crp_attention_bwd_kv_csr_f32": ("crpspmm_hip.h", _KV % (("f32",) + ("float",) * 8)),
    "crp_rp_spmm_attention_bwd_ex": ("crp_engine.h", _ENG % (("",) + ("double",) * 10)),
    "crp_rp_spmm_attention_bwd_f32_ex": ("crp_engine.h", _ENG % (("_f32",) + ("float",) * 10)),
    "crp_rp_spmm_attention_bwd_built": ("crp_engine.h", "int crp_rp_spmm_attention_bwd_built(crp_rp_spmm_p rp_spmm);"),
}


@pytest.mark.parametrize("name", sorted(SYMBOLS))
def test_symbol_is_exported_declared_and_bound(crp, name):
    from crp_spmm_amd import _lib
    header, proto = SYMBOLS[name]
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert any(ln.split()[-1] == name and " T " in ln for ln in out.splitlines()), "%s is not exported" % name
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", header)).read())
    assert proto in text, "%s is not declared in include/%s as documented" % (name, header)
    res, args = _lib.SIGNATURES[name]
    want = [_ctype_of(a) for a in proto[proto.index("(") + 1:proto.rindex(")")].split(",")]
    assert res == {"int": C.c_int, "void": None}[proto[:proto.index(" crp_")]] and list(args) == want, (name, args, want)
    fn = getattr(crp.load(), name)
    assert fn.restype == res and list(fn.argtypes) == want


def test_a_null_handle_is_refused_without_a_device(crp):
    lib = crp.load()
    buf = (C.c_double * 8)()
    p = C.addressof(buf)
    for fn in (lib.crp_attention_bwd_q_csr_f64, lib.crp_attention_bwd_q_csr_f32):
        assert fn(None, 4, 4, 1.0, 0, p, 4, p, 4, None, 0, p, 4, None, 0, p, 4, p, 4, p, p, 4, p, p, None, None) == -1
        assert fn(None, 0, 0, float("nan"), 7, None, 0, None, 0, None, 0, None, 0, None, 0, None, 0, None, 0, None, None, 0, None, None,
                  None, None) == -1
    for fn in (lib.crp_attention_bwd_kv_csr_f64, lib.crp_attention_bwd_kv_csr_f32):
        assert fn(None, 4, 4, 1.0, 0, p, 4, p, 4, p, 4, p, 4, p, p, p, 4, p, 4, None) == -1
        assert fn(None, 9999, 9999, 1.0, 0, None, 0, None, 0, None, 0, None, 0, None, None, None, 0, None, 0, None) == -1
    assert bytes(buf) == bytes(64)


def test_the_width_code_is_documented():
    text = open(os.path.join(ROOT, "include", "crpspmm_hip.h")).read()
    assert "#define CRP_ATTN_BWD_EWIDTH (-6)" in text


def test_null_engine_is_a_no_op_and_reads_not_built(crp):
    lib = crp.load()
    buf = (C.c_double * 8)()
    p = C.addressof(buf)
    for fn in (lib.crp_rp_spmm_attention_bwd_ex, lib.crp_rp_spmm_attention_bwd_f32_ex):
        fn(None, 1.0, 0, None, 0, None, 0, None, 0, None, 0, None, 0, None, None, 0, None, 0, None, 0, None, None)
        fn(None, 0.5, 1, p, 1, p, 1, p, 1, p, 1, p, 1, p, p, 1, p, 1, p, 1, p, None)
    assert lib.crp_rp_spmm_attention_bwd_built(None) == 0
    assert bytes(buf) == bytes(64)


def test_engine_wrapper_refuses_before_any_library_call(crp, monkeypatch):
    """a plan-only engine would abort in the library: every refusal below comes from the wrapper"""
    import torch
    from test_attention_args import _plan_only, M as EM, K as EK, N as EN

    class Spy:
        def __init__(self, lib, called):
            self._lib, self._called = lib, called

        def __getattr__(self, name):
            self._called.append(name)
            return getattr(self._lib, name)
    f4 = torch.float32
    z = lambda r, c, dt=torch.float64: torch.zeros((r, c), dtype=dt)
    good = dict(Q=z(EM, EN), K=z(EK, EN), V=z(EK, EN), O=z(EM, EN), dO=z(EM, EN), lse=torch.zeros(EM, dtype=torch.float64), dQ=z(EM, EN),
                dK=z(EK, EN), dV=z(EK, EN))
    cases = [(TypeError, dict(Q=np.zeros((EM, EN)))), (TypeError, dict(K=z(EK, EN, f4))), (TypeError, dict(dV=z(EK, EN, f4))),
             (TypeError, dict(lse=torch.zeros(EM, dtype=f4))), (TypeError, dict(Q=torch.zeros(EM, dtype=torch.float64))),
             (ValueError, dict(Q=z(EM - 1, EN))), (ValueError, dict(K=z(EK + 1, EN))), (ValueError, dict(dO=z(EM, EN + 1))),
             (ValueError, dict(dK=z(EK - 1, EN))), (ValueError, dict(lse=torch.zeros(EM - 1, dtype=torch.float64))),
             (ValueError, dict(ds_out=torch.zeros(3, dtype=torch.float64))), (ValueError, dict(bias=2)), (ValueError, dict(scale=float("nan"))),
             (TypeError, dict())]                               # (last: well-formed, but on the host)
    for exc, kw in cases:
        e, sc, nnz = _plan_only(crp)
        called = []
        monkeypatch.setattr(e, "_lib", Spy(e._lib, called))
        a = dict(good, **kw)
        extra = {k: a.pop(k) for k in list(a) if k in ("scale", "bias", "ds_out")}
        with pytest.raises(exc):
            e.attention_bwd(a["Q"], a["K"], a["V"], a["O"], a["dO"], a["lse"], a["dQ"], a["dK"], a["dV"], **extra)
        assert not [c for c in called if c.startswith("crp_rp_spmm_attention_bwd")], called
        monkeypatch.undo()
        assert e.attention_bwd_built() is False
        e.free()
        sc.free()


M, K, N, NV = 40, 36, 8, 5


class _Handle:
    """the wrappers on an object that has the attributes the checks read and a library that fails the test when reached"""
    nrow, ncol, nnz = M, K, 50

    class _Lib:
        def __getattr__(self, name):
            pytest.fail("the library was reached (%s)" % name)
    _lib = _Lib()
    handle = None


def _t(r, c, dt=None):
    import torch
    return torch.zeros((r, c), dtype=dt or torch.float64)


def _v(n, dt=None):
    import torch
    return torch.zeros(n, dtype=dt or torch.float64)


def test_bwd_q_refuses_before_the_library(crp):
    import torch
    from crp_spmm_amd import hip
    h = _Handle()
    f4 = torch.float32
    good = dict(Q=_t(M, N), K0=_t(K, N), V0=_t(K, NV), O=_t(M, NV), dO=_t(M, NV), lse=_v(M))

    def call(**kw):
        a = dict(good, **kw)
        pos = [a.pop(k) for k in ("Q", "K0", "V0", "O", "dO", "lse")]
        return hip.CsrDev.attention_bwd_q(h, *pos, **a)
    for kw in (dict(Q=np.zeros((M, N))), dict(K0=_t(K, N, f4)), dict(V0=_t(K, NV, f4)), dict(O=_t(M, NV, f4)), dict(dO=_t(M, NV, f4)),
               dict(lse=_v(M, f4)), dict(dQ=_t(M, N, f4)), dict(delta=_v(M, f4)), dict(ds_out=np.zeros(50)), dict(lse=[0.0] * M),
               dict(Q=_v(M)), dict(ds_out=_v(50), out_pos=torch.zeros(50, dtype=torch.int64)), dict()):      # (last: on the host)
        with pytest.raises(TypeError):
            call(**kw)
    for kw in (dict(K1=_t(4, N)), dict(V1=_t(4, NV)), dict(K1=_t(4, N + 1), V1=_t(4, NV)), dict(K1=_t(4, N), V1=_t(3, NV)),
               dict(Q=_t(M - 1, N)), dict(K0=_t(K - 1, N)), dict(V0=_t(K - 1, NV)), dict(K0=_t(K, N + 1)), dict(O=_t(M, NV + 1)),
               dict(O=_t(M - 1, NV)), dict(dO=_t(M, NV - 1)), dict(dO=_t(M - 1, NV)), dict(dQ=_t(M, N + 1)), dict(dQ=_t(M - 1, N)),
               dict(lse=_v(M - 1)), dict(lse=_v(M - 2)), dict(delta=_v(M - 1)),
               dict(lse=_v(2 * M)[::2]), dict(ds_out=_v(49)), dict(out_pos=torch.zeros(50, dtype=torch.int32)),
               dict(ds_out=_v(50), out_pos=torch.zeros(49, dtype=torch.int32)), dict(bias=3), dict(scale=float("inf")),
               dict(scale=float("nan")), dict(Q=_t(M, 0), K0=_t(K, 0)), dict(Q=_t(M, 2 * N)[:, ::2]),
               dict(Q=_t(M, 513), K0=_t(K, 513)), dict(V0=_t(K, 513), O=_t(M, 513), dO=_t(M, 513)),
               dict(Q=_t(M, 1025, f4), K0=_t(K, 1025, f4), V0=_t(K, NV, f4), O=_t(M, NV, f4), dO=_t(M, NV, f4), lse=_v(M, f4))):
        with pytest.raises(ValueError):
            call(**kw)


def test_bwd_kv_refuses_before_the_library(crp):
    import torch
    from crp_spmm_amd import hip
    h = _Handle()                                               # as a handle of A^T: M rows (K, V), K columns (Q, dO)
    f4 = torch.float32
    good = dict(K=_t(M, N), V=_t(M, NV), Q=_t(K, N), dO=_t(K, NV), lse=_v(K), delta=_v(K))

    def call(**kw):
        a = dict(good, **kw)
        pos = [a.pop(k) for k in ("K", "V", "Q", "dO", "lse", "delta")]
        return hip.CsrDev.attention_bwd_kv(h, *pos, **a)
    for kw in (dict(K=np.zeros((M, N))), dict(V=_t(M, NV, f4)), dict(Q=_t(K, N, f4)), dict(dO=_t(K, NV, f4)), dict(lse=_v(K, f4)),
               dict(delta=_v(K, f4)), dict(dK=_t(M, N, f4)), dict(dV=_t(M, NV, f4)), dict(delta=None), dict(K=_v(M)), dict()):
        with pytest.raises(TypeError):
            call(**kw)
    for kw in (dict(K=_t(M - 1, N)), dict(V=_t(M - 1, NV)), dict(Q=_t(K - 1, N)), dict(dO=_t(K - 1, NV)), dict(Q=_t(K, N + 1)),
               dict(dO=_t(K, NV + 1)), dict(dK=_t(M, N + 1)), dict(dV=_t(M, NV - 1)), dict(dK=_t(M - 1, N)), dict(lse=_v(K - 1)),
               dict(delta=_v(K - 1)), dict(delta=_v(2 * K)[::2]), dict(bias=-1), dict(scale=float("nan")),
               dict(K=_t(M, 513), Q=_t(K, 513)), dict(V=_t(M, 513), dO=_t(K, 513))):
        with pytest.raises(ValueError):
            call(**kw)


def test_sparse_attention_refuses_handles_that_do_not_match(crp):
    from crp_spmm_amd import hip

    class Other(_Handle):
        nrow, ncol, nnz = K, M, 49                              # the transposed shape, another nonzero count
    with pytest.raises(ValueError):
        hip.sparse_attention(_Handle(), Other(), _t(M, N), _t(K, N), _t(K, NV))
    with pytest.raises(ValueError):
        hip.sparse_attention(_Handle(), _Handle(), _t(M, N), _t(K, N), _t(K, NV))      # (not transposed)
