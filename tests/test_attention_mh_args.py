"""CPU: the multi-head forms of the fused attention and its backward, without a device.  The new entry points exist with the
documented prototypes, are bound in _lib.SIGNATURES with matching ctypes and are exported; a NULL handle returns -1 and a NULL
engine is a no-op; and every wrapper error of ``heads`` -- widths that the heads do not divide, wrong shapes of lse / delta /
p_out / ds_out, heads < 1 -- is raised before any library call.  In the style of tests/test_attention_args.py and
tests/test_attention_bwd_args.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

_KV0 = ("const %s *K0, long long ldK0, const %s *K1, long long ldK1, const %s *V0, long long ldV0, const %s *V1, long long ldV1, ")
_FWD = ("int crp_attention_mh_csr_%s(crp_csr_dev_p A, int heads, int dk, int dv, double scale, int bias, const %s *Q, long long ldQ, "
        + _KV0 + "%s *O, long long ldO, %s *lse, %s *p_out, const int *out_pos, void *stream);")
_BQ = ("int crp_attention_bwd_q_mh_csr_%s(crp_csr_dev_p A, int heads, int dk, int dv, double scale, int bias, const %s *Q, long long ldQ, "
       + _KV0 + "const %s *O, long long ldO, const %s *dO, long long lddO, const %s *lse, %s *dQ, long long lddQ, %s *delta, %s *ds_out, "
       "const int *out_pos, void *stream);")
_BKV = ("int crp_attention_bwd_kv_mh_csr_%s(crp_csr_dev_p At, int heads, int dk, int dv, double scale, int bias, const %s *K, long long ldK, "
        "const %s *V, long long ldV, const %s *Q, long long ldQ, const %s *dO, long long lddO, const %s *lse, const %s *delta, "
        "%s *dK, long long lddK, %s *dV, long long lddV, void *stream);")
_ENG = ("void crp_rp_spmm_attention_mh%s_ex(crp_rp_spmm_p rp_spmm, int layout, int heads, double scale, int bias, const %s *Q, "
        "long long ldQ, const %s *K, long long ldK, const %s *V, long long ldV, %s *O, long long ldO, %s *lse, %s *p_out, void *stream);")
_ENGB = ("void crp_rp_spmm_attention_bwd_mh%s_ex(crp_rp_spmm_p rp_spmm, int heads, double scale, int bias, const %s *Q, long long ldQ, "
         "const %s *K, long long ldK, const %s *V, long long ldV, const %s *O, long long ldO, const %s *dO, long long lddO, "
         "const %s *lse, %s *dQ, long long lddQ, %s *dK, long long lddK, %s *dV, long long lddV, %s *ds_out, void *stream);")
SYMBOLS = {}
for _sfx, _t_ in (("f64", "double"), ("f32", "float")):
    SYMBOLS["crp_attention_mh_csr_" + _sfx] = ("crpspmm_hip.h", _FWD % ((_sfx,) + (_t_,) * 8))
    SYMBOLS["crp_attention_bwd_q_mh_csr_" + _sfx] = ("crpspmm_hip.h", _BQ % ((_sfx,) + (_t_,) * 11))
    SYMBOLS["crp_attention_bwd_kv_mh_csr_" + _sfx] = ("crpspmm_hip.h", _BKV % ((_sfx,) + (_t_,) * 8))
    _e = "" if _sfx == "f64" else "_f32"
    SYMBOLS["crp_rp_spmm_attention_mh%s_ex" % _e] = ("crp_engine.h", _ENG % ((_e,) + (_t_,) * 6))
    SYMBOLS["crp_rp_spmm_attention_bwd_mh%s_ex" % _e] = ("crp_engine.h", _ENGB % ((_e,) + (_t_,) * 10))


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


def test_the_streams_section_names_the_multi_head_calls():
    text = re.sub(r"[\s*]+", " ", open(os.path.join(ROOT, "include", "crpspmm_hip.h")).read())
    head = text[text.index("Streams."):text.index("#ifndef CRPSPMM_HIP_H")]
    for name in ("crp_attention_mh_csr_", "crp_attention_bwd_q_mh_csr_", "crp_attention_bwd_kv_mh_csr_"):
        assert name in head, name
    assert "allocate nothing, wait for nothing and touch no other stream" in head


def test_a_null_handle_returns_minus_one_and_a_null_engine_is_a_no_op(crp):
    """A NULL handle is refused first, so no pointer is dereferenced and no device is needed; the codes that need a live handle are
    pinned in tests/test_gpu_attention_mh.py::test_error_codes_that_need_a_live_handle."""
    lib = crp.load()
    buf = (C.c_double * 8)()
    p = C.addressof(buf)
    for sfx in ("f64", "f32"):
        fn = getattr(lib, "crp_attention_mh_csr_" + sfx)
        assert fn(None, 2, 4, 4, 1.0, 0, p, 8, p, 8, None, 0, p, 8, None, 0, p, 8, p, p, None, None) == -1
        assert fn(None, 0, 0, 0, float("nan"), 7, None, 0, None, 0, None, 0, None, 0, None, 0, None, 0, None, None, None, None) == -1
        fn = getattr(lib, "crp_attention_bwd_q_mh_csr_" + sfx)
        assert fn(None, 2, 4, 4, 1.0, 0, p, 8, p, 8, None, 0, p, 8, None, 0, p, 8, p, 8, p, p, 8, p, p, None, None) == -1
        assert fn(None, -1, 9999, 9999, 1.0, 0, None, 0, None, 0, None, 0, None, 0, None, 0, None, 0, None, 0, None, None, 0, None, None,
                  None, None) == -1
        fn = getattr(lib, "crp_attention_bwd_kv_mh_csr_" + sfx)
        assert fn(None, 2, 4, 4, 1.0, 0, p, 8, p, 8, p, 8, p, 8, p, p, p, 8, p, 8, None) == -1
        assert fn(None, 0, 9999, 9999, 1.0, 0, None, 0, None, 0, None, 0, None, 0, None, None, None, 0, None, 0, None) == -1
    for fn in (lib.crp_rp_spmm_attention_mh_ex, lib.crp_rp_spmm_attention_mh_f32_ex):
        fn(None, 0, 2, 1.0, 0, None, 0, None, 0, None, 0, None, 0, None, None, None)
        fn(None, 1, 0, 0.5, 1, p, 1, p, 1, p, 1, p, 1, p, p, None)                  # (not even heads is looked at)
    for fn in (lib.crp_rp_spmm_attention_bwd_mh_ex, lib.crp_rp_spmm_attention_bwd_mh_f32_ex):
        fn(None, 2, 1.0, 0, None, 0, None, 0, None, 0, None, 0, None, 0, None, None, 0, None, 0, None, 0, None, None)
        fn(None, -3, 0.5, 1, p, 1, p, 1, p, 1, p, 1, p, 1, p, p, 1, p, 1, p, 1, p, None)
    assert lib.crp_rp_spmm_attention_built(None) == 0 and lib.crp_rp_spmm_attention_bwd_built(None) == 0
    assert bytes(buf) == bytes(64)


M, K, H, DK, DV = 40, 36, 2, 4, 3
N, NV, NNZ = H * DK, H * DV, 50


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


def _bad_heads(call):
    for heads in (0, -1):
        with pytest.raises(ValueError):
            call(heads=heads)
    for heads in (2.0, "2", None, True):
        with pytest.raises(TypeError):
            call(heads=heads)


def test_csrdev_attention_refuses_before_the_library(crp):
    import torch
    from crp_spmm_amd import hip
    h = _Handle()
    Q, Kt, V = _t(M, N), _t(K, N), _t(K, NV)
    att = lambda **kw: hip.CsrDev.attention(h, kw.pop("Q", Q), kw.pop("K0", Kt), kw.pop("V0", V), **kw)
    _bad_heads(att)
    with pytest.raises(TypeError):
        att(heads=H, lse=_t(M, H), p_out=_t(NNZ, H))                            # well-formed, but on the host
    with pytest.raises(TypeError):
        att(heads=H, lse=_t(M, H, torch.float32))
    for kw in (dict(heads=3), dict(heads=4), dict(heads=H, Q=_t(M, N + 1), K0=_t(K, N + 1)), dict(heads=H, V0=_t(K, NV + 1)),
               dict(heads=H, lse=torch.zeros(M * H, dtype=torch.float64)), dict(heads=H, lse=_t(M, H + 1)), dict(heads=H, lse=_t(M, 1)),
               dict(heads=H, lse=_t(M - 1, H)), dict(heads=H, lse=_t(H, M).t()), dict(heads=H, lse=_t(M, 2 * H)[:, ::2]),
               dict(heads=H, p_out=torch.zeros(NNZ * H, dtype=torch.float64)), dict(heads=H, p_out=_t(NNZ, H + 1)),
               dict(heads=H, p_out=_t(NNZ - 1, H)), dict(heads=H, p_out=_t(H, NNZ).t()),
               dict(heads=H, p_out=_t(NNZ, H), out_pos=torch.zeros(NNZ - 1, dtype=torch.int32)),
               dict(heads=H, out_pos=torch.zeros(NNZ, dtype=torch.int32))):
        with pytest.raises(ValueError):
            att(**kw)
    # heads = 1: the single-head checks, unchanged -- a 2-D lse is refused, a 1-D one is taken (and then found on the host)
    with pytest.raises(ValueError):
        att(heads=1, lse=_t(M, 1))
    with pytest.raises(TypeError):
        att(heads=1, lse=torch.zeros(M, dtype=torch.float64))


def test_bwd_q_refuses_before_the_library(crp):
    import torch
    from crp_spmm_amd import hip
    h = _Handle()
    good = dict(Q=_t(M, N), K0=_t(K, N), V0=_t(K, NV), O=_t(M, NV), dO=_t(M, NV), lse=_t(M, H))

    def call(**kw):
        a = dict(good, **kw)
        pos = [a.pop(k) for k in ("Q", "K0", "V0", "O", "dO", "lse")]
        return hip.CsrDev.attention_bwd_q(h, *pos, **a)
    _bad_heads(call)
    with pytest.raises(TypeError):
        call(heads=H, delta=_t(M, H), ds_out=_t(NNZ, H))                        # well-formed, but on the host
    with pytest.raises(TypeError):
        call(heads=H, delta=_t(M, H, torch.float32))
    v = lambda n: torch.zeros(n, dtype=torch.float64)
    for kw in (dict(heads=3), dict(heads=4), dict(heads=H, lse=v(M * H)), dict(heads=H, lse=_t(M, H + 1)), dict(heads=H, lse=_t(M - 1, H)),
               dict(heads=H, lse=_t(H, M).t()), dict(heads=H, delta=v(M * H)), dict(heads=H, delta=_t(M, 1)), dict(heads=H, delta=_t(M - 1, H)),
               dict(heads=H, ds_out=v(NNZ * H)), dict(heads=H, ds_out=_t(NNZ, H + 1)), dict(heads=H, ds_out=_t(NNZ - 1, H)),
               dict(heads=H, ds_out=_t(NNZ, 2 * H)[:, ::2]), dict(heads=H, out_pos=torch.zeros(NNZ, dtype=torch.int32)),
               dict(heads=H, ds_out=_t(NNZ, H), out_pos=torch.zeros(NNZ + 1, dtype=torch.int32)),
               # the cap is per head: 2 x 513 is refused, as 1 x 513 is; 2 x 512 passes the checks and ends at the host tensors
               dict(heads=2, Q=_t(M, 1026), K0=_t(K, 1026)), dict(heads=2, V0=_t(K, 1026), O=_t(M, 1026), dO=_t(M, 1026))):
        with pytest.raises(ValueError):
            call(**kw)
    with pytest.raises(TypeError):
        call(heads=2, Q=_t(M, 1024), K0=_t(K, 1024))
    with pytest.raises(ValueError):
        call(heads=1, lse=v(M), Q=_t(M, 1024), K0=_t(K, 1024))
    with pytest.raises(ValueError):
        call(heads=1)                                                           # (a 2-D lse with one head)


def test_bwd_kv_refuses_before_the_library(crp):
    import torch
    from crp_spmm_amd import hip
    h = _Handle()                                               # as a handle of A^T: M rows (K, V), K columns (Q, dO)
    good = dict(K=_t(M, N), V=_t(M, NV), Q=_t(K, N), dO=_t(K, NV), lse=_t(K, H), delta=_t(K, H))

    def call(**kw):
        a = dict(good, **kw)
        pos = [a.pop(k) for k in ("K", "V", "Q", "dO", "lse", "delta")]
        return hip.CsrDev.attention_bwd_kv(h, *pos, **a)
    _bad_heads(call)
    with pytest.raises(TypeError):
        call(heads=H)                                                           # well-formed, but on the host
    v = lambda n: torch.zeros(n, dtype=torch.float64)
    for kw in (dict(heads=3), dict(heads=4), dict(heads=H, lse=v(K * H)), dict(heads=H, lse=_t(K, H + 1)), dict(heads=H, lse=_t(K - 1, H)),
               dict(heads=H, delta=v(K * H)), dict(heads=H, delta=_t(K - 1, H)), dict(heads=H, delta=_t(H, K).t()),
               dict(heads=2, K=_t(M, 1026), Q=_t(K, 1026)), dict(heads=1)):
        with pytest.raises(ValueError):
            call(**kw)


def test_sparse_attention_refuses_bad_heads(crp):
    from crp_spmm_amd import hip

    class At(_Handle):
        nrow, ncol = K, M
    for heads, exc in ((0, ValueError), (-2, ValueError), (1.5, TypeError), (3, ValueError)):
        with pytest.raises(exc):
            hip.sparse_attention(_Handle(), At(), _t(M, N), _t(K, N), _t(K, NV), heads=heads)


def test_engine_wrappers_refuse_before_any_library_call(crp, monkeypatch):
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
        assert not [c for c in called if c.startswith("crp_rp_spmm_attention")], called
        monkeypatch.undo()
        assert e.attention_built() is False and e.attention_bwd_built() is False
        e.free()
        sc.free()
    z = lambda r, c: np.zeros((r, c))
    fwd = lambda **kw: (lambda e, nnz: e.attention(0, z(EM, EN), z(EK, EN), z(EK, EN), z(EM, EN),
                                                   **{k: (v(nnz) if callable(v) else v) for k, v in kw.items()}))
    for exc, kw in ((ValueError, dict(heads=0)), (ValueError, dict(heads=-1)), (ValueError, dict(heads=3)), (ValueError, dict(heads=16)),
                    (TypeError, dict(heads=2.0)), (TypeError, dict(heads=True)),
                    (ValueError, dict(heads=2, lse=np.zeros(EM * 2))), (ValueError, dict(heads=2, lse=z(EM, 3))),
                    (ValueError, dict(heads=2, lse=z(EM - 1, 2))), (ValueError, dict(heads=2, lse=z(2, EM).T)),
                    (TypeError, dict(heads=2, lse=z(EM, 2).astype(np.float32))),
                    (ValueError, dict(heads=2, p_out=lambda nnz: np.zeros(nnz * 2))), (ValueError, dict(heads=2, p_out=lambda nnz: z(nnz, 4))),
                    (ValueError, dict(heads=2, p_out=lambda nnz: z(nnz - 1, 2))),
                    (ValueError, dict(heads=2, lse=torch.zeros((EM, 2), dtype=torch.float64)[:, :1]))):
        refused(exc, fwd(**kw))
    t = lambda r, c: torch.zeros((r, c), dtype=torch.float64)

    def bwd(**kw):
        a = dict(dict(Q=t(EM, EN), K=t(EK, EN), V=t(EK, EN), O=t(EM, EN), dO=t(EM, EN), lse=t(EM, 2), dQ=t(EM, EN), dK=t(EK, EN),
                      dV=t(EK, EN), heads=2), **kw)
        extra = {k: a.pop(k) for k in list(a) if k in ("heads", "ds_out")}
        return lambda e, nnz: e.attention_bwd(a["Q"], a["K"], a["V"], a["O"], a["dO"], a["lse"], a["dQ"], a["dK"], a["dV"],
                                              **{k: (v(nnz) if callable(v) else v) for k, v in extra.items()})
    for exc, kw in ((ValueError, dict(heads=0)), (ValueError, dict(heads=3)), (TypeError, dict(heads="2")),
                    (ValueError, dict(lse=torch.zeros(EM * 2, dtype=torch.float64))), (ValueError, dict(lse=t(EM, 3))),
                    (ValueError, dict(lse=t(EM + 1, 2))), (ValueError, dict(lse=t(2, EM).t())),
                    (ValueError, dict(ds_out=lambda nnz: torch.zeros(nnz * 2, dtype=torch.float64))),
                    (ValueError, dict(ds_out=lambda nnz: t(nnz, 3))), (ValueError, dict(ds_out=lambda nnz: t(nnz - 1, 2))),
                    (ValueError, dict(heads=1)),                                # (a 2-D lse with one head)
                    (TypeError, dict(ds_out=lambda nnz: t(nnz, 2)))):           # (last: well-formed, but on the host)
        refused(exc, bwd(**kw))
