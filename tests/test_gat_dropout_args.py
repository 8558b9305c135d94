"""CPU: the attention dropout of the fused GAT and GATv2 calls without a device.  The fourteen new entry points exist with the
documented prototypes, are bound in _lib.SIGNATURES with matching ctypes and are exported; a NULL handle returns -1 whatever the
rate, and so does a bad rate on the host call; every wrapper error -- the rate, the seed, and everything the calls without
dropout refuse -- is raised before any library call.  In the style of tests/test_gat_args.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

_TAIL = "double drop, unsigned long long seed, void *stream);"
_GSRC = ("const %s *el, long long ldel, const %s *er0, long long lder0, const %s *er1, long long lder1, const %s *V0, long long ldV0, "
         "const %s *V1, long long ldV1, ")
_XSRC = "const %s *XT, long long ldXT, const %s *XS0, long long ldXS0, const %s *XS1, long long ldXS1, const %s *a, "
PROTOS = {
    "crp_gat_attention_drop_csr_%s": (8, "int crp_gat_attention_drop_csr_%s(crp_csr_dev_p A, int heads, int dv, double slope, int bias, " + _GSRC +
                                      "%s *O, long long ldO, %s *lse, %s *p_out, const int *out_pos, " + _TAIL),
    "crp_gat_attention_drop_bwd_row_csr_%s": (11, "int crp_gat_attention_drop_bwd_row_csr_%s(crp_csr_dev_p A, int heads, int dv, double slope, "
                                              "int bias, " + _GSRC + "const %s *O, long long ldO, const %s *dO, long long lddO, "
                                              "const %s *lse, %s *d_el, long long ldd_el, %s *delta, %s *ds_out, const int *out_pos, " + _TAIL),
    "crp_gat_attention_drop_bwd_col_csr_%s": (8, "int crp_gat_attention_drop_bwd_col_csr_%s(crp_csr_dev_p At, int heads, int dv, double slope, "
                                              "int bias, const %s *er, long long lder, const %s *V, long long ldV, const %s *el, "
                                              "long long ldel, const %s *dO, long long lddO, const %s *lse, const %s *delta, %s *d_er, "
                                              "long long ldd_er, %s *dV, long long lddV, " + _TAIL),
    "crp_gatv2_attention_drop_csr_%s": (7, "int crp_gatv2_attention_drop_csr_%s(crp_csr_dev_p A, int heads, int dv, double slope, int bias, " +
                                        _XSRC + "%s *O, long long ldO, %s *lse, %s *p_out, const int *out_pos, " + _TAIL),
    "crp_gatv2_attention_drop_bwd_row_csr_%s": (11, "int crp_gatv2_attention_drop_bwd_row_csr_%s(crp_csr_dev_p A, int heads, int dv, "
                                                "double slope, int bias, " + _XSRC + "const %s *O, long long ldO, const %s *dO, "
                                                "long long lddO, const %s *lse, %s *dXT, long long lddXT, %s *da_part, long long ldda, "
                                                "%s *delta, %s *ds_out, const int *out_pos, " + _TAIL),
    "crp_gatv2_attention_drop_bwd_col_csr_%s": (7, "int crp_gatv2_attention_drop_bwd_col_csr_%s(crp_csr_dev_p At, int heads, int dv, "
                                                "double slope, int bias, const %s *XS, long long ldXS, const %s *XT, long long ldXT, "
                                                "const %s *a, const %s *dO, long long lddO, const %s *lse, const %s *delta, %s *dXS, "
                                                "long long lddXS, " + _TAIL),
}
SYMBOLS = {
    "crp_dropout_keep_host": "int crp_dropout_keep_host(unsigned long long seed, unsigned r, unsigned c, unsigned h, double drop);",
    "crp_dropout_mask_csr": ("int crp_dropout_mask_csr(crp_csr_dev_p A, int heads, double drop, unsigned long long seed, "
                             "unsigned char *mask, const int *out_pos, void *stream);"),
}
for _name, (_n, _proto) in PROTOS.items():
    for _sfx, _t_ in (("f64", "double"), ("f32", "float")):
        SYMBOLS[_name % _sfx] = _proto % ((_sfx,) + (_t_,) * _n)


def _ctype_of(arg):
    arg = arg.strip()
    if "*" in arg or arg.split()[0].endswith("_p"):
        return C.c_void_p
    return {"int": C.c_int, "long long": C.c_longlong, "double": C.c_double, "unsigned long long": C.c_ulonglong,
            "unsigned": C.c_uint}[" ".join(arg.split()[:-1])]


def test_there_are_fourteen():
    assert len(SYMBOLS) == 14


@pytest.mark.parametrize("name", sorted(SYMBOLS))
def test_symbol_is_exported_declared_and_bound(crp, name):
    from crp_spmm_amd import _lib
    proto = SYMBOLS[name]
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert any(ln.split()[-1] == name and " T " in ln for ln in out.splitlines()), "%s is not exported" % name
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "crpspmm_hip.h")).read())
    assert proto in text, "%s is not declared in include/crpspmm_hip.h as documented" % name
    assert name in _lib.SIGNATURES, "%s is not bound in _lib.SIGNATURES" % name
    res, args = _lib.SIGNATURES[name]
    want = [_ctype_of(a) for a in proto[proto.index("(") + 1:proto.rindex(")")].split(",")]
    assert res == C.c_int and list(args) == want, (name, args, want)
    fn = getattr(crp.load(), name)
    assert fn.restype == res and list(fn.argtypes) == want
    if "attention_drop" in name:                       # the existing argument list with (drop, seed) before the stream
        plain = _lib.SIGNATURES[name.replace("_drop", "")][1]
        assert list(args) == list(plain[:-1]) + [C.c_double, C.c_ulonglong, C.c_void_p]


def test_a_null_handle_returns_minus_one(crp):
    """A NULL handle is refused first, whatever the rate, so no pointer is dereferenced and no device is needed; the rates that need
    a live handle to be told apart from it are pinned in the GPU tests."""
    lib = crp.load()
    buf = (C.c_double * 8)()
    p = C.addressof(buf)
    for sfx in ("f64", "f32"):
        for drop in (0.0, 0.5, float("nan"), -0.1, 1.0):
            fn = getattr(lib, "crp_gat_attention_drop_csr_" + sfx)
            assert fn(None, 2, 4, 0.2, 0, p, 2, p, 2, None, 0, p, 8, None, 0, p, 8, p, p, None, drop, 7, None) == -1
            fn = getattr(lib, "crp_gat_attention_drop_bwd_row_csr_" + sfx)
            assert fn(None, 2, 4, 0.2, 0, p, 2, p, 2, None, 0, p, 8, None, 0, p, 8, p, 8, p, p, 2, p, p, None, drop, 7, None) == -1
            fn = getattr(lib, "crp_gat_attention_drop_bwd_col_csr_" + sfx)
            assert fn(None, 2, 4, 0.2, 0, p, 2, p, 8, p, 2, p, 8, p, p, p, 2, p, 8, drop, 7, None) == -1
            fn = getattr(lib, "crp_gatv2_attention_drop_csr_" + sfx)
            assert fn(None, 2, 4, 0.2, 0, p, 8, p, 8, None, 0, p, p, 8, p, p, None, drop, 7, None) == -1
            fn = getattr(lib, "crp_gatv2_attention_drop_bwd_row_csr_" + sfx)
            assert fn(None, 2, 4, 0.2, 0, p, 8, p, 8, None, 0, p, p, 8, p, 8, p, p, 8, p, 8, p, p, None, drop, 7, None) == -1
            fn = getattr(lib, "crp_gatv2_attention_drop_bwd_col_csr_" + sfx)
            assert fn(None, 2, 4, 0.2, 0, p, 8, p, 8, p, p, 8, p, p, p, 8, drop, 7, None) == -1
    for drop in (0.0, 0.5, float("nan")):
        assert lib.crp_dropout_mask_csr(None, 1, drop, 7, p, None, None) == -1
    assert bytes(buf) == bytes(64)


def test_the_host_call_refuses_a_bad_rate(crp):
    lib = crp.load()
    for drop in (float("nan"), -0.0001, 1.0, 1.5, float("inf"), -float("inf")):
        assert lib.crp_dropout_keep_host(1, 2, 3, 0, drop) == -1
    for drop in (0.0, -0.0, 2.0 ** -40, 0.999999):
        assert lib.crp_dropout_keep_host(1, 2, 3, 0, drop) in (0, 1)
    assert lib.crp_dropout_keep_host(1, 2, 3, 0, 0.0) == 1


M, K, H, DV = 40, 36, 2, 3
NV, NNZ = H * DV, 50
BAD_RATES = ((float("nan"), ValueError), (-0.1, ValueError), (1.0, ValueError), (2, ValueError), (float("inf"), ValueError),
             ("half", TypeError), (None, TypeError))
BAD_SEEDS = ((-1, ValueError), (1 << 64, ValueError), (1.0, TypeError), ("7", TypeError), (True, TypeError), (None, TypeError))


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


def _calls():
    """name -> a call of each of the six wrappers with well-formed host operands (which is what ends it: TypeError, on the host)"""
    from crp_spmm_amd import hip
    h = _Handle()
    a = _t(H, DV)
    return {
        "gat_attention": lambda **kw: hip.CsrDev.gat_attention(h, _t(M, H), _t(K, H), _t(K, NV), heads=H, **kw),
        "gat_attention_bwd_row": lambda **kw: hip.CsrDev.gat_attention_bwd_row(h, _t(M, H), _t(K, H), _t(K, NV), _t(M, NV), _t(M, NV), _t(M, H),
                                                                               heads=H, **kw),
        "gat_attention_bwd_col": lambda **kw: hip.CsrDev.gat_attention_bwd_col(h, _t(M, H), _t(M, NV), _t(K, H), _t(K, NV), _t(K, H), _t(K, H),
                                                                               heads=H, **kw),
        "gatv2_attention": lambda **kw: hip.CsrDev.gatv2_attention(h, _t(M, NV), _t(K, NV), a, heads=H, **kw),
        "gatv2_attention_bwd_row": lambda **kw: hip.CsrDev.gatv2_attention_bwd_row(h, _t(M, NV), _t(K, NV), a, _t(M, NV), _t(M, NV), _t(M, H),
                                                                                   heads=H, **kw),
        "gatv2_attention_bwd_col": lambda **kw: hip.CsrDev.gatv2_attention_bwd_col(h, _t(M, NV), _t(K, NV), a, _t(K, NV), _t(K, H), _t(K, H),
                                                                                   heads=H, **kw),
    }


@pytest.mark.parametrize("name", ["gat_attention", "gat_attention_bwd_row", "gat_attention_bwd_col", "gatv2_attention",
                                  "gatv2_attention_bwd_row", "gatv2_attention_bwd_col"])
def test_wrapper_refuses_before_the_library(crp, name):
    call = _calls()[name]
    for rate, exc in BAD_RATES:
        with pytest.raises(exc):
            call(dropout=rate, seed=1)
    for seed, exc in BAD_SEEDS:
        with pytest.raises(exc):
            call(dropout=0.5, seed=seed)
        with pytest.raises(exc):
            call(dropout=0.0, seed=seed)                # the seed is checked whatever the rate
    # a good rate and seed pass on to the checks of the call without dropout: the operands are on the host
    for kw in (dict(), dict(dropout=0.0), dict(dropout=0.6, seed=(1 << 64) - 1), dict(dropout=np.float32(0.5), seed=np.int64(3))):
        with pytest.raises(TypeError, match="on the device"):
            call(**kw)
    # ... and what that call refuses is refused under dropout too
    with pytest.raises(ValueError):
        call(dropout=0.5, seed=1, slope=float("nan"))
    with pytest.raises(ValueError):
        call(dropout=0.5, seed=1, bias=2)


def test_dropout_mask_refuses_before_the_library(crp):
    import torch
    from crp_spmm_amd import hip
    h = _Handle()
    for rate, exc in BAD_RATES:
        with pytest.raises(exc):
            hip.CsrDev.dropout_mask(h, H, rate, 1)
    for seed, exc in BAD_SEEDS:
        with pytest.raises(exc):
            hip.CsrDev.dropout_mask(h, H, 0.5, seed)
    for heads, exc in ((0, ValueError), (-1, ValueError), (2.0, TypeError), (True, TypeError)):
        with pytest.raises(exc):
            hip.CsrDev.dropout_mask(h, heads, 0.5, 1)
    u8 = lambda *s: torch.zeros(s, dtype=torch.uint8)
    for out in (torch.zeros((NNZ, H)), np.zeros((NNZ, H), np.uint8), u8(NNZ, 2 * H)[:, ::2], u8(NNZ, H)):     # (last: on the host)
        with pytest.raises(TypeError):
            hip.CsrDev.dropout_mask(h, H, 0.5, 1, out=out)
    with pytest.raises(ValueError):
        hip.CsrDev.dropout_mask(h, H, 0.5, 1, out_pos=torch.zeros(NNZ, dtype=torch.int32))      # out_pos needs an out


def test_the_functions_refuse_before_the_library(crp):
    from crp_spmm_amd import hip

    class At(_Handle):
        nrow, ncol = K, M
    for rate, exc in BAD_RATES:
        with pytest.raises(exc):
            hip.gat_attention(_Handle(), At(), _t(M, H), _t(K, H), _t(K, NV), heads=H, dropout=rate)
        with pytest.raises(exc):
            hip.gatv2_attention(_Handle(), At(), _t(M, NV), _t(K, NV), _t(H, DV), heads=H, dropout=rate, seed=3)
    for seed, exc in BAD_SEEDS[:-1]:                    # (None is "draw one")
        with pytest.raises(exc):
            hip.gat_attention(_Handle(), At(), _t(M, H), _t(K, H), _t(K, NV), heads=H, dropout=0.5, seed=seed)
    for rate, exc in BAD_RATES:
        with pytest.raises(exc):
            hip.dropout_keep(1, 2, 3, 0, rate)
    with pytest.raises(ValueError):
        hip.dropout_keep(-1, 2, 3, 0, 0.5)
