"""CPU: the sampled dense-dense product (SDDMM) without a device.  The four entry points exist with the documented
signatures; the Python wrappers refuse mixed dtypes, wrong shapes and a short `out` before any library call (a plan-only
engine, or a handle without a device, would abort or fault in the library); the engine's data flow, replayed in numpy from
the plans of 2 and 4 ranks (tests/dist_sddmm_worker.py), equals the global SDDMM entry for entry."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

SYMBOLS = {
    # name -> (header, the prototype as documented, ctypes result and arguments)
    "crp_sddmm_csr_f64": ("crpspmm_hip.h",
                          "int crp_sddmm_csr_f64(crp_csr_dev_p A, int n, const double *X, long long ldX, const double *Y0, long long ldY0, "
                          "const double *Y1, long long ldY1, double *out, const int *out_pos, int mode, void *stream);"),
    "crp_sddmm_csr_f32": ("crpspmm_hip.h",
                          "int crp_sddmm_csr_f32(crp_csr_dev_p A, int n, const float *X, long long ldX, const float *Y0, long long ldY0, "
                          "const float *Y1, long long ldY1, float *out, const int *out_pos, int mode, void *stream);"),
    "crp_rp_spmm_sddmm_ex": ("crp_engine.h",
                             "void crp_rp_spmm_sddmm_ex(crp_rp_spmm_p rp_spmm, int layout, const double *X, long long ldX, "
                             "const double *Y, long long ldY, double *out, int mode, void *stream);"),
    "crp_rp_spmm_sddmm_f32_ex": ("crp_engine.h",
                                 "void crp_rp_spmm_sddmm_f32_ex(crp_rp_spmm_p rp_spmm, int layout, const float *X, long long ldX, "
                                 "const float *Y, long long ldY, float *out, int mode, void *stream);"),
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
    res, args = _lib.SIGNATURES[name]
    want = [_ctype_of(a) for a in proto[proto.index("(") + 1:proto.rindex(")")].split(",")]
    assert res == (C.c_int if proto.startswith("int ") else None), name
    assert list(args) == want, (name, args, want)
    fn = getattr(crp.load(), name)
    assert fn.restype == res and list(fn.argtypes) == want


class _Spy:
    """Stands in for the library on one object: records every SDDMM entry point fetched for a call."""

    def __init__(self, lib, called):
        self._lib, self._called = lib, called

    def __getattr__(self, name):
        if name.startswith("crp_") and "sddmm" in name and not name.endswith("built"):
            self._called.append(name)
        return getattr(self._lib, name)


M, K, N = 40, 40, 8


def _plan_only(crp):
    from crp_spmm_amd import comm, engine, gen
    rp, ci, va = gen.random_csr(M, K, 6, seed=3)
    sc = comm.SelfComm()
    e = engine.RpSpmm(0, M, rp, ci, va, [0, K], N, sc, plan_only=True)
    return e, sc, int(rp[-1])


def _refused(crp, monkeypatch, exc, call):
    e, sc, nnz = _plan_only(crp)
    called = []
    monkeypatch.setattr(e, "_lib", _Spy(e._lib, called))
    with pytest.raises(exc):
        call(e, nnz)
    assert called == []
    monkeypatch.undo()
    e.free()
    sc.free()


@pytest.mark.parametrize("x, y, o", [("f8", "f4", "f8"), ("f4", "f8", "f4"), ("f8", "f8", "f4"), ("f4", "f4", "f8"),
                                     ("f2", "f2", "f2"), ("i4", "i4", "i4")])
@pytest.mark.parametrize("layout", [0, 1])
def test_rp_sddmm_refuses_mixed_or_unsupported_dtypes(crp, monkeypatch, x, y, o, layout):
    shape = (M, N) if layout == 0 else (N, M)
    _refused(crp, monkeypatch, TypeError,
             lambda e, nnz: e.sddmm(layout, np.zeros(shape, x), np.zeros(shape, y), np.zeros(nnz, o)))


def test_rp_sddmm_refuses_mixed_torch_dtypes_and_non_arrays(crp, monkeypatch):
    import torch
    for x, y, o in ((torch.float64, torch.float32, torch.float64), (torch.float32, torch.float32, torch.float64),
                    (torch.bfloat16, torch.bfloat16, torch.bfloat16)):
        _refused(crp, monkeypatch, TypeError,
                 lambda e, nnz: e.sddmm(0, torch.zeros((M, N), dtype=x), torch.zeros((K, N), dtype=y), torch.zeros(nnz, dtype=o)))
    _refused(crp, monkeypatch, TypeError, lambda e, nnz: e.sddmm(0, [[0.0] * N] * M, [[0.0] * N] * K, [0.0] * nnz))
    _refused(crp, monkeypatch, TypeError, lambda e, nnz: e.sddmm(0, np.zeros((M, N)), np.zeros((K, N)), np.zeros((nnz, 1))))


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_rp_sddmm_refuses_wrong_shapes_and_out_length(crp, monkeypatch, dt):
    bad = [
        lambda e, nnz: e.sddmm(0, np.zeros((M, N - 1), dt), np.zeros((K, N), dt), np.zeros(nnz, dt)),      # X a column short
        lambda e, nnz: e.sddmm(0, np.zeros((M - 1, N), dt), np.zeros((K, N), dt), np.zeros(nnz, dt)),      # X a row short
        lambda e, nnz: e.sddmm(0, np.zeros((M, N), dt), np.zeros((K - 1, N), dt), np.zeros(nnz, dt)),      # Y a row short
        lambda e, nnz: e.sddmm(0, np.zeros((M, N), dt), np.zeros((K, N + 1), dt), np.zeros(nnz, dt)),      # Y a column wide
        lambda e, nnz: e.sddmm(1, np.zeros((N, M - 1), dt), np.zeros((N, K), dt), np.zeros(nnz, dt)),      # column-major X a row short
        lambda e, nnz: e.sddmm(1, np.zeros((N, M), dt), np.zeros((N + 1, K), dt), np.zeros(nnz, dt)),
        lambda e, nnz: e.sddmm(0, np.zeros((M, N), dt), np.zeros((K, N), dt), np.zeros(nnz - 1, dt)),      # out short
        lambda e, nnz: e.sddmm(0, np.zeros((M, N), dt), np.zeros((K, N), dt), np.zeros(nnz + 1, dt)),      # out long
        lambda e, nnz: e.sddmm(0, np.zeros((M, N), dt), np.zeros((K, N), dt), np.zeros(2 * nnz, dt)[::2]),  # out strided
        lambda e, nnz: e.sddmm(0, np.zeros((M, N), dt), np.zeros((K, N), dt), np.zeros(nnz, dt), mode=2),
    ]
    for call in bad:
        _refused(crp, monkeypatch, ValueError, call)


class _NoDevice:
    """A CsrDev of given sizes without a device behind it: every check of ``sddmm`` runs, the library must not."""

    def __new__(cls, crp, nrow, ncol, nnz, called):
        from crp_spmm_amd import hip

        class Fake(hip.CsrDev):
            def __init__(self):
                pass

            def free(self):
                pass
        Fake.nnz = nnz
        a = Fake()
        a.nrow, a.ncol, a.handle = nrow, ncol, None
        a._lib = _Spy(crp.load(), called)
        return a


def test_csrdev_sddmm_refuses_before_the_library(crp):
    import torch
    called = []
    nnz = 50
    A = _NoDevice(crp, M, K, nnz, called)
    f64, f32 = torch.float64, torch.float32
    z = lambda shape, dt=f64: torch.zeros(shape, dtype=dt)
    with pytest.raises(TypeError):                                  # mixed dtypes
        A.sddmm(z((M, N)), z((K, N), f32), out=z(nnz))
    with pytest.raises(TypeError):
        A.sddmm(z((M, N)), z((K, N)), Y1=z((3, N), f32), out=z(nnz))
    with pytest.raises(TypeError):
        A.sddmm(z((M, N), f32), z((K, N), f32), out=z(nnz))
    with pytest.raises(TypeError):
        A.sddmm(z((M, N), torch.float16), z((K, N), torch.float16), out=z(nnz, torch.float16))
    with pytest.raises(TypeError):
        A.sddmm(np.zeros((M, N)), np.zeros((K, N)), out=np.zeros(nnz))
    with pytest.raises(ValueError):                                 # wrong shapes
        A.sddmm(z((M, N)), z((K, N + 1)), out=z(nnz))
    with pytest.raises(ValueError):
        A.sddmm(z((M, N)), z((K, N)), Y1=z((3, N - 1)), out=z(nnz))
    with pytest.raises(ValueError):
        A.sddmm(z((M - 1, N)), z((K, N)), out=z(nnz))
    with pytest.raises(ValueError):
        A.sddmm(z((M, N)), z((K - 1, N)), out=z(nnz))
    with pytest.raises(ValueError):
        A.sddmm(z((M, 0)), z((K, 0)), out=z(nnz))
    with pytest.raises(ValueError):                                 # a short out, a short out_pos, out_pos without out
        A.sddmm(z((M, N)), z((K, N)), out=z(nnz - 1))
    with pytest.raises(ValueError):
        A.sddmm(z((M, N)), z((K, N)), out=z(nnz), out_pos=torch.zeros(nnz - 1, dtype=torch.int32))
    with pytest.raises(ValueError):
        A.sddmm(z((M, N)), z((K, N)), out_pos=torch.zeros(nnz, dtype=torch.int32))
    with pytest.raises(TypeError):
        A.sddmm(z((M, N)), z((K, N)), out=z(nnz), out_pos=torch.zeros(nnz, dtype=torch.int64))
    with pytest.raises(ValueError):
        A.sddmm(z((M, N)), z((K, N)), out=z(nnz), mode=3)
    with pytest.raises(TypeError, match="on the device"):          # all of it right, but host memory: device pointers only
        A.sddmm(z((M, N)), z((K, N)), out=z(nnz))
    assert called == []


@pytest.mark.parametrize("world", [2, 4])
def test_engine_data_flow_replayed_in_numpy(world):
    env = dict(os.environ)
    env.pop("RP_SPMM_REIDX", None)
    env["OMP_NUM_THREADS"] = "1"
    # the ranks neither see nor open a GPU, also on a machine that has one (tests/test_dist_cpu.py)
    env["HIP_VISIBLE_DEVICES"] = "-1"
    env["GPU_ENABLE_PAL"] = "1"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world),
           "--master-addr", "127.0.0.1", "--master-port", str(29640 + world), os.path.join(ROOT, "tests", "dist_sddmm_worker.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "DIST_SDDMM_WORKER_OK world=%d" % world in r.stdout
