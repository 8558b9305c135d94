"""CPU: the fp32 exec's Python front door on plan-only engines (no device).  Operands of mixed or unsupported dtypes
are refused with TypeError before any C call -- a plan-only engine would abort in the library."""
import numpy as np
import pytest


def _plan_only(crp, glb_n=8):
    from crp_spmm_amd import comm, engine, gen
    rp, ci, va = gen.random_csr(40, 40, 6, seed=3)
    sc = comm.SelfComm()
    e = engine.RpSpmm(0, 40, rp, ci, va, [0, 40], glb_n, sc, plan_only=True)
    return e, sc, (rp, ci, va)


def _operands():
    import torch
    m, n = 40, 8
    return {
        "np64": np.zeros((m, n)), "np32": np.zeros((m, n), np.float32), "np16": np.zeros((m, n), np.float16),
        "npi32": np.zeros((m, n), np.int32), "t64": torch.zeros((m, n), dtype=torch.float64),
        "t32": torch.zeros((m, n), dtype=torch.float32), "tbf16": torch.zeros((m, n), dtype=torch.bfloat16),
        "t1d32": torch.zeros(m * n, dtype=torch.float32), "list": [[0.0] * n] * m,
    }


@pytest.mark.parametrize("b, c", [("np64", "np32"), ("np32", "np64"), ("t32", "t64"), ("t64", "t32"), ("np32", "t64"),
                                  ("np16", "np16"), ("npi32", "npi32"), ("tbf16", "tbf16"), ("t1d32", "t1d32"),
                                  ("t32", "tbf16"), ("list", "list"), ("np32", "np16")])
@pytest.mark.parametrize("layout", [0, 1])
def test_rp_exec_refuses_mixed_or_unsupported_dtypes(crp, monkeypatch, b, c, layout):
    e, sc, _ = _plan_only(crp)
    ops = _operands()
    called = []
    # any exec entry point fetched from the library shows up here (on a plan-only engine it would abort the process)
    monkeypatch.setattr(e, "_lib", _Spy(e._lib, called))
    with pytest.raises(TypeError):
        e.exec(layout, ops[b], ops[c])
    assert called == []
    monkeypatch.undo()
    e.free()
    sc.free()


def test_para2d_exec_refuses_mixed_dtypes(crp, monkeypatch):
    from crp_spmm_amd import comm, engine, gen
    rp, ci, va = gen.random_csr(40, 40, 6, seed=3)
    sc = comm.SelfComm()
    e2 = engine.Para2dSpmm(sc, 1, 1, [0, 40], [0, 40], [0, 40], [0, 8], rp, ci, va, plan_only=True)
    called = []
    monkeypatch.setattr(e2, "_lib", _Spy(e2._lib, called))
    ops = _operands()
    for b, c in (("np64", "np32"), ("t32", "t64"), ("np16", "np16"), ("tbf16", "tbf16")):
        with pytest.raises(TypeError):
            e2.exec(0, ops[b], ops[c])
    assert called == []
    monkeypatch.undo()
    e2.free()
    sc.free()


def test_f32_shape_checks_match_f64(crp, monkeypatch):
    """The plan's shape checks apply to float32 operands as they do to float64 ones."""
    e, sc, _ = _plan_only(crp)
    called = []
    monkeypatch.setattr(e, "_lib", _Spy(e._lib, called))
    for dt in (np.float64, np.float32):
        with pytest.raises(ValueError):
            e.exec(0, np.zeros((40, 7), dt), np.zeros((40, 8), dt))      # B one column short
        with pytest.raises(ValueError):
            e.exec(0, np.zeros((40, 8), dt), np.zeros((39, 8), dt))      # C one row short
        with pytest.raises(ValueError):
            e.exec(1, np.zeros((8, 39), dt), np.zeros((8, 40), dt))      # column-major B one row short
    assert called == []
    monkeypatch.undo()
    e.free()
    sc.free()


def test_set_variant_f32_and_alg_bytes_f32(crp):
    e, sc, (rp, ci, va) = _plan_only(crp, glb_n=24)
    for v in (0, 1, 5):
        e.set_variant_f32(v)
    for v in (2, 3, 7, -1):
        with pytest.raises(ValueError):
            e.set_variant_f32(v)
    nnz, m, n = int(rp[-1]), 40, 24
    needed = np.unique(ci).size
    assert e.alg_bytes_f32() == 8 * nnz + 4 * (m + 1) + 4 * n * needed + 4 * m * n
    assert e.alg_bytes() == 12 * nnz + 4 * (m + 1) + 8 * n * needed + 8 * m * n
    e.free()
    sc.free()


class _Spy:
    """Stands in for the library on one engine object: records every attribute fetched for a call."""

    def __init__(self, lib, called):
        self._lib, self._called = lib, called

    def __getattr__(self, name):
        if name.startswith("crp_") and "exec" in name:
            self._called.append(name)
        return getattr(self._lib, name)
