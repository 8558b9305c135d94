"""Host path of crp_csr_transpose (include/crpspmm_hip.h) against numpy: A^T as a stable sort of the nonzeros by
column.  No GPU needed; the device path is checked against this one in tests/test_gpu_transpose.py."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def numpy_transpose(rp, ci, va, ncol):
    """the definition: order = stable argsort of the columns; -> (rowptr_t, colidx_t, val_t, tmap)"""
    rp, ci = np.asarray(rp, np.int32), np.asarray(ci, np.int32)
    order = np.argsort(ci, kind="stable")
    rows = np.repeat(np.arange(rp.size - 1, dtype=np.int32), np.diff(rp))
    rowptr_t = np.concatenate([[0], np.cumsum(np.bincount(ci, minlength=ncol))]).astype(np.int32)
    return rowptr_t, rows[order].astype(np.int32), np.asarray(va, np.float64)[order], order.astype(np.int32)


def _handmade():
    """duplicate (row, column) pairs, unsorted columns, an empty row"""
    rp = np.array([0, 5, 5, 9, 12], np.int32)
    ci = np.array([3, 1, 3, 0, 1, 2, 2, 0, 2, 4, 1, 4], np.int32)
    va = np.arange(1, 13, dtype=np.float64) * 0.5
    return rp, ci, va, 5


def _empty_tail():
    """no entry in the last columns: rowptr_t ends in a run of equal offsets"""
    rp = np.array([0, 2, 3, 3, 6], np.int32)
    ci = np.array([1, 0, 2, 2, 0, 1], np.int32)
    return rp, ci, np.linspace(-1, 1, 6), 9


def _cases(gen):
    rp, ci, va = gen.random_csr(3000, 1700, 40, empty_every=13)
    yield "random_csr", rp, ci, va, 1700
    rp, ci, va = gen.kkt3d(9)
    yield "kkt3d", rp, ci, va, rp.size - 1
    yield ("handmade",) + _handmade()
    yield ("empty_tail",) + _empty_tail()
    yield "0xk", np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0), 7
    yield "mx0", np.zeros(6, np.int32), np.zeros(0, np.int32), np.zeros(0), 0
    yield "nnz0", np.zeros(5, np.int32), np.zeros(0, np.int32), np.zeros(0), 3


def test_host_transpose_matches_numpy(crp):
    from crp_spmm_amd import gen, hip
    seen = 0
    for name, rp, ci, va, ncol in _cases(gen):
        got = hip.csr_transpose(rp, ci, va, ncol)
        want = numpy_transpose(rp, ci, va, ncol)
        for what, g, w in zip(("rowptr_t", "colidx_t", "val_t", "tmap"), got, want):
            assert g.dtype == w.dtype, (name, what, g.dtype, w.dtype)
            assert g.shape == w.shape and np.array_equal(g, w), (name, what)
        assert np.array_equal(got[2], np.asarray(va, np.float64)[got[3]]), name      # val_t[q] = val[tmap[q]]
        seen += 1
    assert seen == 7


def test_transpose_twice_returns_the_input_in_column_order(crp):
    from crp_spmm_amd import gen, hip
    for name, rp, ci, va, ncol in _cases(gen):
        nrow = rp.size - 1
        rp1, ci1, va1, _ = hip.csr_transpose(rp, ci, va, ncol)
        rp2, ci2, va2, _ = hip.csr_transpose(rp1, ci1, va1, nrow)
        # the input with the columns of every row in stable ascending order
        rows = np.repeat(np.arange(nrow), np.diff(rp))
        order = np.lexsort((np.arange(ci.size), ci, rows))
        assert np.array_equal(rp2, np.asarray(rp, np.int32)), name
        assert np.array_equal(ci2, np.asarray(ci, np.int32)[order]), name
        assert np.array_equal(va2, np.asarray(va, np.float64)[order]), name


def _raw(lib, nrow, ncol, rp, ci, va, rp_t, ci_t, va_t, tmap):
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)       # noqa: E731
    return lib.crp_csr_transpose(nrow, ncol, p(rp), p(ci), p(va), p(rp_t), p(ci_t), p(va_t), p(tmap), None)


@pytest.mark.parametrize("case", ["negative column", "column >= ncol", "rowptr[0] != 0", "decreasing rowptr", "NULL output"])
def test_bad_input_returns_its_code_and_writes_nothing(crp, case):
    from crp_spmm_amd import _lib, hip
    lib = _lib.load()
    rp, ci, va, ncol = _handmade()
    rp, ci = rp.copy(), ci.copy()
    nrow = rp.size - 1
    want = {"negative column": hip.T_ECOL, "column >= ncol": hip.T_ECOL, "rowptr[0] != 0": hip.T_EPTR,
            "decreasing rowptr": hip.T_EPTR, "NULL output": hip.T_EARG}[case]
    if case == "negative column":
        ci[4] = ~2                                   # the two-source encoding is refused
    elif case == "column >= ncol":
        ci[7] = ncol
    elif case == "rowptr[0] != 0":
        rp[0] = 1
    elif case == "decreasing rowptr":
        rp[2] = 4
    SENT = -77
    rp_t = np.full(ncol + 1, SENT, np.int32)
    ci_t = np.full(ci.size, SENT, np.int32)
    va_t = np.full(ci.size, float(SENT))
    tmap = np.full(ci.size, SENT, np.int32)
    rc = _raw(lib, nrow, ncol, rp, ci, va, None if case == "NULL output" else rp_t, ci_t, va_t, tmap)
    assert rc == want, (case, rc)
    assert (ci_t == SENT).all() and (va_t == SENT).all() and (tmap == SENT).all(), case
    # the codes are the header's named constants
    hdr = open(os.path.join(ROOT, "include", "crpspmm_hip.h")).read()
    for nm, code in (("EARG", hip.T_EARG), ("ECOL", hip.T_ECOL), ("EPTR", hip.T_EPTR), ("EMIXED", hip.T_EMIXED)):
        assert "#define CRP_CSR_T_%s" % nm in hdr and "(%d)" % code in hdr.split("#define CRP_CSR_T_%s" % nm)[1].split("\n")[0]
    # the Python wrapper raises with the same code
    if case != "NULL output":
        with pytest.raises(hip.TransposeError) as ei:
            hip.csr_transpose(rp, ci, va, ncol)
        assert ei.value.code == want


def test_a_missing_colidx_output_is_an_argument_error(crp):
    from crp_spmm_amd import _lib, hip
    rp, ci, va, ncol = _handmade()
    rp_t = np.zeros(ncol + 1, np.int32)
    assert _raw(_lib.load(), rp.size - 1, ncol, rp, ci, va, rp_t, None, None, None) == hip.T_EARG


def test_values_and_map_are_optional(crp):
    from crp_spmm_amd import _lib
    rp, ci, va, ncol = _handmade()
    want = numpy_transpose(rp, ci, va, ncol)
    rp_t, ci_t = np.zeros(ncol + 1, np.int32), np.zeros(ci.size, np.int32)
    assert _raw(_lib.load(), rp.size - 1, ncol, rp, ci, None, rp_t, ci_t, None, None) == 0
    assert np.array_equal(rp_t, want[0]) and np.array_equal(ci_t, want[1])


def test_exec_t_refuses_fp32_operands_before_any_c_call(crp):
    """RpSpmm.exec_t is fp64 only (no engine needed: the dtype check comes first)."""
    from crp_spmm_amd import engine
    e = engine.RpSpmm.__new__(engine.RpSpmm)
    e.handle, e._owned = None, False
    B = np.zeros((4, 8), np.float32)
    with pytest.raises(TypeError):
        e.exec_t(0, B, np.zeros((4, 8), np.float32))
    with pytest.raises(TypeError):
        e.exec_t(0, B.astype(np.float64), np.zeros((4, 8), np.float32))
