"""CPU: the oracle (oracle/crp_oracle.c + numpy) against the golden vectors
produced by the reference's own code (oracle/_ref) and by MKL, against _ref
itself when it is present, and against closed forms."""
import hashlib
import os

import numpy as np
import pytest

from conftest import GOLDEN, GOLDEN_NAMES, load_golden

PS = (1, 2, 3, 4, 6, 8)
NS = (1, 4, 64, 128, 512)


@pytest.mark.parametrize("name", GOLDEN_NAMES)
def test_ingest_matches_reference_golden(orc, name):
    g = load_golden(name, "csr")
    m, k, rp, ci, cv, bw = orc.read_mtx_csr(os.path.join(GOLDEN, name + ".mtx"))
    assert (m, k, bw) == (int(g["m"]), int(g["k"]), int(g["bandwidth"]))
    assert np.array_equal(rp, g["rowptr"]) and np.array_equal(ci, g["colidx"])
    assert np.array_equal(cv, g["val"])          # bit-exact, duplicates in the reference's order


@pytest.mark.parametrize("name", GOLDEN_NAMES)
def test_planner_matches_reference_golden(orc, name):
    g, p = load_golden(name, "csr"), load_golden(name, "plan")
    m, k = int(g["m"]), int(g["k"])
    for P in PS:
        rb = orc.csr_row_partition(g["rowptr"], P)
        assert np.array_equal(rb, p["rb_P%d" % P])
        for n in NS:
            r = orc.part2d_from_1d(P, m, n, k, rb, g["rowptr"], g["colidx"])
            key = "P%d_n%d_" % (P, n)
            assert [r["pm"], r["pn"]] == list(p[key + "grid"])
            assert r["comm_cost"] == int(p[key + "cost"][0])
            for a in ("A0_rowptr", "B_rowptr", "AC_rowptr", "BC_colptr"):
                assert np.array_equal(r[a], p[key + a]), (P, n, a)


@pytest.mark.parametrize("name", GOLDEN_NAMES)
def test_spmm_matches_mkl_golden(orc, name):
    g, s = load_golden(name, "csr"), load_golden(name, "spmm")
    k, m = int(g["k"]), int(g["m"])
    for n in (4, 33):
        c = orc.spmm_csr(g["rowptr"], g["colidx"], g["val"], orc.fill_B(0, k, 0, n))
        assert orc.rel_fro_err(s["C_fillB_n%d" % n], c) <= 1e-14
    c = orc.spmm_csr(g["rowptr"], g["colidx"], g["val"], s["B2"])
    assert orc.rel_fro_err(s["C_B2"], c) <= 1e-14
    Bc = np.zeros((5, k + 3))
    Bc[:, :k] = orc.fill_B(0, k, 0, 5).T
    cc = orc.spmm_csr(g["rowptr"], g["colidx"], g["val"], Bc, n=5, layout=1, ldB=k + 3, ldC=m + 2)
    assert orc.rel_fro_err(s["C_fillB_colmajor_n5"], cc) <= 1e-14


def test_spmm_closed_form(orc):
    """B = fill_B(fi, fj) gives C[i][j] = fi * sum(val*col) + fj * j * sum(val): an
    answer that does not come from any SpMM code (harness: examples/test_utils.c:121-154)."""
    from crp_spmm_amd import gen
    rp, ci, va = gen.random_csr(500, 700, 20, seed=11, empty_every=9)
    n = 12
    c = orc.spmm_csr(rp, ci, va, orc.fill_B(0, 700, 0, n))
    rows = np.repeat(np.arange(500), np.diff(rp))
    s1 = np.bincount(rows, weights=va * ci, minlength=500)
    s0 = np.bincount(rows, weights=va, minlength=500)
    expect = 0.19 * s1[:, None] + 0.24 * np.arange(n)[None, :] * s0[:, None]
    assert np.abs(c - expect).max() <= 1e-9 * max(1.0, np.abs(expect).max())
    assert not c[::9].any()                    # empty rows give exact zeros (beta = 0)


def test_restatement_matches_compiled_reference(orc):
    """Restatement == reference on seeded random inputs: against the reference's answers stored in
    tests/golden/ref_random.npz (make_golden_random.py), and against oracle/_ref itself when it is built."""
    from crp_spmm_amd import gen
    g = np.load(os.path.join(GOLDEN, "ref_random.npz"), allow_pickle=False)
    live = orc.ref() is not None
    for seed, (m, k) in enumerate([(900, 900), (400, 1300), (1300, 400)]):
        rp, ci, va = gen.random_csr(m, k, 15, seed=seed, empty_every=13 if seed else 0)
        sha = hashlib.sha256(rp.astype(np.int32).tobytes() + ci.astype(np.int32).tobytes() + va.astype(np.float64).tobytes())
        assert sha.hexdigest() == str(g["s%d_input_sha256" % seed]), "gen.random_csr changed: regenerate ref_random.npz"
        for P in (1, 2, 3, 5, 6, 8, 12):
            t = "s%d_P%d_" % (seed, P)
            a = orc.csr_row_partition(rp, P)
            assert np.array_equal(a, g[t + "rb"])
            if live:
                assert np.array_equal(a, orc.csr_row_partition(rp, P, use_ref=True))
            x = orc.even_displs(k, P) if m != k else a
            s1, t1 = orc.csr_row_part_comm_size(k, rp, ci, a, x)
            assert np.array_equal(s1, g[t + "comm_sizes"]) and t1 == int(g[t + "comm_total"]), (seed, P)
            if live:
                s2, t2 = orc.csr_row_part_comm_size(k, rp, ci, a, x, use_ref=True)
                assert np.array_equal(s1, s2) and t1 == t2
            for n in (1, 16, 256, 2048):
                r1 = orc.part2d_from_1d(P, m, n, k, a, rp, ci)
                r2 = orc.part2d_from_1d(P, m, n, k, a, rp, ci, use_ref=True) if live else None
                for key in r1:
                    assert np.array_equal(np.asarray(r1[key]), g["%sn%d_%s" % (t, n, key)]), (seed, P, n, key)
                    if live:
                        assert np.array_equal(np.asarray(r1[key]), np.asarray(r2[key])), (P, n, key)
        assert orc.prime_factorization(360) == list(g["prime_360"]) == [2, 2, 2, 3, 3, 5]
        if live:
            assert orc.prime_factorization(360, use_ref=True) == [2, 2, 2, 3, 3, 5]
        rows = np.repeat(np.arange(m), np.diff(rp)).astype(np.int32)
        perm = np.random.default_rng(seed).permutation(rows.size)
        o = orc.coo2csr(m, rows[perm], ci[perm], va[perm])
        order = g["s%d_coo2csr_order" % seed]
        want = (g["s%d_coo2csr_rowptr" % seed], ci[perm][order], va[perm][order])
        assert all(np.array_equal(u, v) for u, v in zip(o, want)), seed
        if live:
            r = orc.coo2csr(m, rows[perm], ci[perm], va[perm], use_ref=True)
            assert all(np.array_equal(u, v) for u, v in zip(o, r))
    spos = [tuple(int(x) for x in row) for row in g["block_spos"]]
    assert [row[:3] for row in spos] == [(length, nblk, i) for length, nblk in [(10, 3), (7, 7), (5, 8), (0, 2)]
                                         for i in range(-1, nblk + 2)]
    for length, nblk, i, s, z in spos:
        assert orc.block_spos(length, nblk, i) == (s, z), (length, nblk, i)
        if live:
            assert orc.block_spos(length, nblk, i) == orc.block_spos(length, nblk, i, use_ref=True)


def test_rp_plan_exec_restatement_consistent(orc):
    """The numpy restatement of rp_spmm_init/exec (parity unpinned: its reference
    translation unit needs mkl.h) reproduces the single-process product A*B."""
    from crp_spmm_amd import gen
    m = k = 600
    rp, ci, va = gen.random_csr(m, k, 10, seed=5, empty_every=7)
    n = 6
    B = orc.fill_B(0, k, 0, n)
    ref = orc.spmm_csr(rp, ci, va, B)
    for P in (1, 2, 3, 4):
        rb = orc.csr_row_partition(rp, P)
        parts = [(rp[rb[r]:rb[r + 1] + 1], ci[rp[rb[r]]:rp[rb[r + 1]]], va[rp[rb[r]]:rp[rb[r + 1]]]) for r in range(P)]
        for reidx in (1, 0):
            plans = orc.rp_plan_all(parts, rb, n, reidx=reidx)
            for d in plans:
                d["reidx"] = reidx
            Cs = orc.rp_exec_all(plans, [B[rb[r]:rb[r + 1]] for r in range(P)], n)
            assert orc.rel_fro_err(ref, np.vstack(Cs)) <= 1e-14
