#!/usr/bin/env python3
"""Generates ref_random.npz in this directory.  Run where oracle/_ref is built
(needs the reference's sources for `make -C oracle`):

    python tests/golden/make_golden_random.py

What the fixture pins: the answers of the REFERENCE's own planner and ingest
(oracle/_ref, compiled unmodified from src/spmat_part.c, src/utils.c,
examples/mmio_utils.c) on the seeded random matrices of
tests/test_oracle.py::test_restatement_matches_compiled_reference, so that the
test holds the restatement to them on machines without oracle/_ref:
  * s<seed>_input_sha256         sha256 of the generated (rowptr, colidx, val),
                                 to tell a changed generator from a changed planner;
  * s<seed>_P<P>_rb              csr_mat_row_partition;
  * s<seed>_P<P>_comm_sizes/_total   csr_mat_row_part_comm_size;
  * s<seed>_P<P>_n<n>_<field>    calc_spmm_part2d_from_1d (pm, pn, comm_cost and the four displacement arrays);
  * s<seed>_coo2csr_rowptr/_order    coo2csr of the entries in a seeded random order: the CSR row pointer and,
                                 for every CSR slot, the index of the input entry that lands there;
  * prime_360, block_spos        prime_factorization(360); calc_block_spos_size as rows (length, nblk, i, spos, size).
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import oracle  # noqa: E402

CASES = [(900, 900), (400, 1300), (1300, 400)]
PS = (1, 2, 3, 5, 6, 8, 12)
NS = (1, 16, 256, 2048)
SPOS = [(10, 3), (7, 7), (5, 8), (0, 2)]
PART2D = ("pm", "pn", "comm_cost", "A0_rowptr", "B_rowptr", "AC_rowptr", "BC_colptr")


def inputs(seed, m, k):
    """The test's matrix, its COO in a seeded random order, and the input digest."""
    from crp_spmm_amd import gen
    rp, ci, va = gen.random_csr(m, k, 15, seed=seed, empty_every=13 if seed else 0)
    rp, ci, va = (np.ascontiguousarray(rp, dtype=np.int32), np.ascontiguousarray(ci, dtype=np.int32),
                  np.ascontiguousarray(va, dtype=np.float64))
    sha = hashlib.sha256(rp.tobytes() + ci.tobytes() + va.tobytes()).hexdigest()
    rows = np.repeat(np.arange(m), np.diff(rp)).astype(np.int32)
    perm = np.random.default_rng(seed).permutation(rows.size)
    return rp, ci, va, sha, (rows[perm], ci[perm], va[perm])


def slot_order(row, col, val, rp, ci, cv):
    """For every slot of the CSR (rp, ci, cv), the index of the COO entry (row, col, val) it holds."""
    out_rows = np.repeat(np.arange(rp.size - 1), np.diff(rp))
    a = np.lexsort((val.view(np.int64), col, row))
    b = np.lexsort((cv.view(np.int64), ci, out_rows))
    order = np.empty(row.size, dtype=np.int32)
    order[b] = a
    assert np.array_equal(ci, col[order]) and np.array_equal(cv.view(np.int64), val[order].view(np.int64))
    return order


def main():
    oracle.build()
    assert oracle.ref() is not None, "oracle/_ref/libcrpref.so is not built: the reference's sources are needed"
    out = {}
    for seed, (m, k) in enumerate(CASES):
        rp, ci, va, sha, coo = inputs(seed, m, k)
        out["s%d_input_sha256" % seed] = np.array(sha)
        for P in PS:
            t = "s%d_P%d_" % (seed, P)
            a = oracle.csr_row_partition(rp, P, use_ref=True)
            out[t + "rb"] = a
            x = oracle.even_displs(k, P, use_ref=True) if m != k else a
            sizes, tot = oracle.csr_row_part_comm_size(k, rp, ci, a, x, use_ref=True)
            out[t + "comm_sizes"], out[t + "comm_total"] = sizes, np.array(tot, dtype=np.int64)
            for n in NS:
                r = oracle.part2d_from_1d(P, m, n, k, a, rp, ci, use_ref=True)
                for f in PART2D:
                    out["%sn%d_%s" % (t, n, f)] = np.asarray(r[f], dtype=np.int64 if np.isscalar(r[f]) else np.int32)
        rrp, rci, rcv = oracle.coo2csr(m, *coo, use_ref=True)
        out["s%d_coo2csr_rowptr" % seed] = rrp
        out["s%d_coo2csr_order" % seed] = slot_order(*coo, rrp, rci, rcv)
        print("seed %d: %d x %d, nnz %d" % (seed, m, k, rp[-1]))
    out["prime_360"] = np.array(oracle.prime_factorization(360, use_ref=True), dtype=np.int32)
    out["block_spos"] = np.array([(length, nblk, i) + oracle.block_spos(length, nblk, i, use_ref=True)
                                  for length, nblk in SPOS for i in range(-1, nblk + 2)], dtype=np.int32)
    np.savez_compressed(os.path.join(HERE, "ref_random.npz"), **out)


if __name__ == "__main__":
    main()
