"""CPU: graph-based 1D row partitioning (part-method 1, include/crp_part.h) and the host path of the symmetric
permutation P A P^T -- validity and balance of the partition, the permutation against a numpy restatement of its
output rule, independence of the thread count, partition quality on the planner's own comm measure, bad inputs."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

NPROCS = (1, 2, 3, 5, 8)


def _shuffled(rp, ci, va, seed=11):
    from crp_spmm_amd import partition
    perm = np.random.default_rng(seed).permutation(rp.size - 1).astype(np.int32)
    return partition.permute_sym(rp, ci, va, perm)


def _from_coo(n, rows, cols, seed=5):
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    o = np.lexsort((cols, rows))
    rows, cols = rows[o], cols[o]
    rp = np.zeros(n + 1, np.int64)
    np.add.at(rp, rows + 1, 1)
    vals = np.random.default_rng(seed).uniform(-1.0, 1.0, rows.size)
    return np.cumsum(rp).astype(np.int32), cols.astype(np.int32), vals


def _disconnected():
    from crp_spmm_amd import gen
    parts, off, rows, cols = [gen.kkt3d(4), gen.fem3d(3, dof=2), gen.kkt3d(3)], 0, [], []
    for rp, ci, _ in parts:
        n = rp.size - 1
        rows.append(np.repeat(np.arange(n), np.diff(rp)) + off)
        cols.append(ci.astype(np.int64) + off)
        off += n
    rows.append(np.arange(off, off + 7))                     # and a few isolated diagonal-only rows
    cols.append(np.arange(off, off + 7))
    return _from_coo(off + 7, np.concatenate(rows), np.concatenate(cols))


def _arrow(n=72000):
    """dense first row and column, plus the diagonal: one row of n >= 70 000 entries"""
    i = np.arange(n)
    rows = np.concatenate([np.zeros(n, np.int64), i[1:], i[1:]])
    cols = np.concatenate([i, np.zeros(n - 1, np.int64), i[1:]])
    return _from_coo(n, rows, cols)


def _matrices():
    from crp_spmm_amd import gen
    return {
        "kkt3d": gen.kkt3d(8),
        "fem3d_shuffled": _shuffled(*gen.fem3d(6)),
        "empty_rows": gen.random_csr(700, 700, 9, seed=3, empty_every=4),
        "disconnected": _disconnected(),
        "arrow": _arrow(),
    }


@pytest.fixture(scope="module")
def mats(crp):
    return _matrices()


def numpy_permute(rp, ci, va, perm):
    """the output rule of crp_csr_permute_sym: row perm[i] <- row i, columns perm[c] ascending, ties by position"""
    n = rp.size - 1
    rows = np.repeat(np.arange(n), np.diff(rp))
    o = np.lexsort((np.arange(ci.size), perm[ci], perm[rows]))
    rp1 = np.zeros(n + 1, np.int64)
    np.add.at(rp1, perm[rows] + 1, 1)
    return np.cumsum(rp1).astype(np.int32), perm[ci][o].astype(np.int32), va[o]


def check_partition(rp, perm, displs, nproc):
    n = rp.size - 1
    assert perm.shape == (n,) and displs.shape == (nproc + 1,)
    assert np.array_equal(np.sort(perm), np.arange(n)), "perm is not a bijection"
    assert displs[0] == 0 and displs[-1] == n and np.all(np.diff(displs) >= 0)
    # nonzeros of every part after the permutation
    lens = np.diff(rp).astype(np.int64)
    new_lens = np.zeros(n, np.int64)
    new_lens[perm] = lens
    part_nnz = np.add.reduceat(np.append(new_lens, 0), displs[:-1]) * (np.diff(displs) > 0)
    bound = 1.05 * lens.sum() / nproc + (lens.max() if n else 0)
    assert part_nnz.max() <= bound, (part_nnz.max(), bound)
    # inside a part, the rows keep their original relative order
    part_of = np.searchsorted(displs, perm, side="right") - 1
    for q in range(nproc):
        mine = np.nonzero(part_of == q)[0]
        assert np.array_equal(perm[mine], np.arange(displs[q], displs[q + 1]))


@pytest.mark.parametrize("name", ["kkt3d", "fem3d_shuffled", "empty_rows", "disconnected", "arrow"])
@pytest.mark.parametrize("nproc", NPROCS)
def test_partition_valid_and_balanced(mats, name, nproc):
    from crp_spmm_amd import partition
    rp, ci, _ = mats[name]
    perm, displs = partition.graph_row_order(rp, ci, nproc)
    check_partition(rp, perm, displs, nproc)
    if nproc == 1:
        assert np.array_equal(perm, np.arange(rp.size - 1))


@pytest.mark.parametrize("nproc", [8, 13])
def test_partition_more_ranks_than_rows(crp, nproc):
    from crp_spmm_amd import gen, partition
    rp, ci, _ = gen.random_csr(5, 5, 3, seed=2)
    perm, displs = partition.graph_row_order(rp, ci, nproc)
    check_partition(rp, perm, displs, nproc)


@pytest.mark.parametrize("name", ["kkt3d", "fem3d_shuffled", "empty_rows", "disconnected", "arrow"])
def test_host_permutation_matches_numpy(mats, name):
    from crp_spmm_amd import partition
    rp, ci, va = mats[name]
    for nproc in (3, 8):
        perm, _ = partition.graph_row_order(rp, ci, nproc)
        got = partition.permute_sym(rp, ci, va, perm)
        want = numpy_permute(rp, ci, va, perm)
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and np.array_equal(g, w)        # bit for bit, values included


def test_host_permutation_duplicate_columns(crp):
    """duplicate columns of one row keep their original order (the tie rule)"""
    from crp_spmm_amd import partition
    rng = np.random.default_rng(4)
    n = 300
    lens = rng.integers(0, 90, n)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ci = rng.integers(0, 20, rp[-1]).astype(np.int32)        # unsorted, many repeats
    va = rng.standard_normal(rp[-1])
    perm = rng.permutation(n).astype(np.int32)
    for g, w in zip(partition.permute_sym(rp, ci, va, perm), numpy_permute(rp, ci, va, perm)):
        assert np.array_equal(g, w)


def test_graph_row_partition_host_in_place(mats):
    from crp_spmm_amd import partition
    rp, ci, va = mats["fem3d_shuffled"]
    rp1, ci1, va1, perm, displs = partition.graph_row_partition(rp, ci, va, 5, where=0)
    p2, d2 = partition.graph_row_order(rp, ci, 5)
    assert np.array_equal(perm, p2) and np.array_equal(displs, d2)
    for g, w in zip((rp1, ci1, va1), numpy_permute(rp, ci, va, perm)):
        assert np.array_equal(g, w)


_DIGEST = """
import hashlib, sys
sys.path.insert(0, %r)
import numpy as np
import crp_spmm_amd
from crp_spmm_amd import gen, partition
rp, ci, va = gen.fem3d(7)
perm0 = np.random.default_rng(3).permutation(rp.size - 1).astype(np.int32)
rp, ci, va = partition.permute_sym(rp, ci, va, perm0)
h = hashlib.sha256()
for p in (3, 8):
    perm, displs = partition.graph_row_order(rp, ci, p)
    for a in (perm, displs) + tuple(partition.permute_sym(rp, ci, va, perm)):
        h.update(np.ascontiguousarray(a).tobytes())
print(h.hexdigest())
"""


def test_deterministic_across_thread_counts(crp):
    digests = []
    for threads in ("1", "8"):
        env = dict(os.environ, OMP_NUM_THREADS=threads)
        env.pop("CRPSPMM_NUM_THREADS", None)
        r = subprocess.run([sys.executable, "-c", _DIGEST % ROOT], capture_output=True, text=True, env=env, cwd=ROOT,
                           timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        digests.append(r.stdout.strip().splitlines()[-1])
    assert digests[0] == digests[1]


@pytest.mark.parametrize("nproc", [3, 8])
def test_quality_on_kkt(crp, nproc):
    """planner.csr_mat_row_part_comm_size: the graph partition needs at most half the B rows of the native split in
    natural order, at most a quarter when the rows are shuffled"""
    from crp_spmm_amd import gen, partition, planner
    for rp, ci, va, limit in [gen.kkt3d(20) + (0.5,), _shuffled(*gen.kkt3d(20)) + (0.25,)]:
        n = rp.size - 1
        native = planner.csr_mat_row_partition(rp, nproc)
        _, tot0 = planner.csr_mat_row_part_comm_size(n, rp, ci, native, native)
        perm, displs = partition.graph_row_order(rp, ci, nproc)
        rp1, ci1, _ = partition.permute_sym(rp, ci, va, perm)
        _, tot1 = planner.csr_mat_row_part_comm_size(n, rp1, ci1, displs, displs)
        assert tot1 <= limit * tot0, (tot1, tot0)


def test_bad_inputs_return_codes(crp):
    from crp_spmm_amd import gen, partition
    rp, ci, va = gen.kkt3d(4)
    n = rp.size - 1
    perm = np.arange(n, dtype=np.int32)[::-1].copy()
    dup = perm.copy()
    dup[3] = dup[4]
    with pytest.raises(partition.PartitionError) as e:
        partition.permute_sym(rp, ci, va, dup)
    assert e.value.code == partition.EPERM
    out = perm.copy()
    out[0] = n
    with pytest.raises(partition.PartitionError) as e:
        partition.permute_sym(rp, ci, va, out)
    assert e.value.code == partition.EPERM
    bad = ci.copy()
    bad[17] = n
    with pytest.raises(partition.PartitionError) as e:
        partition.permute_sym(rp, bad, va, perm)
    assert e.value.code == partition.ECOL
    with pytest.raises(partition.PartitionError) as e:
        partition.graph_row_order(rp, bad, 3)
    assert e.value.code == partition.ECOL
    neg = ci.copy()
    neg[0] = -1
    with pytest.raises(partition.PartitionError) as e:
        partition.graph_row_partition(rp, neg, va, 2, where=0)
    assert e.value.code == partition.ECOL
    dec = rp.copy()
    dec[5] = dec[7]
    with pytest.raises(partition.PartitionError) as e:
        partition.permute_sym(dec, ci, va, perm)
    assert e.value.code == partition.EPTR
    with pytest.raises(partition.PartitionError) as e:
        partition.graph_row_order(rp, ci, 0)
    assert e.value.code == partition.EARG
