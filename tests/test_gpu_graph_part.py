"""GPU: the device path of the symmetric permutation P A P^T (csrc/permute_kernels.hip) against the host path, bit
for bit, over every row-length tier; bad inputs return codes on the device; products on the permuted matrix; the
example programs with part-method 1 (graph 1D row partitioning)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

MPIEXEC = shutil.which("mpiexec") or "/opt/conda/bin/mpiexec"


def _dev(gpu, *arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).to(gpu) for a in arrays]


def _tier_matrix(seed=1):
    """row lengths on every tier edge of the device sort (0, 1, 64, 65, the LDS limit, one more, >= 70 000) plus
    random ones; columns unsorted with repeats (the tie rule)"""
    from crp_spmm_amd import partition
    rng = np.random.default_rng(seed)
    n = 3000
    lens = rng.integers(0, 120, n)
    edges = [0, 1, 2, 63, 64, 65, 66, 127, 128, 129, partition.PERMUTE_LDS_PAIRS - 1, partition.PERMUTE_LDS_PAIRS,
             partition.PERMUTE_LDS_PAIRS + 1, 70000, 70001]
    pos = rng.choice(n, size=len(edges), replace=False)
    lens[pos] = edges
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ci = rng.integers(0, n, rp[-1]).astype(np.int32)
    va = rng.standard_normal(rp[-1])
    perm = rng.permutation(n).astype(np.int32)
    return rp, ci, va, perm


def _host_and_device(gpu, rp, ci, va, perm):
    import torch
    from crp_spmm_amd import partition
    want = partition.permute_sym(rp, ci, va, perm)
    got = partition.permute_sym(*_dev(gpu, rp, ci, va, perm))
    torch.cuda.synchronize()
    return want, [t.cpu().numpy() for t in got]


def test_device_permutation_matches_host_on_every_tier(crp, gpu):
    rp, ci, va, perm = _tier_matrix()
    want, got = _host_and_device(gpu, rp, ci, va, perm)
    for w, g in zip(want, got):
        assert w.dtype == g.dtype and np.array_equal(w, g)


def test_device_permutation_matches_host_on_partitions(crp, gpu):
    from crp_spmm_amd import gen, partition
    for rp, ci, va in (gen.kkt3d(10), gen.fem3d(7)):
        perm0 = np.random.default_rng(2).permutation(rp.size - 1).astype(np.int32)
        want, got = _host_and_device(gpu, rp, ci, va, perm0)
        for w, g in zip(want, got):
            assert np.array_equal(w, g)
        perm, _ = partition.graph_row_order(*want[:2], 6)
        w2, g2 = _host_and_device(gpu, *want, perm)
        for w, g in zip(w2, g2):
            assert np.array_equal(w, g)


def test_graph_row_partition_device_staging_matches_host(crp, gpu):
    from crp_spmm_amd import gen, partition
    rp, ci, va = gen.fem3d(6)
    host = partition.graph_row_partition(rp, ci, va, 5, where=0)
    dev = partition.graph_row_partition(rp, ci, va, 5, where=1)
    for h, d in zip(host, dev):
        assert np.array_equal(h, d)


def test_device_bad_inputs_return_codes(crp, gpu):
    import torch
    from crp_spmm_amd import _lib, gen, partition
    rp, ci, va = gen.kkt3d(5)
    n = rp.size - 1
    perm = np.random.default_rng(5).permutation(n).astype(np.int32)
    dup = perm.copy()
    dup[10] = dup[11]
    out = perm.copy()
    out[3] = n + 5
    bad = ci.copy()
    bad[-1] = n
    for args, code in (((rp, ci, va, dup), partition.EPERM), ((rp, ci, va, out), partition.EPERM),
                       ((rp, bad, va, perm), partition.ECOL)):
        with pytest.raises(partition.PartitionError) as e:
            partition.permute_sym(*_dev(gpu, *args))
        assert e.value.code == code
    # one host pointer among device pointers
    d_rp, d_ci, d_va, d_perm = _dev(gpu, rp, ci, va, perm)
    rp1, ci1, va1 = torch.empty_like(d_rp), torch.empty_like(d_ci), torch.empty_like(d_va)
    rc = _lib.load().crp_csr_permute_sym(n, rp.ctypes.data, d_ci.data_ptr(), d_va.data_ptr(), d_perm.data_ptr(),
                                         rp1.data_ptr(), ci1.data_ptr(), va1.data_ptr(), None)
    assert rc == partition.EMIXED
    # and the device is still fine afterwards
    want, got = _host_and_device(gpu, rp, ci, va, perm)
    for w, g in zip(want, got):
        assert np.array_equal(w, g)


def test_product_on_permuted_matrix(crp, gpu):
    """(P A P^T)(P B) = P (A B)"""
    import torch
    import oracle
    from crp_spmm_amd import gen, hip, partition
    rp, ci, va = gen.kkt3d(9)
    n, ncol = rp.size - 1, 40
    perm, _ = partition.graph_row_order(rp, ci, 4)
    d1 = partition.permute_sym(*_dev(gpu, rp, ci, va, perm))
    rp1, ci1, va1 = [t.cpu().numpy() for t in d1]
    B = oracle.fill_B(0, n, 0, ncol)
    PB = np.empty_like(B)
    PB[perm] = B
    A1 = hip.CsrDev(n, n, rp1, ci1, va1)
    Cd = torch.empty((n, ncol), dtype=torch.float64, device=gpu)
    hip.spmm_csr(A1, torch.from_numpy(PB).to(gpu), Cd)
    torch.cuda.synchronize()
    A1.free()
    ref = oracle.spmm_csr(rp, ci, va, B)
    Pref = np.empty_like(ref)
    Pref[perm] = ref
    assert oracle.rel_fro_err(Pref, Cd.cpu().numpy()) <= 1e-12


# ---- the example programs with part-method 1

def _kkt_mtx(tmp_path):
    from crp_spmm_amd import gen, mmio
    rp, ci, va = gen.kkt3d(6)
    rows = np.repeat(np.arange(rp.size - 1), np.diff(rp))
    keep = rows >= ci
    path = os.path.join(str(tmp_path), "kkt3d_6.mtx")
    mmio.write_mtx(path, rp.size - 1, rp.size - 1, rows[keep], ci[keep], va[keep], symmetry="symmetric")
    return path


def _launch(exe, np_, mtx, *tail):
    path = os.path.join(ROOT, "examples", exe)
    if not os.path.exists(path) or not os.path.exists(MPIEXEC):
        pytest.skip("no MPI launcher / example drivers not built on this machine")
    env = dict(os.environ, OMP_NUM_THREADS="1")
    env["PATH"] = os.path.dirname(MPIEXEC) + ":" + env["PATH"]
    return subprocess.run([MPIEXEC, "-np", str(np_), path, mtx, *[str(t) for t in tail]], capture_output=True, text=True,
                          env=env, timeout=600, cwd=ROOT)


def _run_checked(exe, np_, mtx, n, method):
    r = _launch(exe, np_, mtx, n, 2, method, 1)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    m = re.search(r"\|\|C_ref - C\|\|_f / \|\|C_ref\|\|_f = ([0-9.eE+-]+)", r.stdout)
    assert m, r.stdout[-2000:]
    assert float(m.group(1)) <= 1e-12
    return r.stdout


def _comm(out):
    return int(re.search(r"Total SpMV comm size = (\d+)", out).group(1))


@pytest.mark.parametrize("np_", [1, 2, 3])
def test_rp_spmm_driver_graph_partition(np_, tmp_path):
    out = _run_checked("test_rp_spmm.exe", np_, os.path.join(GOLDEN, "g_symm.mtx"), 33, 1)
    assert "Using graph 1D row partitioning (METIS-free)" in out and "Total rp_spmm_exec()" in out
    kkt = _kkt_mtx(tmp_path)
    graph = _run_checked("test_rp_spmm.exe", np_, kkt, 16, 1)
    assert "Using graph 1D row partitioning (METIS-free)" in graph
    if np_ > 1:
        native = _run_checked("test_rp_spmm.exe", np_, kkt, 16, 0)
        assert "Using naive 1D row partitioning" in native
        assert _comm(graph) < _comm(native), (_comm(graph), _comm(native))


@pytest.mark.parametrize("np_", [1, 2, 4])
def test_para2d_spmm_driver_graph_partition(np_):
    out = _run_checked("test_para2d_spmm.exe", np_, os.path.join(GOLDEN, "g_symm.mtx"), 64, 1)
    assert "Using graph 1D row partitioning (METIS-free)" in out
    assert "2D process grid: pm, pn =" in out and "Total para2d_spmm_exec()" in out


def test_spmm_2dpg_graph_partition_lowers_comm_cost(tmp_path):
    kkt = _kkt_mtx(tmp_path)
    costs = []
    for method in (0, 1):
        r = _launch("test_spmm_2dpg.exe", 1, kkt, 64, 4, method)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        costs.append(int(re.search(r"Calculated 2D grid: pm, pn = \d+, \d+, comm cost = (\d+)", r.stdout).group(1)))
    assert costs[1] < costs[0], costs


def test_graph_partition_refuses_general_file():
    r = _launch("test_rp_spmm.exe", 1, os.path.join(GOLDEN, "g_gen.mtx"), 8, 2, 1, 1)
    assert r.returncode != 0
    r = _launch("test_rp_spmm.exe", 1, os.path.join(GOLDEN, "g_symm.mtx"), 8, 2, 2, 1)
    assert r.returncode == 254
