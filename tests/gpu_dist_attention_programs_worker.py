"""Worker for tests/test_gpu_attention_programs.py: the several-rank family of the row-engine programs of
tests/attention_programs.py on N ranks that share ONE GPU, device payloads staged through the host (the rehearsal mode of
tests/gpu_dist_worker.py).  Every rank generates the same programs from their seeds and issues the same steps through the runner
class of the test module (EngineRun) on its rows of A and of B: the partition is planner.csr_mat_row_partition; one program runs on
the layout with a rank without rows of A and one on the layout with a rank without rows of B; on the balanced layout some rank's
engine is split into interior and boundary rows.  What is held is stated in the test module."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import torch
    import torch.distributed as dist
    import crp_spmm_amd
    from crp_spmm_amd import comm as crp_comm
    import attention_programs as AP
    import test_gpu_attention_programs as TP

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    crp_comm.init_process_group(device=None)
    assert crp_comm.exchange_mode() == "host"
    world = crp_comm.TorchComm()
    P, me = world.nproc, world.rank
    assert P > 1
    crp_spmm_amd.load()
    for index, (prog, n) in enumerate(AP.engine_programs(True)):
        layout = AP.ENGINE_LAYOUTS[index]
        pat = AP.pattern(prog.matrix, False)
        rb, bd = AP.partition(layout, pat.rp, P, pat.k)
        run = TP.EngineRun(prog, n, dev, world, (rb[me], rb[me + 1]), bd, True)
        # what the layout is for, seen on the engines themselves
        probe = run.engine()
        flags = torch.tensor([int(sum(probe.overlap_rows()) > 0), int(run.m == 0), int(run.kb == 0)], device=dev)
        probe.free()
        dist.all_reduce(flags)
        if layout == "balanced":
            assert int(flags[0]) > 0, "no rank's engine is split"
        elif layout == "a rank without rows of A":
            assert int(flags[1]) > 0, "every rank holds rows of A"
        else:
            assert int(flags[2]) > 0, "every rank holds rows of B"
        t = time.perf_counter()
        # a failed comparison is held until every rank has issued the whole program, and the ranks then stop together: a rank that
        # left alone would take its peers down inside their next exchange
        failure, ms = None, 0.0
        try:
            ms = run.run()
        except TP.Stranded:
            raise                       # (the peers are inside an exchange and cannot be told: they end when this rank is gone)
        except AssertionError as e:
            failure = e
        failed = torch.tensor([int(failure is not None)], device=dev)
        dist.all_reduce(failed)
        if int(failed[0]) > 0:
            if failure is not None:
                print("rank %d: %s" % (me, failure), flush=True)
            dist.barrier()
            dist.destroy_process_group()
            sys.exit(1)
        if me == 0:
            print("attention engine program %d (seed %d, %s, glb_n %d, %s) on %d ranks: %d steps, %.1f ms on the device, %.2f s in all; "
                  "steps / bitwise / bounded so far %r; worst error / bound so far: %s"
                  % (index, prog.seed, prog.matrix, n, layout, P, len(prog.steps), ms, time.perf_counter() - t, TP.COUNTS["engine"], TP._worst()))
    torch.cuda.synchronize()
    if me == 0:
        print("GPU_DIST_ATTENTION_PROGRAMS_WORKER_OK world=%d" % P)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
