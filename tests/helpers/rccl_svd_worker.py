"""Worker of tests/test_gpu_comm.py::test_ranks_over_the_collective_calls (and of the segmented product pass test):
ranks of a column-sharded bed_randomSVD whose exchange runs inside the library over RCCL.  torch.distributed (gloo)
only carries the unique id and the results.  One rank (= one GPU) per process; with BSN_TEST_RANKS_PER_PROCESS=r the
BSN_TEST_WORLD ranks run as threads, r to a process (process p holds ranks p r ... p r + r - 1), so that a world larger
than the processes one GPU takes still runs through the same library calls.
Usage (via torch.distributed.run): rccl_svd_worker.py n m k out.json"""
import json
import os
import sys
import threading
import time
import traceback

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch  # noqa: F401  (first: the library binds to the HIP runtime torch brings)
import torch.distributed as dist


def run_rank(ba, _lib, uid, rank, world, n, m, k):
    # one GPU per rank; with BSN_RCCL_LIBRARY naming the shared-memory stand-in the ranks share what there is
    _lib.check(_lib.load().bsn_set_device(rank % ba.device_count()))
    comm = ba.Comm(uid, rank, world)
    j0, j1 = (m * rank) // world, (m * (rank + 1)) // world
    gb = ba.bed.synthetic(n, j1 - j0, seed=31, j_begin=j0)
    # BSN_TEST_BLOCK / BSN_TEST_TOL: the configuration of the segmented product pass test (16-vector blocks)
    res = ba.bed_randomSVD(gb, k=k, tol=float(os.environ.get("BSN_TEST_TOL", "1e-9")), comm=comm, m_total=m,
                           block=int(os.environ.get("BSN_TEST_BLOCK", "0")))
    # one-shot product of the column shards: x is the same seeded vector on every rank, each takes its slice
    x = np.random.default_rng(7).normal(size=m)
    y = ba.bed_prodVec(gb, x[j0:j1], center=res["center"], scale=res["scale"], comm=comm)
    comm.close()
    return dict(d=res["d"].tolist(), niter=res["niter"], y=y.tolist() if rank == 0 else None,
                usum=float(np.abs(res["u"]).sum()), vsum=float(np.abs(res["v"]).sum()),
                segmented_passes=res["segmented_passes"], compact_gathers=res["compact_gathers"], tiled=res["tiled"])


def main():
    n, m, k, out = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    proc, nproc = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    per = int(os.environ.get("BSN_TEST_RANKS_PER_PROCESS", "1"))
    world = int(os.environ.get("BSN_TEST_WORLD", str(nproc * per)))
    dist.init_process_group("gloo", rank=proc, world_size=nproc)
    import bigsnpr_amd as ba
    from bigsnpr_amd import _lib
    uid = [ba.Comm.unique_id() if proc == 0 else None]
    dist.broadcast_object_list(uid, src=0)
    ranks = range(proc * per, min(world, (proc + 1) * per))
    results = {}
    if per == 1:
        results[proc] = run_rank(ba, _lib, uid[0], proc, world, n, m, k)
    else:
        ba.Comm.unique_id()   # binds the transport's entry points once, before the threads
        errors = []

        def body(rank):
            try:
                results[rank] = run_rank(ba, _lib, uid[0], rank, world, n, m, k)
            except BaseException:
                errors.append("rank %d: %s" % (rank, traceback.format_exc()))

        threads = [threading.Thread(target=body, args=(r,), daemon=True) for r in ranks]
        for t in threads:
            t.start()
        while any(t.is_alive() for t in threads) and not errors:
            time.sleep(0.05)
        if errors:
            # the other ranks of this process wait in a collective that will not complete: end the process, the
            # launcher ends the others
            sys.stderr.write(errors[0])
            sys.stderr.flush()
            os._exit(1)
    gathered = [None] * nproc
    dist.all_gather_object(gathered, results)
    every = {r: res for part in gathered for r, res in part.items()}
    if proc == 0:
        assert sorted(every) == list(range(world)), sorted(every)
        key = lambda r: (every[r]["d"], every[r]["niter"], every[r]["usum"])
        first = every[0]
        json.dump(dict(d=first["d"], niter=first["niter"], same=all(key(r) == key(0) for r in every), y=first["y"],
                       usum=first["usum"], vsum=first["vsum"], segmented_passes=first["segmented_passes"],
                       compact_gathers=first["compact_gathers"], tiled=first["tiled"]), open(out, "w"))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
