"""Worker of tests/test_cheb_multirank_gpu.py: the 60 x 61 Laplacian split by rows over the ranks (rendez-vous and
communicator as in tests/mp_worker_gpu.py), 3 smallest with GD+k and the Chebyshev polynomial preconditioner — whose operator
applications go through the ready-made operator with its halo exchange (the generic path).  Results to <out>.<rank>."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def run(rank, world, port, out_path):
    import torch
    import torch.distributed as dist
    from mp_worker_gpu import split
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(rank % max(torch.cuda.device_count(), 1))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from primme_amd import _ffi as F, problems
    from primme_amd.api import Operator, Session
    lib = F.load_product()
    buf = (C.c_char * 128)()
    if rank == 0:
        assert lib.primme_amd_comm_unique_id(buf) == 0
    uid = torch.frombuffer(bytearray(buf.raw), dtype=torch.uint8).clone()
    dist.broadcast(uid, 0)
    comm = C.c_void_p()
    assert lib.primme_amd_comm_create(C.byref(comm), bytes(uid.numpy().tobytes()), rank, world) == 0
    dims = (60, 61)
    n = int(np.prod(dims))
    row0, nloc = split(n, world, rank)
    rp, ci, va, _ = problems.laplacian_csr(dims, row0=row0, nrows=nloc)
    s = Session(Operator(n, csr=(rp, ci, va), row0=row0, nrows=nloc), comm=comm)
    glo, ghi = C.c_double(), C.c_double()
    assert lib.primme_amd_operator_gershgorin(s.oph, C.byref(glo), C.byref(ghi)) == 0
    r = s.solve(numEvals=3, eps=1e-8, aNorm=8.0, method="GD_plusK", numProcs=world, procID=rank, precond=("chebyshev", 8, 0.1),
                v0=problems.start_vector(n, row0=row0, nrows=nloc))
    s.close()
    json.dump(dict(rank=rank, ret=r.ret, evals=r.evals.tolist(), resNorms=r.resNorms.tolist(), its=r.stats["numOuterIterations"],
                   preconds=r.stats["numPreconds"], stats=r.precond_stats, gershgorin=[glo.value, ghi.value]), open(f"{out_path}.{rank}", "w"))
    dist.barrier()
    lib.primme_amd_comm_destroy(comm)
    dist.destroy_process_group()


if __name__ == "__main__":
    run(int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4])
