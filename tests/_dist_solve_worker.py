"""Worker of tests/test_gpu_dist_solve.py::test_two_processes_over_gloo: one rank of a gloo group, both on device 0.  Each rank takes its
rows of the dist2d slab world of tests/halo_cases.py, assembles them, and the group solves through
polydeal_amd.distributed.TorchRank.solve_cg_torch (all_to_all_single for the halo, all_reduce for the sums, staged through the host under
gloo); rank 0 checks the gathered solution against the dense solve of the oracle's matrix."""
import os
import sys

import numpy as np
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import halo_cases as hc  # noqa: E402
import polydeal_amd as pa  # noqa: E402
from device_buffers import Device  # noqa: E402
from polydeal_amd.distributed import TorchRank  # noqa: E402


def main():
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    w = hc.world("slab_dist2d_dgq1")
    part = w.part
    assert part.world == world == 2
    prob, (r0, r1) = part.problems()[rank]
    b = hc.rhs("slab_dist2d_dgq1")
    ctx, dev = pa.Context(0), Device()
    try:
        ctx.set_problem(prob, r0, r1)
        ctx.assemble_device()
        ctx.setup_preconditioner("block_jacobi")
        tr = TorchRank(ctx, part.splits)
        exp = w.expected()
        assert tr.send_count == hc.send_matrix(exp)[rank].tolist() and tr.recv_count == hc.send_matrix(exp)[:, rank].tolist()
        d_b, d_x = dev.put(b[r0:r1]), dev.put(np.zeros(r1 - r0))
        info = tr.solve_cg_torch(d_b, d_x)
        ctx.synchronize()
        x_own = dev.get(d_x, r1 - r0)
    finally:
        ctx.close()
        dev.free()
    pieces, infos = [None] * world, [None] * world
    dist.all_gather_object(pieces, x_own)
    dist.all_gather_object(infos, info)
    assert infos[0] == infos[1], infos  # the same iteration count and the same residual bits on both ranks
    if rank == 0:
        A = w.dense()
        ref = np.linalg.solve(A, b)
        x = np.concatenate(pieces)
        assert np.linalg.norm(x - ref) <= 1e-9 * np.linalg.norm(ref), (infos, np.linalg.norm(x - ref) / np.linalg.norm(ref))
        assert info["residual"] <= 1e-13 * np.linalg.norm(b)
        print("DIST_SOLVE_OK world=%d iterations=%d" % (world, info["iterations"]))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
