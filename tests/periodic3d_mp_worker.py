"""Worker of tests/test_periodic3d_sharded.py: every rank runs Taylor-Green of tests/periodic3d_cases.py with
mesh=(world,) (kx block-distributed, grid space sharded along the Fourier pencil axis z; torch.distributed gloo) on the
NumPy oracle executor and saves its local coefficient blocks."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    outdir, ts = sys.argv[1], sys.argv[2]
    import torch.distributed as dist
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    import dedalus_amd.public as d3
    import periodic3d_cases as pc
    from oracle.np_executor import NumpyExecutor
    solver, start, end = pc.run_ivp(d3, pc.taylor_green, shape=(16, 16, 8), timestepper=ts,
                                    dist_kw=dict(executor=NumpyExecutor(), mesh=(world,)))
    assert solver.dist.shard_grid_axis == 2 and solver.dist.shard_coeff_axis == 0
    np.savez(os.path.join(outdir, "rank%d.npz" % rank), **end)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
