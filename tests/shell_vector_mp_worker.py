"""Worker of tests/test_shell_vector_sharded.py: every rank runs the rotating shell convection of
tests/shell_vector_cases.py with mesh=(world,) (azimuthal wavenumbers block-distributed, torch.distributed gloo) on the
NumPy oracle executor and saves its local coefficient blocks."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    outdir = sys.argv[1]
    import torch.distributed as dist
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    import dedalus_amd.public as d3
    import shell_vector_cases as sv
    from oracle.np_executor import NumpyExecutor
    solver, res = sv.run_rotating_convection(d3, dict(executor=sv.with_rot(NumpyExecutor), mesh=(world,)))
    np.savez(os.path.join(outdir, "rank%d.npz" % rank), **res)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
