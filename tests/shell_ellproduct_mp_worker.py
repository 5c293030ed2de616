"""Worker of tests/test_shell_ellproduct_sharded.py: every rank runs the induction problem with potential-field walls of
tests/shell_ellproduct_cases.py with mesh=(world,) (azimuthal wavenumbers block-distributed, torch.distributed gloo) on the
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
    import shell_ellproduct_cases as se
    import shell_tensor_cases as st
    import shell_vector_cases as sv
    from oracle.np_executor import NumpyExecutor
    gold = np.load(os.path.join(ROOT, "tests", "golden", "shell_ellproduct_ivp.npz"))
    ex = sv.with_rot(type(st.with_mix(NumpyExecutor)))
    solver, f, res = se.run_potential_induction(d3, ts, gold["ivp/in_A"], dict(executor=ex, mesh=(world,)))
    np.savez(os.path.join(outdir, "rank%d.npz" % rank), **res)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
