"""Worker of tests/test_shell_curl_lhs_sharded.py: every rank runs the alpha^2 dynamo of tests/shell_curl_lhs_cases.py with
mesh=(world,) (azimuthal wavenumbers block-distributed, torch.distributed gloo) on the NumPy oracle executor with complex
per-ell systems and saves its local coefficient blocks."""
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
    import shell_curl_lhs_cases as sc
    gold = np.load(os.path.join(ROOT, "tests", "golden", "shell_curl_lhs.npz"))
    solver, f, res = sc.run_alpha2_dynamo(d3, ts, gold["ivp/in_B"], dict(executor=sc.oracle_executor(), mesh=(world,)))
    assert solver.cx and solver._band and solver._band["plan"].cx
    np.savez(os.path.join(outdir, "rank%d.npz" % rank), **res)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
