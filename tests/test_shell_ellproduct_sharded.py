"""CPU, 2 processes (gloo): the induction run with potential-field walls of tests/shell_ellproduct_cases.py on the m-sharded
shell.  SphericalEllProduct is local in (m, l): with the azimuthal wavenumbers block-distributed the run reproduces the
reference's serial end state (tests/golden/shell_ellproduct_ivp.npz) to the serial test's 1e-10 -- every variable in its own
norm here, which for a tau is the stricter measure (its own term is one of the terms of the equation it corrects)."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-10


def test_m_sharded_potential_wall_induction_matches_reference(golden_dir):
    import dedalus_amd.public as d3
    assert callable(d3.SphericalEllProduct)
    gold = np.load(os.path.join(golden_dir, "shell_ellproduct_ivp.npz"))
    world, ts = 2, "SBDF2"
    with tempfile.TemporaryDirectory() as tmp:
        port = 29500 + (os.getpid() % 2000)
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world),
               "--master-addr", "127.0.0.1", "--master-port", str(port),
               os.path.join(ROOT, "tests", "shell_ellproduct_mp_worker.py"), tmp, ts]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=dict(os.environ, OMP_NUM_THREADS="1"))
        assert r.returncode == 0, r.stderr[-3000:]
        parts = [np.load(os.path.join(tmp, "rank%d.npz" % k)) for k in range(world)]
    for key in ("A", "phi", "tau_A1", "tau_A2"):
        ref = gold["%s/%s" % (ts, key)]
        full = np.concatenate([p[key] for p in parts], axis=ref.ndim - 3)      # the packed azimuthal axis is distributed
        assert full.shape == ref.shape, (key, full.shape, ref.shape)
        err = float(np.linalg.norm((full - ref).ravel()) / np.linalg.norm(ref.ravel()))
        print("sharded %s %s: %.2e" % (ts, key, err))
        assert err <= TOL, (key, err)
    assert all(abs(float(p["tau_phi"].reshape(-1)[0])) < 1e-10 for p in parts)
