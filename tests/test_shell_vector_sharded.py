"""CPU, 2 processes (gloo): cross product and curl on the m-sharded shell.  The rotating convection run of
tests/shell_vector_cases.py with the azimuthal wavenumbers block-distributed -- ez set on the local colatitudes, the
(m, l) = (0, 0) msin hole of the curl on the rank that owns m = 0 only -- reproduces the reference's serial end state, the
curl(u) task and sqrt(curl(u)@curl(u)) (tests/golden/shell_vector_ivp.npz) within the bounds of the serial test."""
import os
import subprocess
import sys
import tempfile

import numpy as np

from test_shell_fields import CONV_TOL, _rel as rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_m_sharded_rotating_convection_matches_reference(golden_dir):
    gold = np.load(os.path.join(golden_dir, "shell_vector_ivp.npz"))
    world = 2
    with tempfile.TemporaryDirectory() as tmp:
        port = 29500 + (os.getpid() % 2000)
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world),
               "--master-addr", "127.0.0.1", "--master-port", str(port),
               os.path.join(ROOT, "tests", "shell_vector_mp_worker.py"), tmp]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=dict(os.environ, OMP_NUM_THREADS="1"))
        assert r.returncode == 0, r.stderr[-3000:]
        parts = [np.load(os.path.join(tmp, "rank%d.npz" % k)) for k in range(world)]
    tol = dict(CONV_TOL, curl_u=CONV_TOL["u"], enstrophy_sqrt=CONV_TOL["u"])
    for key, t in tol.items():
        ref = gold["end/" + key]
        full = np.concatenate([p[key] for p in parts], axis=ref.ndim - 3)      # the packed azimuthal axis is distributed
        assert full.shape == ref.shape, (key, full.shape, ref.shape)
        assert rel(full, ref) < t, (key, rel(full, ref))
    assert all(abs(float(p["tau_p"].reshape(-1)[0])) < 1e-10 for p in parts)
