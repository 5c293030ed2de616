"""CPU, 2 processes (gloo): the RK222 alpha^2 dynamo of tests/shell_curl_lhs_cases.py on the m-sharded shell.  The complex
per-ell systems are local in (m, ell) and a (cos, msin) pair never straddles ranks: with the azimuthal wavenumbers
block-distributed the run reproduces the reference's serial end state (tests/golden/shell_curl_lhs.npz) to 1e-10, every
variable in its own norm (for a tau the stricter measure)."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-10


def test_m_sharded_alpha2_dynamo_matches_reference(golden_dir):
    gold = np.load(os.path.join(golden_dir, "shell_curl_lhs.npz"))
    world, ts = 2, "RK222"
    with tempfile.TemporaryDirectory() as tmp:
        port = 29500 + (os.getpid() % 2000)
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world),
               "--master-addr", "127.0.0.1", "--master-port", str(port),
               os.path.join(ROOT, "tests", "shell_curl_lhs_mp_worker.py"), tmp, ts]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=dict(os.environ, OMP_NUM_THREADS="1"))
        assert r.returncode == 0, r.stderr[-3000:]
        parts = [np.load(os.path.join(tmp, "rank%d.npz" % k)) for k in range(world)]
    for key in ("B", "tau_1", "tau_2"):
        ref = gold["%s/%s" % (ts, key)]
        full = np.concatenate([p[key] for p in parts], axis=ref.ndim - 3)      # the packed azimuthal axis is distributed
        assert full.shape == ref.shape, (key, full.shape, ref.shape)
        err = float(np.linalg.norm((full - ref).ravel()) / np.linalg.norm(ref.ravel()))
        print("sharded %s %s: %.2e" % (ts, key, err))
        assert err <= TOL, (key, err)
