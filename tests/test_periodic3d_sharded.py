"""CPU, 2 ranks (gloo): a triply periodic box sharded along kx (coefficients) and along the Fourier pencil axis z (grid)
against the serial run (1e-12) and the reference's end state (1e-10)."""
import os
import subprocess
import sys
import tempfile

import numpy as np

import periodic3d_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_two_ranks_match_serial_and_reference(golden_dir):
    import dedalus_amd.public as d3
    from oracle.np_executor import NumpyExecutor
    gold = np.load(os.path.join(golden_dir, "periodic3d.npz"))
    world, ts = 2, "RK222"
    with tempfile.TemporaryDirectory() as tmp:
        port = 29500 + (os.getpid() % 2000)
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world),
               "--master-addr", "127.0.0.1", "--master-port", str(port),
               os.path.join(ROOT, "tests", "periodic3d_mp_worker.py"), tmp, ts]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=dict(os.environ, OMP_NUM_THREADS="1"))
        assert r.returncode == 0, r.stderr[-3000:]
        parts = [np.load(os.path.join(tmp, "rank%d.npz" % k)) for k in range(world)]
        parts = [{k: p[k] for k in p.files} for p in parts]
    solver, start, serial = pc.run_ivp(d3, pc.taylor_green, shape=(16, 16, 8), timestepper=ts,
                                       dist_kw=dict(executor=NumpyExecutor()))
    for key in ("u", "p"):
        ref = gold["tg/16x16x8/%s/%s" % (ts, key)]
        full = np.concatenate([p[key] for p in parts], axis=ref.ndim - 3)      # the x modes are distributed
        assert full.shape == ref.shape, (key, full.shape, ref.shape)
        scale = np.abs(ref).max()
        e_serial, e_ref = np.abs(full - serial[key]).max() / scale, np.abs(full - ref).max() / scale
        print("sharded %s %s: vs serial %.2e, vs reference %.2e" % (ts, key, e_serial, e_ref))
        assert e_serial <= 1e-12, (key, e_serial)
        assert e_ref <= 1e-10, (key, e_ref)
