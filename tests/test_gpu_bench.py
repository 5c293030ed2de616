"""GPU: a plain `bench.py` run times exactly --steps steps once, prints the headline keys only, and --dump-outputs
writes the state its last timed step computed -- the same state the solver reaches when stepped here directly."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("b", "p", "tau_b1", "tau_b2", "tau_u1", "tau_u2", "u")


def test_plain_run_times_its_steps_and_dumps_the_end_state(tmp_path):
    steps, warmup = 3, 2
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--size", "32,32,16", "--steps", str(steps),
           "--warmup", str(warmup), "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == steps and line["warmup"] == warmup and line["repeats"]["n"] == 1
    assert line["unit"] == "timesteps/sec" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert abs(line["ms_per_step"] * line["value"] - 1e3) < 1e-9
    assert not {"roofline", "kernels", "parity", "cfl_mode", "cpu_baseline", "checksum_b_c_l2"} & set(line)
    assert sorted(os.listdir(tmp_path)) == sorted(n + ".npy" for n in FIELDS)

    import problems
    import dedalus_amd.public as d3
    solver, fields = problems.rayleigh_benard_3d(d3, Nx=32, Ny=32, Nz=16, timestepper="RK222")
    for _ in range(warmup + steps):
        solver.step(1e-3)
    for name in FIELDS:
        got = np.load(os.path.join(tmp_path, name + ".npy"))
        want = np.asarray(fields[name]["c"]).ravel()
        assert got.dtype == np.float64 and got.shape == want.shape, name
        assert np.linalg.norm(got - want) <= 1e-12 * max(np.linalg.norm(want), 1e-300), name
