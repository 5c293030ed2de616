"""Host-level checks of the CFL NaN policy, shared by tests/test_grid_cases_host.py (NumpyExecutor) and
tests/test_gpu_grid_kernels.py (HIP): with a NaN velocity CFL.compute_timestep() returns the unchanged stored_dt."""
import math

import numpy as np

import problems


def nan_velocity_leaves_dt_unchanged(d3, dist_kw=None):
    """Finite steps first (dt follows the flow), then a NaN in the velocity: the frequency sampled by the next step is NaN,
    the threshold comparison of compute_timestep is false and stored_dt stays (the reference's logic)."""
    solver, f = problems.rayleigh_benard_2d(d3, Nx=32, Nz=16, timestepper="RK222", dist_kw=dist_kw)
    u = f["u"]
    xb, zb = [b for b in u.domain.bases]
    x, z = u.dist.local_grids(xb, zb)
    ug = np.zeros((2,) + np.broadcast(x, z).shape)
    ug[0] = 0.5 * np.sin(2 * np.pi * x / 4) * z * (1 - z) * 4
    ug[1] = 0.3 * np.cos(4 * np.pi * x / 4) * z * (1 - z) * 4
    u["g"] = ug
    cfl = d3.CFL(solver, initial_dt=0.02, cadence=1, safety=0.5, threshold=0.0, max_change=1.5, min_change=0.5, max_dt=0.125)
    cfl.add_velocity(u)
    dts = []
    for _ in range(3):
        dts.append(cfl.compute_timestep())
        solver.step(dts[-1])
    assert dts[0] == dts[1] == 0.02 and dts[2] != 0.02 and math.isfinite(dts[2])   # the finite flow moved dt
    stored = cfl.stored_dt
    ug = np.array(u["g"])
    ug[1, 5, 7] = np.nan
    u["g"] = ug
    solver.step(stored)                                                   # samples the frequency of the NaN velocity
    assert math.isnan(cfl._max_freq)
    assert cfl.compute_timestep() == stored and cfl.stored_dt == stored
    return solver


def nan_shell_velocity_leaves_dt_unchanged(d3, dist_kw=None):
    """The same through the shell's own reduction (Field.cfl_frequency_max -> cfl_max_spherical) and the branch of
    CFL._sample that folds it into the running maximum."""
    solver, f = problems.shell_convection(d3, shape=(16, 12, 8), timestepper="SBDF2", dist_kw=dist_kw)
    u = f["u"]
    phi, theta, r = u.dist.local_grids(problems._shell_basis_of(f["b"]))
    ug = np.zeros((3,) + np.broadcast(phi, theta, r).shape)
    ug[0] = 8.0 * np.sin(theta) * (r - 14) * (15 - r) * 4
    ug[2] = 3.0 * np.cos(theta) * (r - 14) * (15 - r) * 4 + 0 * phi
    u["g"] = ug
    assert u.cfl_frequency_max() > 0
    cfl = d3.CFL(solver, initial_dt=0.006, cadence=1, safety=0.5, threshold=0.0, max_change=1.5, min_change=0.5, max_dt=0.1)
    cfl.add_velocity(u)
    dts = []
    for _ in range(3):
        dts.append(cfl.compute_timestep())
        solver.step(dts[-1])
    assert dts[2] != 0.006 and math.isfinite(dts[2])
    stored = cfl.stored_dt
    ug = np.array(u["g"])
    ug[1, 3, 4, 2] = np.nan
    u["g"] = ug
    assert math.isnan(u.cfl_frequency_max())
    solver.step(stored)
    assert math.isnan(cfl._max_freq)
    assert cfl.compute_timestep() == stored and cfl.stored_dt == stored
    return solver
