"""Adaptive runs under a CFL of several velocities and scalar frequencies, shared by the reference run
(tools/make_golden_cfl_terms.py -> tests/golden/cfl_terms.npz) and tests/test_gpu_cfl_terms.py.  `d3` is the reference
package or dedalus_amd.public; every case returns (solver, dt sequence).  Unless a case says otherwise: 10 steps under
CFL(cadence=1, safety=0.5, max_change=1.5)."""
import numpy as np

import periodic3d_cases as pc
import problems

STEPS = 10
CFL_KW = dict(cadence=1, safety=0.5, max_change=1.5)


def _run(d3, solver, cfl, steps=STEPS):
    dts = []
    for _ in range(steps):
        dt = cfl.compute_timestep()
        solver.step(dt)
        dts.append(dt)
    return solver, np.array(dts)


def _rb(d3, dist_kw):
    """2-D Rayleigh-Benard 64 x 32 with the O(1) flow of problems.run_cfl_case"""
    solver, f = problems.rayleigh_benard_2d(d3, Nx=64, Nz=32, timestepper="RK222", dist_kw=dist_kw)
    u = f["u"]
    xb, zb = u.domain.bases
    x, z = u.dist.local_grids(xb, zb)
    ug = np.zeros((2,) + np.broadcast(x, z).shape)
    ug[0] = 0.5 * np.sin(2 * np.pi * x / 4) * z * (1 - z) * 4
    ug[1] = 0.3 * np.cos(4 * np.pi * x / 4) * z * (1 - z) * 4
    u['g'] = ug
    return solver, f, (xb, zb), (x, z)


def rb_sqrt(d3, dist_kw=None):
    """add_velocity(u) + add_frequency(sqrt(b b)): an expression, evaluated on the grid at every sample"""
    solver, f, _, _ = _rb(d3, dist_kw)
    cfl = d3.CFL(solver, initial_dt=0.01, **CFL_KW)
    cfl.add_velocity(f["u"])
    cfl.add_frequency(np.sqrt(f["b"] * f["b"]))
    return _run(d3, solver, cfl)


def _profile(f, zb, z):
    N = f["u"].dist.Field(name='N', bases=zb)
    N['g'] = 6.0 * (1 + z) ** 2
    return N


def rb_profile(d3, dist_kw=None):
    """add_velocity(u) + add_frequency(N(z)): a field with a basis along z only"""
    solver, f, (xb, zb), (x, z) = _rb(d3, dist_kw)
    cfl = d3.CFL(solver, initial_dt=0.01, **CFL_KW)
    cfl.add_velocity(f["u"])
    cfl.add_frequency(_profile(f, zb, z))
    return _run(d3, solver, cfl)


def rb_no_vertical_basis(d3, dist_kw=None):
    """add_velocity(u) + add_velocity(B), B on the x basis only: its z component has no basis and adds no frequency"""
    solver, f, (xb, zb), (x, z) = _rb(d3, dist_kw)
    u = f["u"]
    B = u.dist.VectorField(u.tensorsig[0], name='B', bases=xb)
    B['g'][0] = 0.6 + 0.4 * np.cos(2 * np.pi * x / 4)
    B['g'][1] = 50.0
    cfl = d3.CFL(solver, initial_dt=0.01, **CFL_KW)
    cfl.add_velocity(u)
    cfl.add_velocity(B)
    return _run(d3, solver, cfl)


GRAPH_STEPS = 14


def rb_profile_capped(d3, dist_kw=None):
    """rb_profile with cadence 3 and max_dt below the CFL limit: the timestep climbs to the cap and stays, so that the steps
    between two samples can be replayed from a captured graph (a sample reads the velocity on the grid, which makes
    that one step an ordinary one)."""
    solver, f, (xb, zb), (x, z) = _rb(d3, dist_kw)
    cfl = d3.CFL(solver, initial_dt=0.004, cadence=3, safety=0.5, max_change=1.5, max_dt=0.006)
    cfl.add_velocity(f["u"])
    cfl.add_frequency(_profile(f, zb, z))
    return _run(d3, solver, cfl, GRAPH_STEPS)


def box_two_velocities(d3, dist_kw=None):
    """Triply periodic 16^3 box: Taylor-Green flow u and a vector A it advects; add_velocity(u) + add_velocity(A)"""
    coords, dist, B = pc._bases(d3, (16, 16, 16), dist_kw)
    u = dist.VectorField(coords, name='u', bases=B)
    A = dist.VectorField(coords, name='A', bases=B)
    p = dist.Field(name='p', bases=B)
    tau_p = dist.Field(name='tau_p')
    nu, eta = pc.NU, 0.04
    problem = d3.IVP([u, A, p, tau_p], namespace=locals())
    problem.add_equation("dt(u) - nu*lap(u) + grad(p) = - u@grad(u)")
    problem.add_equation("dt(A) - eta*lap(A) = - u@grad(A)")
    problem.add_equation("div(u) + tau_p = 0")
    problem.add_equation("integ(p) = 0")
    solver = problem.build_solver(d3.RK222)
    x, y, z = dist.local_grids(*B)
    u['g'] = pc.tg_velocity(x, y, z)
    A['g'] = 0.7 * pc.tg_velocity(y + 0.4, z * 2 + 0.1, x / 2 + 0.3)
    cfl = d3.CFL(solver, initial_dt=0.02, **CFL_KW)
    cfl.add_velocity(u)
    cfl.add_velocity(A)
    return _run(d3, solver, cfl)


def shell_profile(d3, dist_kw=None):
    """Shell convection (16, 12, 8) with the O(1) flow of problems.run_shell_cfl_case: add_velocity(u) + add_frequency
    of a field on the radial basis"""
    solver, f = problems.shell_convection(d3, shape=(16, 12, 8), timestepper="SBDF2", dist_kw=dist_kw)
    u = f["u"]
    dist = u.dist
    shell = problems._shell_basis_of(f["b"])
    phi, theta, r = dist.local_grids(shell)
    ug = np.zeros((3,) + np.broadcast(phi, theta, r).shape)
    ug[0] = 8.0 * np.sin(theta) * (r - 14) * (15 - r) * 4
    ug[1] = 5.0 * np.sin(theta) * np.cos(phi) * (r - 14) * (15 - r) * 4
    ug[2] = 3.0 * np.cos(theta) * (r - 14) * (15 - r) * 4
    u['g'] = ug
    N = dist.Field(name='N', bases=shell.radial_basis)
    N['g'] = 20.0 * (1 + (r - 14) ** 2)
    cfl = d3.CFL(solver, initial_dt=0.004, **CFL_KW)
    cfl.add_velocity(u)
    cfl.add_frequency(N)
    return _run(d3, solver, cfl)


def sphere_velocity(d3, dist_kw=None):
    """Shallow water on the sphere 32 x 16: add_velocity(u) of an S2 vector"""
    solver, f, extra = problems.shallow_water(d3, Nphi=32, Ntheta=16, timestepper="RK222", dist_kw=dist_kw)
    cfl = d3.CFL(solver, initial_dt=extra["timestep"], **CFL_KW)
    cfl.add_velocity(f["u"])
    return _run(d3, solver, cfl)


CASES = dict(rb_sqrt=rb_sqrt, rb_profile=rb_profile, rb_no_vertical_basis=rb_no_vertical_basis,
             rb_profile_capped=rb_profile_capped, box_two_velocities=box_two_velocities, shell_profile=shell_profile,
             sphere_velocity=sphere_velocity)
