"""Triply periodic problems (three RealFourier bases), shared by the reference run (tools/make_golden_periodic3d.py), the
CPU tests and the GPU tests.  `d3` is the reference package or dedalus_amd.public."""
import numpy as np

LX, LY, LZ = 2 * np.pi, 2 * np.pi, np.pi
NU = 0.05
DEALIAS = 3 / 2
DT = 0.02
STEPS = 6
CFL_STEPS = 20

TG_SHAPES = [(16, 16, 8), (12, 20, 8)]
TG_STEPPERS = ["RK222", "SBDF2", "RK443"]
BOUSSINESQ_SHAPE = (12, 16, 8)
BOUSSINESQ_STEPPERS = ["RK222", "SBDF2"]
LBVP_SHAPE = (12, 20, 8)
MATRIX_GROUPS = [(0, 0), (1, 2), (3, 1)]          # (mx, my) of the pencils whose M and L the golden holds, TG (12, 20, 8)


def _bases(d3, shape, dist_kw):
    coords = d3.CartesianCoordinates('x', 'y', 'z')
    dist = d3.Distributor(coords, dtype=np.float64, **(dist_kw or {}))
    xb = d3.RealFourier(coords['x'], size=shape[0], bounds=(0, LX), dealias=DEALIAS)
    yb = d3.RealFourier(coords['y'], size=shape[1], bounds=(0, LY), dealias=DEALIAS)
    zb = d3.RealFourier(coords['z'], size=shape[2], bounds=(0, LZ), dealias=DEALIAS)
    return coords, dist, (xb, yb, zb)


def tg_velocity(x, y, z):
    """Taylor-Green vortex plus a small band-limited perturbation without any symmetry between the axes."""
    kz = 2 * np.pi / LZ
    u = np.zeros((3,) + np.broadcast(x, y, z).shape)
    u[0] = np.sin(x) * np.cos(y) * np.cos(kz * z)
    u[1] = -np.cos(x) * np.sin(y) * np.cos(kz * z)
    u[0] += 0.05 * np.sin(2 * x + y + 0.3) * np.cos(kz * z + 0.7) + 0.03 * np.cos(y - 2 * kz * z + 0.2)
    u[1] += 0.04 * np.cos(x - 2 * y + 1.1) * np.sin(kz * z + 0.1) + 0.02 * np.sin(3 * x + 0.5)
    u[2] += 0.05 * np.sin(x + 2 * y + 0.4) + 0.03 * np.cos(2 * x - y + kz * z + 0.9)
    return u


def taylor_green(d3, shape=(16, 16, 8), timestepper="RK222", dist_kw=None):
    coords, dist, B = _bases(d3, shape, dist_kw)
    u = dist.VectorField(coords, name='u', bases=B)
    p = dist.Field(name='p', bases=B)
    tau_p = dist.Field(name='tau_p')
    nu = NU
    problem = d3.IVP([u, p, tau_p], namespace=locals())
    problem.add_equation("dt(u) - nu*lap(u) + grad(p) = - u@grad(u)")
    problem.add_equation("div(u) + tau_p = 0")
    problem.add_equation("integ(p) = 0")
    solver = problem.build_solver(getattr(d3, timestepper))
    x, y, z = dist.local_grids(*B)
    u['g'] = tg_velocity(x, y, z)
    return solver, dict(u=u, p=p, tau_p=tau_p)


def boussinesq(d3, shape=BOUSSINESQ_SHAPE, timestepper="RK222", dist_kw=None):
    """Rotating stratified Boussinesq: Coriolis and buoyancy terms on the left-hand side (non-symmetric blocks, a zero
    diagonal in the continuity row)."""
    coords, dist, B = _bases(d3, shape, dist_kw)
    u = dist.VectorField(coords, name='u', bases=B)
    p = dist.Field(name='p', bases=B)
    b = dist.Field(name='b', bases=B)
    tau_p = dist.Field(name='tau_p')
    ex, ey, ez = coords.unit_vector_fields(dist)
    nu, kappa, f, N2 = NU, 0.03, 2.0, 4.0
    problem = d3.IVP([u, p, b, tau_p], namespace=locals())
    problem.add_equation("div(u) + tau_p = 0")
    problem.add_equation("dt(u) - nu*lap(u) + grad(p) + f*cross(ez, u) - b*ez = - u@grad(u)")
    problem.add_equation("dt(b) - kappa*lap(b) + N2*(u@ez) = - u@grad(b)")
    problem.add_equation("integ(p) = 0")
    solver = problem.build_solver(getattr(d3, timestepper))
    x, y, z = dist.local_grids(*B)
    kz = 2 * np.pi / LZ
    u['g'] = 0.5 * tg_velocity(x, y, z)
    b['g'] = 0.3 * np.sin(x - y + 0.2) * np.cos(kz * z + 0.5) + 0.1 * np.cos(2 * y + kz * z)
    return solver, dict(u=u, p=p, b=b, tau_p=tau_p)


def run_ivp(d3, builder, **kw):
    solver, f = builder(d3, **kw)
    start = {k: np.array(v['c']) for k, v in f.items()}
    for _ in range(STEPS):
        solver.step(DT)
    return solver, start, {k: np.array(v['c']) for k, v in f.items()}


def run_cfl(d3, dist_kw=None, nsteps=CFL_STEPS):
    solver, f = taylor_green(d3, (16, 16, 8), "RK222", dist_kw=dist_kw)
    CFL = d3.CFL(solver, initial_dt=0.02, cadence=2, safety=0.4, threshold=0.05, max_change=1.5, min_change=0.5,
                 max_dt=0.1)
    CFL.add_velocity(f["u"])
    dts = []
    for _ in range(nsteps):
        dt = CFL.compute_timestep()
        solver.step(dt)
        dts.append(dt)
    return solver, np.array(dts), {k: np.array(v['c']) for k, v in f.items()}


def poisson_rhs(x, y, z):
    kz = 2 * np.pi / LZ
    return (np.sin(x + 2 * y + 0.3) * np.cos(kz * z + 0.4) + 0.5 * np.cos(3 * x - y + 0.1)
            + 0.25 * np.sin(2 * kz * z + 0.6) * np.cos(y) + 0.0 * x)


def poisson(d3, shape=LBVP_SHAPE, dist_kw=None):
    coords, dist, B = _bases(d3, shape, dist_kw)
    phi = dist.Field(name='phi', bases=B)
    tau = dist.Field(name='tau')
    f = dist.Field(name='f', bases=B)
    x, y, z = dist.local_grids(*B)
    f['g'] = poisson_rhs(x, y, z)
    problem = d3.LBVP([phi, tau], namespace=locals())
    problem.add_equation("lap(phi) + tau = f")
    problem.add_equation("integ(phi) = 0")
    solver = problem.build_solver()
    return solver, dict(phi=phi, tau=tau, f=f)


def run_poisson(d3, dist_kw=None):
    solver, f = poisson(d3, dist_kw=dist_kw)
    solver.solve()
    return solver, {k: np.array(f[k]['c']) for k in ("phi", "tau")}
