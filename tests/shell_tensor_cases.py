"""Cases of the shell transpose and radial component (tests/test_shell_tensor_ops.py, tests/test_gpu_shell_tensor_ops.py,
tools/make_golden_shell_tensor_ops.py -> tests/golden/shell_tensor_ops.npz, shell_tensor_volume.npz), and the kernel-level cases that pin
ddh_ell_mix_apply (csrc/ddh_ellmix.hip) at the edges of its launch shape.

Launch shape of the kernel: one workgroup = 8 consecutive (m, part) slots of one ell; along a line 8 / 16 / 32 threads for
<= 8 / <= 16 / more units, a unit being 16 bytes (two radial modes) when nr is even and both buffers are 16-byte aligned and
one mode otherwise; 4 output components at a time.  Hence the edges: 2 nm = 8 | 10; nr = 16 | 18 and 32 | 34 (even: units of
two), nr = 7 | 9 and 15 | 17 (odd: units of one), nr even with a buffer that is only 8-byte aligned; more units than
threads (nr = 66 even, 35 odd); ncomp_out = 4 | 5 and the transpose's 9."""
import numpy as np

RADII = (0.7, 1.9)
DEALIAS = 3 / 2

# full-spectrum random vector u, ShellBasis shapes (Nphi, Ntheta, Nr)
OP_SHAPES = [
    (8, 4, 6),        # one slot group, fewer radii than a wavefront
    (20, 10, 9),      # a half-empty last slot group, odd Nr, ell range no multiple of any tile
    (32, 16, 12),
    (8, 4, 64),
    (8, 4, 65),
]
# tasks the reference evaluates itself ...
REF_TASKS = ("trans_grad", "strain", "trace_trans_grad", "radial_u_inner", "radial_strain_outer", "angular_u_inner",
             "stress_outer")
# ... and radial components of shell (volume) operands.  The reference defines RadialComponent on surface operands only
# (S2RadialComponent, basis_type = SphereBasis): for these the fixture holds the coefficients of the reference's own
# coordinate component, the field whose grid data is operand['g'][..., 2, ...] at the index taken.
VOLUME_TASKS = ("radial_u", "radial_grad_0", "radial_grad_1")


def tag(shape):
    return "%dx%dx%d" % tuple(shape)


def build(d3, shape, dist_kw=None):
    coords = d3.SphericalCoordinates("phi", "theta", "r")
    dist = d3.Distributor(coords, dtype=np.float64, **(dist_kw or {}))
    shell = d3.ShellBasis(coords, shape=shape, radii=RADII, dealias=DEALIAS, dtype=np.float64)
    u = dist.VectorField(coords, name="u", bases=shell)
    return coords, dist, shell, u


def ref_tasks(d3, u):
    strain = d3.grad(u) + d3.trans(d3.grad(u))
    return dict(trans_grad=d3.trans(d3.grad(u)), strain=strain, trace_trans_grad=d3.trace(d3.trans(d3.grad(u))),
                radial_u_inner=d3.radial(u(r=RADII[0])), radial_strain_outer=d3.radial(strain(r=RADII[1]), 0),
                angular_u_inner=d3.angular(u(r=RADII[0])), stress_outer=d3.angular(d3.radial(strain(r=RADII[1]), 0), 0))


def volume_tasks(d3, u):
    return dict(radial_u=d3.radial(u), radial_grad_0=d3.radial(d3.grad(u), 0), radial_grad_1=d3.radial(d3.grad(u), 1))


def volume_operands(d3, u):
    """task -> (operand, index whose radial component is taken): what the fixture generator slices on the grid"""
    return dict(radial_u=(u, 0), radial_grad_0=(d3.grad(u), 0), radial_grad_1=(d3.grad(u), 1))


def with_mix(executor_cls):
    """The NumPy oracle executor with the component mix in NumPy: per slot its row of scalars, the identity along n."""
    class _Mix(executor_cls):
        def make_ell_mix(self, nm, nl, nr, ncomp_out, ncomp_in, terms, slot_map=None):
            if slot_map is None:
                i1, ell = np.indices((2 * nm, nl))
                slot_map = np.where(i1 // 2 <= ell, ell, -1)
            sm = np.asarray(slot_map)
            live = sm >= 0

            class _Terms:
                def apply(self_, x, y):
                    out = np.zeros((ncomp_out, 2 * nm, nl, nr))
                    xs = np.where(live[None, :, :, None], np.asarray(x), 0.0)
                    for (co, ci, q) in terms:
                        out[co] += np.asarray(q)[np.where(live, sm, 0)][:, :, None] * xs[ci]
                    y[...] = out * live[None, :, :, None]
            return _Terms()
    return _Mix()


# ---- kernel-level cases: (label, nm, nl, nr, ncomp_out, ncomp_in, misalign, holes)
# misalign: the buffers start 8 bytes off a 16-byte boundary; holes: slots whose slot_map is -1 besides ell < m
KERNEL_CASES = [
    ("slots8", 4, 5, 6, 3, 3, False, ((1, 0),)),              # (1, 0): the msin part of m = 0
    ("slots10", 5, 6, 6, 3, 3, False, ((1, 0), (3, 4))),
    ("nr16", 2, 3, 16, 3, 3, False, ()),
    ("nr18", 2, 3, 18, 3, 3, False, ((1, 0), (2, 2))),
    ("nr32", 2, 3, 32, 3, 3, False, ()),
    ("nr34", 2, 3, 34, 3, 3, False, ()),
    ("nr7", 2, 3, 7, 3, 3, False, ()),
    ("nr9", 2, 3, 9, 3, 3, False, ((1, 0),)),
    ("nr15", 2, 3, 15, 3, 3, False, ()),
    ("nr17", 2, 3, 17, 3, 3, False, ()),
    ("nr66_loop", 1, 2, 66, 3, 3, False, ((1, 1),)),
    ("nr35_loop", 1, 2, 35, 3, 3, False, ((1, 0),)),
    ("nr16_unaligned", 2, 3, 16, 3, 3, True, ((1, 1),)),
    ("co4", 3, 4, 10, 4, 3, False, ()),
    ("co5_extra_ids", 3, 4, 10, 5, 2, False, ((4, 3),)),
    ("co9_transpose", 3, 4, 12, 9, 9, False, ((1, 0),)),
    ("co1_select", 5, 7, 5, 1, 3, False, ((1, 0),)),
]


def kernel_case(label):
    """-> nm, nl, nr, nco, nci, terms [(co, ci, q [nq])], slot_map, x (NaN in every slot without a mode), misalign"""
    (_, nm, nl, nr, nco, nci, misalign, holes), = [c for c in KERNEL_CASES if c[0] == label]
    rng = np.random.default_rng(sum(map(ord, label)))
    nq = nl + (2 if "extra" in label else 0)
    i1, ell = np.indices((2 * nm, nl))
    slot_map = np.where(i1 // 2 <= ell, ell, -1).astype(np.int32)
    if "extra" in label:                      # slots of one group with rows of their own
        slot_map[2, 2] = nl
        slot_map[3, 3] = nl + 1
    for (a, b) in holes:
        slot_map[a, b] = -1
    terms = []
    for co in range(nco):
        for ci in range(nci):
            if co == nco - 1 and nco == 5:
                continue                                       # an output component without terms: +0 everywhere
            if rng.random() < 0.6 or ci == co % nci:
                terms.append((co, ci, rng.standard_normal(nq)))
    x = rng.standard_normal((nci, 2 * nm, nl, nr))
    x[:, slot_map < 0, :] = np.nan
    return nm, nl, nr, nco, nci, terms, slot_map, x, misalign


def kernel_reference(nm, nl, nr, nco, terms, slot_map, x):
    """longdouble evaluation of the same mix -> (y, sum |q| |x|, largest number of terms of one output component)"""
    LD = np.longdouble
    live = slot_map >= 0
    xs = np.where(np.isnan(x), 0.0, x).astype(LD)
    y = np.zeros((nco, 2 * nm, nl, nr), LD)
    mag = np.zeros_like(y)
    count = np.zeros(nco, np.int64)
    for (co, ci, q) in terms:
        qs = np.asarray(q).astype(LD)[np.where(live, slot_map, 0)][:, :, None]
        y[co] += qs * xs[ci]
        mag[co] += np.abs(qs) * np.abs(xs[ci])
        count[co] += 1
    y *= live[None, :, :, None]
    return y, mag, int(count.max())


# ---- solver cases with stress-free walls: radial(u(r=R)) = 0 and angular(radial(strain(r=R), 0), 0) = 0
SOLVER_SHAPE = (16, 8, 8)
IVP_STEPS, IVP_DT = 5, 0.02


def stressfree_lbvp(d3, dist_kw=None, shape=SOLVER_SHAPE):
    """Vector Poisson problem div(grad(u)) + tau terms = f in the first-order tau formulation of the shell problems
    (tests/problems.py::shell_convection): stress-free inner wall, no-slip outer wall.  No null mode: the outer wall pins
    rigid rotation.  f is set by the caller (coefficients from the fixture)."""
    Ri, Ro = RADII
    coords, dist, shell, u = build(d3, shape, dist_kw)
    f = dist.VectorField(coords, name="f", bases=shell)
    sphere = shell.outer_surface
    tau_u1 = dist.VectorField(coords, name="tau_u1", bases=sphere)
    tau_u2 = dist.VectorField(coords, name="tau_u2", bases=sphere)
    r = dist.local_grids(shell)[2]
    rvec = dist.VectorField(coords, bases=shell.radial_basis)
    rvec["g"][2] = r
    lift_basis = shell.derivative_basis(1)
    lift = lambda A: d3.Lift(A, lift_basis, -1)
    grad_u = d3.grad(u) + rvec * lift(tau_u1)
    strain = d3.grad(u) + d3.trans(d3.grad(u))
    radial, angular = d3.radial, d3.angular
    problem = d3.LBVP([u, tau_u1, tau_u2], namespace=locals())
    problem.add_equation("div(grad_u) + lift(tau_u2) = f")
    problem.add_equation("radial(u(r=Ri)) = 0")
    problem.add_equation("angular(radial(strain(r=Ri), 0), 0) = 0")
    problem.add_equation("u(r=Ro) = 0")
    return problem.build_solver(), dict(u=u, tau_u1=tau_u1, tau_u2=tau_u2, f=f)


def stressfree_convection(d3, timestepper, dist_kw=None, shape=SOLVER_SHAPE):
    """tests/problems.py::shell_convection (the reference's examples/ivp_shell_convection) with stress-free walls on both
    sides; pressure gauge and the ell = 0 system as there.  Rigid rotation is a null mode of L with these walls and the
    reference leaves it undetermined; in the IVP both sides step the same regular systems M + dt L, in which the mode is
    carried by dt(u): it stays at the (zero) value of the initial state, nothing is projected out on either side."""
    Ri, Ro = 14, 15
    Rayleigh, Prandtl = 3500, 1
    coords = d3.SphericalCoordinates('phi', 'theta', 'r')
    dist = d3.Distributor(coords, dtype=np.float64, **(dist_kw or {}))
    shell = d3.ShellBasis(coords, shape=shape, radii=(Ri, Ro), dealias=DEALIAS, dtype=np.float64)
    sphere = shell.outer_surface
    p = dist.Field(name='p', bases=shell)
    b = dist.Field(name='b', bases=shell)
    u = dist.VectorField(coords, name='u', bases=shell)
    tau_p = dist.Field(name='tau_p')
    tau_b1 = dist.Field(name='tau_b1', bases=sphere)
    tau_b2 = dist.Field(name='tau_b2', bases=sphere)
    tau_u1 = dist.VectorField(coords, name='tau_u1', bases=sphere)
    tau_u2 = dist.VectorField(coords, name='tau_u2', bases=sphere)
    kappa = (Rayleigh * Prandtl) ** (-1 / 2)
    nu = (Rayleigh / Prandtl) ** (-1 / 2)
    phi, theta, r = dist.local_grids(shell)
    er = dist.VectorField(coords, bases=shell.radial_basis)
    er['g'][2] = 1
    rvec = dist.VectorField(coords, bases=shell.radial_basis)
    rvec['g'][2] = r
    lift_basis = shell.derivative_basis(1)
    lift = lambda A: d3.Lift(A, lift_basis, -1)
    grad_u = d3.grad(u) + rvec * lift(tau_u1)
    grad_b = d3.grad(b) + rvec * lift(tau_b1)
    strain = d3.grad(u) + d3.trans(d3.grad(u))
    radial, angular = d3.radial, d3.angular
    problem = d3.IVP([p, b, u, tau_p, tau_b1, tau_b2, tau_u1, tau_u2], namespace=locals())
    problem.add_equation("trace(grad_u) + tau_p = 0")
    problem.add_equation("dt(b) - kappa*div(grad_b) + lift(tau_b2) = - u@grad(b)")
    problem.add_equation("dt(u) - nu*div(grad_u) + grad(p) - b*er + lift(tau_u2) = - u@grad(u)")
    problem.add_equation("b(r=Ri) = 1")
    problem.add_equation("radial(u(r=Ri)) = 0")
    problem.add_equation("angular(radial(strain(r=Ri), 0), 0) = 0")
    problem.add_equation("b(r=Ro) = 0")
    problem.add_equation("radial(u(r=Ro)) = 0")
    problem.add_equation("angular(radial(strain(r=Ro), 0), 0) = 0")
    problem.add_equation("integ(p) = 0")
    solver = problem.build_solver(getattr(d3, timestepper))
    b.fill_random('g', seed=42, distribution='normal', scale=1e-3)       # a full-spectrum perturbation
    b['g'] *= (r - Ri) * (Ro - r)
    b['g'] += (Ri - Ri * Ro / r) / (Ri - Ro)
    return solver, dict(p=p, b=b, u=u, tau_p=tau_p, tau_b1=tau_b1, tau_b2=tau_b2, tau_u1=tau_u1, tau_u2=tau_u2)


def run_stressfree_convection(d3, timestepper, dist_kw=None):
    solver, f = stressfree_convection(d3, timestepper, dist_kw)
    for _ in range(IVP_STEPS):
        solver.step(IVP_DT)
    res = {}
    for k, fld in f.items():
        if hasattr(fld, "change_scales"):
            fld.change_scales(1)
        res[k] = np.array(fld['c'] if k != "tau_p" else fld['g'])
    return solver, res, tau_term_scales(d3, f)


def tau_term_scales(d3, f):
    """tau variable -> (factor, scale): a tau enters its equation as factor * lift(tau), and lift() puts the (orthogonally
    recombined) coefficients of tau into one radial mode, so an error d in the coefficients of tau is an error
    factor * |d| in that equation; scale is the coefficient norm of the largest term of that equation in the end state
    (the tau term included).  Equations of stressfree_convection: grad_b = grad(b) + rvec*lift(tau_b1), likewise grad_u
    (|rvec| <= Ro = 15); dt(b) - kappa*div(grad_b) + lift(tau_b2) = - u@grad(b); the momentum equation with nu*div(grad_u),
    grad(p), b*er (a unit vector: the norm of b), lift(tau_u2), u@grad(u)."""
    Ro, kappa, nu = 15.0, 3500 ** (-1 / 2), 3500 ** (-1 / 2)
    norm = lambda x: float(np.linalg.norm(np.array((x.evaluate() if hasattr(x, "evaluate") else x)["c"]).ravel()))
    p, b, u = f["p"], f["b"], f["u"]
    return dict(
        tau_b1=(Ro, max(norm(d3.grad(b)), Ro * norm(f["tau_b1"]))),
        tau_u1=(Ro, max(norm(d3.grad(u)), Ro * norm(f["tau_u1"]))),
        tau_b2=(1.0, max(kappa * norm(d3.lap(b)), norm(f["tau_b2"]), norm(u @ d3.grad(b)))),
        tau_u2=(1.0, max(nu * norm(d3.lap(u)), norm(d3.grad(p)), norm(b), norm(f["tau_u2"]), norm(u @ d3.grad(u)))))
