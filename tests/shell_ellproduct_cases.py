"""Cases of SphericalEllProduct on the shell and of insulating (potential-field) walls (tests/test_shell_ellproduct.py,
tests/test_gpu_shell_ellproduct.py, tools/make_golden_shell_ellproduct.py -> tests/golden/shell_ellproduct*.npz), and the
diagonal lists that run ddh_ell_mix_apply (csrc/ddh_ellmix.hip) at the edges of its launch shape.

Every function takes the namespace `d3`: the reference's (fixture generator) or this package's (tests), same text."""
import numpy as np

import shell_tensor_cases as st

RADII = st.RADII
DEALIAS = st.DEALIAS
ELL_FUNCS = dict(lp1=lambda ell: ell + 1, neg=lambda ell: -ell, llp1=lambda ell: ell * (ell + 1))

# scalar f, vector u, rank-2 tensor T with full spectra; ShellBasis shapes (Nphi, Ntheta, Nr)
OP_SHAPES = [
    (16, 8, 8),
    (20, 10, 9),      # a half-empty last slot group, odd Nr
    (12, 8, 6),       # Ntheta > Nphi / 2: the packed layout covers some slots with two ell boxes, (1, 3) here
]


def tag(shape):
    return "%dx%dx%d" % tuple(shape)


def build(d3, shape, dist_kw=None):
    coords = d3.SphericalCoordinates("phi", "theta", "r")
    dist = d3.Distributor(coords, dtype=np.float64, **(dist_kw or {}))
    shell = d3.ShellBasis(coords, shape=shape, radii=RADII, dealias=DEALIAS, dtype=np.float64)
    f = dist.Field(name="f", bases=shell)
    u = dist.VectorField(coords, name="u", bases=shell)
    T = dist.TensorField(coords, name="T", bases=shell)
    return coords, dist, shell, dict(s=f, v=u, t=T)


PLAIN_ONLY = [(12, 8, 6)]       # shapes that run the products alone (the interpolation of tensors is not pinned there)


def op_tasks(d3, coords, fields, plain_only=False):
    """name -> expression.  ep_<func>_<operand>: the product itself; ..._ri / ..._ro: interpolated at either radius;
    rg_ep_*: radial(grad(product)(r=Ro)), the product first; ep_rg_*: radial(product(grad)(r=Ro)), the gradient first."""
    Ri, Ro = RADII
    out = {}
    for fn, func in ELL_FUNCS.items():
        ep = lambda X, func=func: d3.SphericalEllProduct(X, coords, func)
        for k, X in fields.items():
            out["ep_%s_%s" % (fn, k)] = ep(X)
            if plain_only:
                continue
            out["ep_%s_%s_ri" % (fn, k)] = ep(X)(r=Ri)
            out["ep_%s_%s_ro" % (fn, k)] = ep(X)(r=Ro)
        for k in () if plain_only else ("s", "v"):
            out["rg_ep_%s_%s" % (fn, k)] = d3.radial(d3.grad(ep(fields[k]))(r=Ro))
            out["ep_rg_%s_%s" % (fn, k)] = d3.radial(ep(d3.grad(fields[k]))(r=Ro))
    return out


# ---- solver cases: vector potential A between two insulators.  Outside r = Ro the field is a potential field that decays,
# inside r = Ri one that is regular: degree by degree d_r A + (l + 1) A / Ro = 0 and d_r A - l A / Ri = 0 on the
# regularity components, l the degree of the component (ell + regtotal): SphericalEllProduct with l + 1 and - l.
SOLVER_SHAPE = (16, 8, 8)
IVP_STEPS, IVP_DT, ETA = 4, 0.01, 0.3
VARIABLES = ("A", "phi", "tau_phi", "tau_A1", "tau_A2")

ellp1 = lambda ell: ell + 1
ellm = lambda ell: -ell


def _potential_problem(d3, kind, dist_kw, shape):
    """The taus enter as in the shell problems of tests/problems.py (first-order formulation: tau_A1 inside the gradient,
    so that it reaches the divergence equation too).  With `-lap(A) + lift(tau_A1, -1) + lift(tau_A2, -2)` and
    `div(A) + tau_phi = 0` the reference's ell = 0 matrix is singular (cond 3e20: the first-order divergence equation
    alone meets both wall conditions there, and the taus sit in the other equation); in this form every ell is regular
    (cond <= 2e4 at SOLVER_SHAPE; tools/make_golden_shell_ellproduct.py asserts it)."""
    Ri, Ro = RADII
    coords = d3.SphericalCoordinates("phi", "theta", "r")
    dist = d3.Distributor(coords, dtype=np.float64, **(dist_kw or {}))
    shell = d3.ShellBasis(coords, shape=shape, radii=RADII, dealias=DEALIAS, dtype=np.float64)
    sphere = shell.outer_surface
    A = dist.VectorField(coords, name="A", bases=shell)
    phi = dist.Field(name="phi", bases=shell)
    tau_phi = dist.Field(name="tau_phi")
    tau_A1 = dist.VectorField(coords, name="tau_A1", bases=sphere)
    tau_A2 = dist.VectorField(coords, name="tau_A2", bases=sphere)
    J = dist.VectorField(coords, name="J", bases=shell)
    u0 = dist.VectorField(coords, name="u0", bases=shell)
    eta = ETA
    rvec = dist.VectorField(coords, bases=shell.radial_basis)
    rvec["g"][2] = dist.local_grids(shell)[2]
    lift_basis = shell.derivative_basis(1)
    lift = lambda X: d3.Lift(X, lift_basis, -1)
    grad_A = d3.grad(A) + rvec * lift(tau_A1)
    SphericalEllProduct, radial, cross, curl = d3.SphericalEllProduct, d3.radial, d3.cross, d3.curl
    ns = dict(locals(), ellp1=ellp1, ellm=ellm)
    problem = (d3.LBVP if kind == "lbvp" else d3.IVP)([A, phi, tau_phi, tau_A1, tau_A2], namespace=ns)
    if kind == "lbvp":
        problem.add_equation("-div(grad_A) + grad(phi) + lift(tau_A2) = J")
    else:
        problem.add_equation("dt(A) - eta*div(grad_A) + grad(phi) + lift(tau_A2) = cross(u0, curl(A))")
    problem.add_equation("trace(grad_A) + tau_phi = 0")
    problem.add_equation("integ(phi) = 0")
    problem.add_equation("radial(grad(A)(r=Ro)) + SphericalEllProduct(A, coords, ellp1)(r=Ro)/Ro = 0")
    problem.add_equation("radial(grad(A)(r=Ri)) + SphericalEllProduct(A, coords, ellm)(r=Ri)/Ri = 0")
    fields = dict(A=A, phi=phi, tau_phi=tau_phi, tau_A1=tau_A1, tau_A2=tau_A2, J=J, u0=u0)
    return problem, dist, shell, fields


def potential_lbvp(d3, dist_kw=None, shape=SOLVER_SHAPE):
    """-lap(A) + grad(phi) = J, div(A) = 0, integ(phi) = 0 with potential-field matching on both walls, in the first-order
    tau formulation (see _potential_problem).  J is set by the caller (coefficients from the fixture)."""
    problem, dist, shell, f = _potential_problem(d3, "lbvp", dist_kw, shape)
    return problem.build_solver(), f


def band_limited_flow(dist, shell, u0):
    """a fixed smooth flow: differential rotation plus a meridional cell and an m = 2 part"""
    phi, theta, r = dist.local_grids(shell)
    Ri, Ro = RADII
    s = (r - Ri) * (Ro - r)
    u0["g"][0] = s * np.sin(theta) * (1 + 0.5 * np.cos(theta) ** 2) + 0.3 * s * np.sin(theta) ** 2 * np.cos(2 * phi)
    u0["g"][1] = 0.4 * s * np.sin(theta) * np.cos(theta) * (1 + 0.5 * np.sin(2 * phi) * np.sin(theta))
    u0["g"][2] = 0.2 * s * (3 * np.cos(theta) ** 2 - 1) * (r - 1.0)


def potential_induction(d3, timestepper, dist_kw=None, shape=SOLVER_SHAPE):
    """dt(A) - eta*lap(A) + grad(phi) + taus = cross(u0, curl(A)) with the same walls; A(t = 0) is set by the caller"""
    problem, dist, shell, f = _potential_problem(d3, "ivp", dist_kw, shape)
    solver = problem.build_solver(getattr(d3, timestepper))
    band_limited_flow(dist, shell, f["u0"])
    return solver, f


def run_potential_induction(d3, timestepper, A0, dist_kw=None, steps=IVP_STEPS):
    solver, f = potential_induction(d3, timestepper, dist_kw)
    A0 = np.asarray(A0, dtype=np.float64)
    size = getattr(f["A"].dist, "size", 1)
    if size > 1:                                  # m-sharded: this rank's block of the packed azimuthal axis
        n = A0.shape[1] // size
        A0 = A0[:, f["A"].dist.rank * n:(f["A"].dist.rank + 1) * n]
    f["A"]["c"] = A0
    for _ in range(steps):
        solver.step(IVP_DT)
    return solver, f, end_state(f)


def end_state(f):
    res = {}
    for k in VARIABLES:
        if hasattr(f[k], "change_scales"):
            f[k].change_scales(1)
        res[k] = np.array(f[k]["c"] if k != "tau_phi" else f[k]["g"])
    return res


def tau_term_scales(d3, f, eta, Ro=RADII[1]):
    """tau variable -> (factor, scale), the measure of tests/shell_tensor_cases.py::tau_term_scales written for the
    equations of this problem (that function lists the terms of the convection problem and cannot be asked about another):
    a tau enters its equation as factor * lift(tau), and lift() puts its coefficients into one radial mode, so an error d
    in tau is an error factor * |d| in that equation; scale is the coefficient norm of the largest term of that equation
    in the state given.  grad_A = grad(A) + rvec*lift(tau_A1) with |rvec| <= Ro; the induction equation with
    eta*div(grad_A), grad(phi), lift(tau_A2) and cross(u0, curl(A)) (eta = 1 and no cross product in the LBVP)."""
    norm = lambda x: float(np.linalg.norm(np.array((x.evaluate() if hasattr(x, "evaluate") else x)["c"]).ravel()))
    A, phi = f["A"], f["phi"]
    terms = [eta * norm(d3.lap(A)), norm(d3.grad(phi)), norm(f["tau_A2"])]
    if np.abs(np.array(f["u0"]["c"])).max() > 0:
        terms.append(norm(d3.cross(f["u0"], d3.curl(A))))
    return dict(tau_A1=(Ro, max(norm(d3.grad(A)), Ro * norm(f["tau_A1"]))), tau_A2=(1.0, max(terms)))


# ---- diagonal lists at the launch-shape edges of ddh_ell_mix_apply (the edges of tests/shell_tensor_cases.py::KERNEL_CASES:
# one workgroup = 8 (m, part) slots of one ell; units of 16 bytes when nr is even, of one mode when it is odd; 8 / 16 / 32
# threads along a line).  (label, nm, nl, nr, ncomp, holes): 2 nm = 8 | 10, nr odd and even on either side of the thread
# counts, more units than threads, a slot without a mode, ncomp = 1, 3 and 9.
DIAG_CASES = [
    ("slots8_c3", 4, 5, 6, 3, ((1, 0),)),
    ("slots10_c3", 5, 6, 6, 3, ((1, 0), (3, 4))),
    ("nr16_c3", 2, 3, 16, 3, ()),
    ("nr18_c3", 2, 3, 18, 3, ((2, 2),)),
    ("nr7_c1", 2, 3, 7, 1, ((1, 0),)),
    ("nr9_c3", 2, 3, 9, 3, ()),
    ("nr34_c1", 2, 3, 34, 1, ()),
    ("nr35_loop_c3", 1, 2, 35, 3, ((1, 0),)),
    ("nr66_loop_c9", 1, 2, 66, 9, ((1, 1),)),
    ("slots10_c9", 5, 6, 12, 9, ((1, 0), (7, 5))),
    ("slots10_c1_odd", 5, 7, 5, 1, ((1, 0),)),
]


def diag_case(label):
    """-> nm, nl, nr, ncomp, terms [(c, c, q [nl])], slot_map, x (NaN in every slot without a mode).  The scalars are those
    of an ell product, ell_func(ell + regtotal) with ell_func = l (l + 1) on the components of a rank-0 / 1 / 2 tensor and 0
    where the component has no mode; a component whose scalars all vanish has no term (ncomp 9 at nl = 2: (-, -))."""
    from dedalus_amd.core.shell import reg_indices, regtotal, regularity_allowed
    (_, nm, nl, nr, nc, holes), = [c for c in DIAG_CASES if c[0] == label]
    rng = np.random.default_rng(sum(map(ord, label)))
    i1, ell = np.indices((2 * nm, nl))
    slot_map = np.where(i1 // 2 <= ell, ell, -1).astype(np.int32)
    for (a, b) in holes:
        slot_map[a, b] = -1
    idx = reg_indices({1: 0, 3: 1, 9: 2}[nc])
    terms = []
    for c, t in enumerate(idx):
        q = np.array([ELL_FUNCS["llp1"](l + regtotal(t)) if regularity_allowed(l, t) else 0.0 for l in range(nl)], dtype=np.float64)
        q *= 1.0 + rng.random(nl)                                 # full mantissas: the product has to be rounded
        if np.any(q != 0):
            terms.append((c, c, q))
    x = rng.standard_normal((nc, 2 * nm, nl, nr))
    x[:, slot_map < 0, :] = np.nan
    return nm, nl, nr, nc, terms, slot_map, x
