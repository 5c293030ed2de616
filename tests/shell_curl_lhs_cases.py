"""Cases of the curl on a shell left-hand side (tests/test_shell_curl_lhs.py, tests/test_gpu_shell_curl_lhs.py,
tests/test_shell_curl_lhs_sharded.py, tools/make_golden_shell_curl_lhs.py -> tests/golden/shell_curl_lhs.npz).

Every problem function takes the namespace `d3`: the reference's (fixture generator) or this package's (tests), same text.
Radii, dealias, solver shape, steps and dt are those of tests/shell_ellproduct_cases.py.

    grad_B = grad(B) + rvec*lift(tau_1)
    -div(grad_B) - lam*curl(B) + lift(tau_2) = J                               (LBVP: a Beltrami-like solve)
    dt(B) - eta*div(grad_B) - alpha*curl(B) + lift(tau_2) = cross(u0, B)       (IVP: an alpha^2 mean-field dynamo)
    B(r=Ri) = 0,  B(r=Ro) = 0

The curl is a lower-order term, so the walls stay well posed; lam and alpha are order one and away from the eigenvalues of
the curl between these walls (tools/make_golden_shell_curl_lhs.py asserts cond < 1e8 for every ell of the reference's
matrices)."""
import numpy as np

import shell_ellproduct_cases as se

RADII, DEALIAS, SOLVER_SHAPE = se.RADII, se.DEALIAS, se.SOLVER_SHAPE
IVP_STEPS, IVP_DT, ETA = se.IVP_STEPS, se.IVP_DT, se.ETA
LAM, ALPHA = 0.7, 1.3
VARIABLES = ("B", "tau_1", "tau_2")
band_limited_flow = se.band_limited_flow


def _problem(d3, kind, dist_kw, shape, wall_curl=False):
    Ri, Ro = RADII
    coords = d3.SphericalCoordinates("phi", "theta", "r")
    dist = d3.Distributor(coords, dtype=np.float64, **(dist_kw or {}))
    shell = d3.ShellBasis(coords, shape=shape, radii=RADII, dealias=DEALIAS, dtype=np.float64)
    sphere = shell.outer_surface
    B = dist.VectorField(coords, name="B", bases=shell)
    tau_1 = dist.VectorField(coords, name="tau_1", bases=sphere)
    tau_2 = dist.VectorField(coords, name="tau_2", bases=sphere)
    J = dist.VectorField(coords, name="J", bases=shell)
    u0 = dist.VectorField(coords, name="u0", bases=shell)
    eta, lam, alpha = ETA, LAM, ALPHA
    rvec = dist.VectorField(coords, bases=shell.radial_basis)
    rvec["g"][2] = dist.local_grids(shell)[2]
    lift_basis = shell.derivative_basis(1)
    lift = lambda X: d3.Lift(X, lift_basis, -1)
    grad_B = d3.grad(B) + rvec * lift(tau_1)
    cross, curl = d3.cross, d3.curl
    ns = dict(locals())
    problem = (d3.LBVP if kind == "lbvp" else d3.IVP)([B, tau_1, tau_2], namespace=ns)
    if kind == "lbvp":
        problem.add_equation("-div(grad_B) - lam*curl(B) + lift(tau_2) = J")
    else:
        problem.add_equation("dt(B) - eta*div(grad_B) - alpha*curl(B) + lift(tau_2) = cross(u0, B)")
    problem.add_equation("B(r=Ri) = 0")
    if wall_curl:       # (refusal case of the band plan: a curl in a boundary row makes that row complex)
        problem.add_equation("B(r=Ro) + curl(B)(r=Ro) = 0")
    else:
        problem.add_equation("B(r=Ro) = 0")
    return problem, dist, shell, dict(B=B, tau_1=tau_1, tau_2=tau_2, J=J, u0=u0)


def beltrami_lbvp(d3, dist_kw=None, shape=SOLVER_SHAPE):
    problem, dist, shell, f = _problem(d3, "lbvp", dist_kw, shape)
    return problem.build_solver(), f


def alpha2_dynamo(d3, timestepper, dist_kw=None, shape=SOLVER_SHAPE, wall_curl=False):
    problem, dist, shell, f = _problem(d3, "ivp", dist_kw, shape, wall_curl)
    solver = problem.build_solver(getattr(d3, timestepper))
    band_limited_flow(dist, shell, f["u0"])
    return solver, f


def set_initial(f, B0):
    B0 = np.asarray(B0, dtype=np.float64)
    size = getattr(f["B"].dist, "size", 1)
    if size > 1:                                  # m-sharded: this rank's block of the packed azimuthal axis
        n = B0.shape[1] // size
        B0 = B0[:, f["B"].dist.rank * n:(f["B"].dist.rank + 1) * n]
    f["B"]["c"] = B0


def run_alpha2_dynamo(d3, timestepper, B0, dist_kw=None, steps=IVP_STEPS, shape=SOLVER_SHAPE, before=None):
    solver, f = alpha2_dynamo(d3, timestepper, dist_kw, shape)
    set_initial(f, B0)
    if before is not None:
        before(solver)
    for _ in range(steps):
        solver.step(IVP_DT)
    return solver, f, end_state(f)


def end_state(f):
    res = {}
    for k in VARIABLES:
        f[k].change_scales(1)
        res[k] = np.array(f[k]["c"])
    return res


def tau_term_scales(d3, f, eta, coef, Ro=RADII[1]):
    """tau variable -> (factor, scale): the measure of shell_ellproduct_cases.tau_term_scales written for these equations.
    grad_B = grad(B) + rvec*lift(tau_1) with |rvec| <= Ro; the induction equation with eta*div(grad_B), coef*curl(B),
    lift(tau_2) and cross(u0, B) (eta = 1, coef = lam and no cross product in the LBVP)."""
    norm = lambda x: float(np.linalg.norm(np.array((x.evaluate() if hasattr(x, "evaluate") else x)["c"]).ravel()))
    B = f["B"]
    terms = [eta * norm(d3.lap(B)), abs(coef) * norm(d3.curl(B)), norm(f["tau_2"])]
    if np.abs(np.array(f["u0"]["c"])).max() > 0:
        terms.append(norm(d3.cross(f["u0"], B)))
    return dict(tau_1=(Ro, max(norm(d3.grad(B)), Ro * norm(f["tau_1"]))), tau_2=(1.0, max(terms)))


# ell = 1, a middle one and the largest that has a subproblem in the reference at SOLVER_SHAPE: its real-form L block of B
# is stored
MATRIX_ELLS = (1, 3, 6)


def real_form(A):
    """complex (n, n) acting on cos + i msin -> the (2 n, 2 n) matrix on [.., part, ..] with part the slower index of a pair
    (row (i, p), column (j, q)): i (c + i s) = -s + i c"""
    n = A.shape[0]
    out = np.zeros((n, 2, n, 2))
    out[:, 0, :, 0] = out[:, 1, :, 1] = A.real
    out[:, 0, :, 1] = -A.imag
    out[:, 1, :, 0] = A.imag
    return out.reshape(2 * n, 2 * n)


# ---- the NumPy oracle executor with complex per-ell systems ------------------------------------------------------------
def oracle_executor():
    """oracle.np_executor.NumpyExecutor with the component mix, rotated terms, complex_ell_systems = True, the complex dense
    inverse applied as real + rotated blocks, and a NumPy band solve (EllBandPlan.reference_solve: LAPACK gbtrf / gbtrs on
    the plan's bands, complex when the plan is)."""
    import shell_tensor_cases as st
    import shell_vector_cases as sv
    from oracle.np_executor import NumpyExecutor
    base = type(sv.with_rot(type(st.with_mix(NumpyExecutor))))

    class _CurlLhs(base):
        complex_ell_systems = True

        def make_ell_terms_from_dense(self, nm, nl, nr, ncomp, mats, old=None, complex_=False):
            if not complex_:
                return super().make_ell_terms_from_dense(nm, nl, nr, ncomp, mats, old=old)
            inv = np.array(mats)
            blocks, rot = [], []
            for part, arr in ((0, inv.real), (1, inv.imag)):
                for co in range(ncomp):
                    for ci in range(ncomp):
                        blk = arr[:, co * nr:(co + 1) * nr, ci * nr:(ci + 1) * nr]
                        if np.any(blk != 0):
                            blocks.append((co, ci, np.ascontiguousarray(blk)))
                            rot.append(part)
            return self.make_ell_terms(nm, nl, nr, ncomp, blocks, rot=rot)

        def make_ell_band(self, plan, ncomp, nslots, nl, nr, slot_limit, offsets=None):
            assert offsets is None
            ex = self

            class _Band:
                count = 0
                cx = bool(plan.cx)

                def __init__(self_):
                    self_.ab = {}

                def factor(self_, a, b, index=None):
                    index = self_.count if index is None else index
                    self_.ab[index] = (a, b)
                    self_.count = max(self_.count, index + 1)
                    return index

                def solve(self_, index, rhs, x):
                    a, b = self_.ab[index]
                    r4, x4 = np.asarray(rhs).reshape(ncomp, nslots, nl, nr), np.asarray(x).reshape(ncomp, nslots, nl, nr)
                    for g in plan.per:
                        k = int(slot_limit[g])
                        if k == 0:
                            continue
                        flat = r4[:, :k, g, :].transpose(0, 2, 1).reshape(ncomp * nr, k)
                        if plan.cx:
                            out = plan.reference_solve(g, a, b, flat[:, 0::2] + 1j * flat[:, 1::2])
                            sol = np.empty_like(flat)
                            sol[:, 0::2], sol[:, 1::2] = out.real, out.imag
                        else:
                            sol = plan.reference_solve(g, a, b, flat)
                        # (only the columns the plan names are written, as the device kernels do)
                        cols = plan.col_index[g, :int(plan.n[g])]
                        tgt = x4[:, :k, g, :].transpose(0, 2, 1).reshape(ncomp * nr, k).copy()
                        tgt[cols] = sol[cols]
                        x4[:, :k, g, :] = tgt.reshape(ncomp, nr, k).transpose(0, 2, 1)
            return _Band()

        def dense_group_solve(self, inv, rhs4, x4, g, complex_=False):
            R, S, _, nr = rhs4.shape
            v = np.asarray(rhs4)[:, :, g, :].transpose(0, 2, 1).reshape(R * nr, S)
            A = np.asarray(inv).reshape(R * nr, R * nr)
            if complex_:
                y = A @ (v[:, 0::2] + 1j * v[:, 1::2])
                out = np.empty_like(v)
                out[:, 0::2], out[:, 1::2] = y.real, y.imag
            else:
                out = A @ v
            x4[:, :, g, :] = out.reshape(R, nr, S).transpose(0, 2, 1)
    return _CurlLhs()
