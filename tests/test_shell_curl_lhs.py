"""The curl on a shell left-hand side on the NumPy oracle executor (no GPU): the assembled per-ell matrices against the
reference's real-form matrices, the LBVP solution and both IVP end states against tests/golden/shell_curl_lhs.npz (written
by tools/make_golden_shell_curl_lhs.py), the complex band plan, the unchanged real plan of a curl-free problem and the
refusals.

Bounds: matrices entry by entry to 1e-12 of the largest entry of that ell (the bound of tests/test_shell_ellproduct.py);
solutions and end states to the project's 1e-10: fields in their own norm, a tau variable as the error of its term against
the largest term of its equation (shell_curl_lhs_cases.tau_term_scales).
The boundary condition with a curl used for the "complex boundary rows" refusal is `B(r=Ro) + curl(B)(r=Ro) = 0`."""
import os

import numpy as np
import pytest

import shell_curl_lhs_cases as sc
import shell_ellproduct_cases as se
from test_shell_tensor_ops import rel_l2

HERE = os.path.dirname(os.path.abspath(__file__))
TOL = 1e-10


def oracle_kw():
    return dict(executor=sc.oracle_executor())


def gold():
    return np.load(os.path.join(HERE, "golden", "shell_curl_lhs.npz"))


def variable_errors(d3, f, res, ref, eta, coef):
    scales = sc.tau_term_scales(d3, f, eta, coef)
    own = {k: rel_l2(res[k], ref[k]) for k in ref}
    errs = {k: (scales[k][0] * float(np.linalg.norm((res[k] - ref[k]).ravel())) / scales[k][1] if k in scales else own[k])
            for k in own}
    return errs, own


def check_lbvp(dist_kw):
    import dedalus_amd.public as d3
    GOLD = gold()
    solver, f = sc.beltrami_lbvp(d3, dist_kw)
    assert solver.cx
    f["J"]["c"] = GOLD["lbvp/in_J"].astype(np.float64)
    solver.solve()
    res = sc.end_state(f)
    ref = {k: GOLD["lbvp/" + k] for k in sc.VARIABLES}
    errs, own = variable_errors(d3, f, res, ref, 1.0, sc.LAM)
    print("curl-LHS LBVP:", {k: "%.1e" % v for k, v in errs.items()}, "own norm:", {k: "%.1e" % v for k, v in own.items()})
    for k, e in errs.items():
        assert res[k].shape == ref[k].shape
        assert e <= TOL, (k, e)
    return solver


def check_dynamo(ts, dist_kw, before=None):
    import dedalus_amd.public as d3
    GOLD = gold()
    solver, f, res = sc.run_alpha2_dynamo(d3, ts, GOLD["ivp/in_B"], dist_kw, before=before)
    ref = {k: GOLD["%s/%s" % (ts, k)] for k in sc.VARIABLES}
    size = getattr(f["B"].dist, "size", 1)
    if size > 1:
        n = ref["B"].shape[1] // size
        ref = {k: v[:, f["B"].dist.rank * n:(f["B"].dist.rank + 1) * n] for k, v in ref.items()}
    errs, own = variable_errors(d3, f, res, ref, sc.ETA, sc.ALPHA)
    print("alpha^2 dynamo %s:" % ts, {k: "%.1e" % v for k, v in errs.items()}, "own norm:", {k: "%.1e" % v for k, v in own.items()})
    for k, e in errs.items():
        assert res[k].shape == ref[k].shape
        assert e <= TOL, (ts, k, e)
    if size == 1:
        assert rel_l2(res["B"], GOLD["ivp/in_B"].astype(np.float64)) > 1e-3          # the state has moved
    return solver, res


def test_assembled_matrices_equal_the_references_real_form():
    import dedalus_amd.public as d3
    GOLD = gold()
    solver, f = sc.alpha2_dynamo(d3, "RK222", oracle_kw())
    Nr = solver.Nr
    assert solver.cx and solver.L_tl.rotated and not solver.M_tl.rotated
    assert list(GOLD["L/ells"]) == list(sc.MATRIX_ELLS)
    for ell in sc.MATRIX_ELLS:
        A = solver._dense(solver.L_tl, ell)
        assert A.dtype == np.complex128
        A = A[:3 * Nr, :3 * Nr]                              # first equation x B (both three full-radius components)
        got = sc.real_form(A).reshape(3, Nr, 2, 3, Nr, 2).transpose(0, 2, 1, 3, 5, 4).reshape(6 * Nr, 6 * Nr)
        ref = GOLD["L/%d" % ell]
        assert np.abs(A.imag).max() >= 1e-3 * np.abs(A.real).max()
        assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max(), (ell, np.abs(got - ref).max())
    assert solver._dense(solver.M_tl, 1).dtype == np.float64
    assert not np.any(solver._dense(solver.L_tl, 0).imag)    # ell = 0: the curl's blocks vanish


def test_curl_lhs_lbvp_oracle():
    check_lbvp(oracle_kw())


@pytest.mark.parametrize("ts", ["RK222", "SBDF2"])
def test_alpha2_dynamo_end_state_oracle(ts):
    solver, res = check_dynamo(ts, oracle_kw())
    band = solver._band
    assert band and band["plan"].cx and band["plan"].per


def _plan(s, **kw):
    from dedalus_amd.core.ellband import EllBandPlan
    prow = sorted({c for m in s.emap for (c, off, nr) in m if nr != s.Nr})
    pcol = sorted({c for m in s.vmap for (c, off, nr) in m if nr != s.Nr})
    return EllBandPlan(lambda g: s._dense(s.M_tl, g), lambda g: s._dense(s.L_tl, g),
                       [s.row_valid[:, g, :] for g in range(s.nl)], [s.col_valid[:, g, :] for g in range(s.nl)],
                       prow, pcol, s.Nr, list(range(s.nl)), **kw)


def test_complex_band_plan_and_its_reference_solve():
    import dedalus_amd.public as d3
    s, f = sc.alpha2_dynamo(d3, "SBDF2", oracle_kw())
    plan = _plan(s)
    print("band plan: banded ell %s, dense %s, kl %d ku %d" % (sorted(plan.per), plan.why_dense, plan.kl, plan.ku))
    assert plan.cx and plan.MB.dtype == np.complex128 and plan.T.dtype == np.float64 and plan.P.dtype == np.float64
    banded = [g for g in sorted(plan.per) if np.any(plan.LB[g].imag != 0)]
    assert banded, "no banded group with an imaginary band"
    assert plan.kl + plan.ku <= plan.cw_max
    rng = np.random.default_rng(0)
    for g in banded[:3]:
        A = s._dense(s.M_tl, g) + 0.01 * s._dense(s.L_tl, g)
        rv, cv = s.row_valid[:, g, :].reshape(-1), s.col_valid[:, g, :].reshape(-1)
        rhs = (rng.standard_normal(A.shape[0]) + 1j * rng.standard_normal(A.shape[0])) * rv
        x = plan.reference_solve(g, 1.0, 0.01, rhs[:, None])[:, 0]
        want = np.zeros(A.shape[0], dtype=complex)
        want[cv] = np.linalg.solve(A[np.ix_(rv, cv)], rhs[rv])
        assert np.abs(x - want).max() <= 1e-9 * np.abs(want).max(), g


def test_curl_free_problem_keeps_its_real_plan_byte_for_byte():
    """The plan of a curl-free problem is float64 and takes the real handle.  The same matrices handed over as complex128
    with a vanishing imaginary part -- the complex code path with nothing in it -- give the same plan byte for byte: nothing
    of the complex handling reaches a real group.
    What this shows: complex input without an imaginary part collapses to the float64 plan.  What it does not show: that the
    plan equals the one the commit before the complex path computed -- no plan of that commit is recorded here (the last
    bits of the LAPACK calls in the analysis may differ between hosts), and the plan-wide window filter of EllBandPlan runs
    for real plans as well (at kl + ku <= 96), in both plans compared here."""
    import dedalus_amd.public as d3
    s, f = se.potential_induction(d3, "SBDF2", oracle_kw())
    assert not s.cx and s._dense(s.L_tl, 2).dtype == np.float64 and s._dense(s.M_tl, 2).dtype == np.float64
    a = _plan(s)
    dense = s._dense
    s._dense = lambda tl, ell: dense(tl, ell).astype(np.complex128)
    b = _plan(s)
    s._dense = dense
    assert not a.cx and not b.cx and a.per and sorted(a.per) == sorted(b.per) and a.dense_groups == b.dense_groups
    assert (a.kl, a.ku, a.mp, a.nbc) == (b.kl, b.ku, b.mp, b.nbc)
    for name in ("MB", "LB", "T", "P", "row_index", "col_index"):
        x, y = getattr(a, name), getattr(b, name)
        assert x.dtype == y.dtype and x.dtype.kind != "c" and x.tobytes() == y.tobytes(), name


def test_plan_wide_band_must_fit_the_complex_windows():
    """the handle is created with max kl and max ku over the groups: two groups that fit one by one (30 + 30, 10 + 50) but
    not together (30 + 50 > 64) must not both stay banded"""
    from dedalus_amd.core.ellband import EllBandPlan
    n = 90
    rng = np.random.default_rng(3)

    def band(kl, ku):
        i, j = np.indices((n, n))
        A = np.where((i - j <= kl) & (j - i <= ku), rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)), 0)
        A[np.arange(n), np.arange(n)] += 8
        A[np.arange(kl, n), np.arange(n - kl)] = 1 + 1j               # the outermost diagonals are there
        A[np.arange(n - ku), np.arange(ku, n)] = 1 - 1j
        return A
    L = [band(30, 30), band(10, 50)]
    valid = [np.ones((1, n), dtype=bool)] * 2
    plan = EllBandPlan(lambda g: np.zeros((n, n)), lambda g: L[g], valid, valid, [], [], n, [0, 1])
    assert plan.cx and len(plan.per) == 1 and len(plan.dense_groups) == 1
    assert plan.kl + plan.ku <= plan.cw_max
    assert "too wide" in plan.why_dense[plan.dense_groups[0]]


def test_refusals():
    import dedalus_amd.public as d3
    # a curl in a boundary row: complex boundary rows go to the dense path (T and P are real)
    s, f = sc.alpha2_dynamo(d3, "SBDF2", oracle_kw(), wall_curl=True)
    plan = _plan(s)
    hit = [g for g, why in plan.why_dense.items() if why == "complex boundary rows"]
    assert hit and all(g >= 1 for g in hit) and not any(g in plan.per for g in hit)
    assert set(hit) == {g for g in range(1, s.nl) if s.row_valid[:, g, :].any()}
    # an executor without complex per-ell systems: today's message, at add_equation
    import shell_tensor_cases as st
    import shell_vector_cases as sv
    from oracle.np_executor import NumpyExecutor
    plain = dict(executor=sv.with_rot(type(st.with_mix(NumpyExecutor))))
    with pytest.raises(NotImplementedError, match="curl in a shell LHS: per-ell systems are real"):
        sc.alpha2_dynamo(d3, "SBDF2", plain)
    # still refused by their present messages
    s2, f2 = sc.alpha2_dynamo(d3, "SBDF2", oracle_kw())
    er = f2["B"].dist.VectorField(f2["B"].dist.coordsys, name="er", bases=f2["B"].basis.radial_basis)
    problem = d3.IVP([f2["B"]], namespace=dict(B=f2["B"], er=er, cross=d3.cross, dt=d3.dt))
    with pytest.raises(NotImplementedError, match="cross product with a radial field in a shell LHS"):
        problem.add_equation("dt(B) + cross(er, B) = 0")
    coords, dist, shell, fields = se.build(d3, (8, 4, 6), oracle_kw())
    with pytest.raises(NotImplementedError, match="SphericalEllProduct: ell_func.* is complex"):
        d3.SphericalEllProduct(fields["v"], coords, lambda l: 1j * l)
