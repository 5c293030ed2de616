"""SphericalEllProduct on the shell and insulating (potential-field) walls on the NumPy oracle executor (no GPU): the public
name, the diagonal mix list and its composition with radial-matrix lists, the reference's results
(tests/golden/shell_ellproduct_ops.npz, shell_ellproduct_ivp.npz, written by tools/make_golden_shell_ellproduct.py) and the
refusals.

Bounds: operator results to a relative L2 error of 1e-12 of the task's norm (the transform tolerance of the README); the
LBVP solution and the IVP end states to the project's 1e-10: fields in their own norm, a tau variable as the error of its
term factor * lift(tau) against the largest term of the equation it corrects (shell_ellproduct_cases.tau_term_scales, the
measure of shell_tensor_cases.tau_term_scales for this problem's equations).  The boundary rows are compared entry by
entry to 1e-12 of the largest entry of the reference's rows of that ell."""
import os

import numpy as np
import pytest

import shell_ellproduct_cases as se
import shell_tensor_cases as st
import shell_vector_cases as sv
from test_shell_tensor_ops import rel_l2

HERE = os.path.dirname(os.path.abspath(__file__))
TOL_OP, TOL = 1e-12, 1e-10


def oracle_kw():
    """the NumPy oracle executor with the component mix (the ell product) and rotated terms (the curl of the induction term)"""
    from oracle.np_executor import NumpyExecutor
    return dict(executor=sv.with_rot(type(st.with_mix(NumpyExecutor))))


def gold(name):
    return np.load(os.path.join(HERE, "golden", name))


def check_ops(shape, dist_kw, record=None):
    import dedalus_amd.public as d3
    assert callable(d3.SphericalEllProduct)
    GOLD = gold("shell_ellproduct_ops.npz")
    coords, dist, shell, fields = se.build(d3, shape, dist_kw)
    key = se.tag(shape) + "/"
    for k, X in fields.items():
        X["c"] = GOLD[key + "in_" + k].astype(np.float64)
    for name, expr in se.op_tasks(d3, coords, fields, shape in se.PLAIN_ONLY).items():
        got, ref = np.array(expr.evaluate()["c"]), GOLD[key + name]
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        err = rel_l2(got, ref)
        print("%s %s: %.3e" % (se.tag(shape), name, err))
        if record is not None:
            record.append((se.tag(shape), name, err))
        assert err <= TOL_OP, (shape, name, err)


def variable_errors(d3, f, res, ref, eta):
    scales = se.tau_term_scales(d3, f, eta)
    own = {k: rel_l2(res[k], ref[k]) for k in ref if k != "tau_phi"}
    errs = {k: (scales[k][0] * float(np.linalg.norm((res[k] - ref[k]).ravel())) / scales[k][1] if k in scales else own[k])
            for k in own}
    return errs, own


def check_lbvp(dist_kw, record=None):
    import dedalus_amd.public as d3
    GOLD = gold("shell_ellproduct_ivp.npz")
    solver, f = se.potential_lbvp(d3, dist_kw)
    f["J"]["c"] = GOLD["lbvp/in_J"].astype(np.float64)
    solver.solve()
    res = se.end_state(f)
    ref = {k: GOLD["lbvp/" + k] for k in se.VARIABLES}
    errs, own = variable_errors(d3, f, res, ref, 1.0)
    print("potential-wall LBVP:", {k: "%.1e" % v for k, v in errs.items()}, "taus in their own norm:",
          {k: "%.1e" % own[k] for k in ("tau_A1", "tau_A2")})
    if record is not None:
        record.append(("lbvp", errs, own))
    for k, e in errs.items():
        assert res[k].shape == ref[k].shape
        assert e <= TOL, (k, e)
    assert abs(float(res["tau_phi"].reshape(-1)[0])) < 1e-10
    # the walls hold in the solution
    A, coords = f["A"], f["A"].dist.coordsys
    Ri, Ro = se.RADII
    size = np.abs(np.array(d3.radial(d3.grad(A)(r=Ro)).evaluate()["c"])).max()
    for R, func in ((Ro, se.ellp1), (Ri, se.ellm)):
        wall = d3.radial(d3.grad(A)(r=R)) + d3.SphericalEllProduct(A, coords, func)(r=R) / R
        assert np.abs(np.array(wall.evaluate()["c"])).max() <= 1e-11 * size
    return solver


def check_induction(ts, dist_kw, record=None):
    import dedalus_amd.public as d3
    GOLD = gold("shell_ellproduct_ivp.npz")
    solver, f, res = se.run_potential_induction(d3, ts, GOLD["ivp/in_A"], dist_kw)
    ref = {k: GOLD["%s/%s" % (ts, k)] for k in se.VARIABLES}
    errs, own = variable_errors(d3, f, res, ref, se.ETA)
    print("potential-wall induction %s:" % ts, {k: "%.1e" % v for k, v in errs.items()}, "taus in their own norm:",
          {k: "%.1e" % own[k] for k in ("tau_A1", "tau_A2")})
    if record is not None:
        record.append((ts, errs, own))
    for k, e in errs.items():
        assert res[k].shape == ref[k].shape
        assert e <= TOL, (ts, k, e)
    assert abs(float(res["tau_phi"].reshape(-1)[0])) < 1e-10
    assert rel_l2(res["A"], GOLD["ivp/in_A"].astype(np.float64)) > 1e-3          # the state has moved
    return solver


def test_public_name_and_structure():
    import dedalus_amd.public as d3
    from dedalus_amd.core.shell import EllMixList, reg_indices, regtotal, regularity_allowed
    assert callable(d3.SphericalEllProduct)
    coords, dist, shell, fields = se.build(d3, (16, 8, 8), oracle_kw())
    nl = shell.sphere.nl
    for k, X in fields.items():
        calls = []

        def func(l):
            calls.append(l)
            return l * (l + 1)
        e = d3.SphericalEllProduct(X, coords, func)
        assert e.rank == X.rank and e.basis is X.basis and e.sig == X.sig
        assert len(calls) == len(set(calls)) and min(calls) >= 0             # once per distinct argument, existing modes only
        ml = e.mixlist()
        assert isinstance(ml, EllMixList) and all(co == ci for (co, ci, q) in ml.terms)
        m = ml.matrices(nl)
        for c, t in enumerate(reg_indices(X.rank)):
            for l in range(nl):
                want = (l + regtotal(t)) * (l + regtotal(t) + 1) if regularity_allowed(l, t) else 0.0
                assert m[l, c, c] == want, (k, c, l)
    # a scalar multiple and a sum of products of one operand stay one diagonal mix
    u = fields["v"]
    e = 2 * d3.SphericalEllProduct(u, coords, se.ellp1) - d3.SphericalEllProduct(u, coords, se.ellm) / 4
    assert type(e).__name__ == "ShEllProduct" and e.arg is u and len(e.mixlist().terms) == 3
    a, b = d3.SphericalEllProduct(u, coords, se.ellp1).mixlist().matrices(nl), d3.SphericalEllProduct(u, coords, se.ellm).mixlist().matrices(nl)
    assert np.array_equal(e.mixlist().matrices(nl), 2 * a - b / 4)
    assert type(-e).__name__ == "ShEllProduct" and np.array_equal((-e).q, -e.q)
    # values of modes that do not exist never reach the table: the - component at ell = 0 would ask for ell_func(-1)
    picky = lambda l: 1.0 / (l + 1)                    # not defined at -1
    assert np.isfinite(d3.SphericalEllProduct(u, coords, picky).q).all()


@pytest.mark.parametrize("shape", se.OP_SHAPES, ids=se.tag)
def test_ell_product_matches_reference_oracle(shape):
    check_ops(shape, oracle_kw())


def test_slots_covered_by_several_ell_boxes_get_the_sum():
    """the evaluation follows SphericalEllOperator.operate: the (12, 8, 6) shape has such slots and the fixture pins them"""
    import dedalus_amd.public as d3
    from dedalus_amd.core.shell import operate_slot_sequences
    coords, dist, shell, fields = se.build(d3, (12, 8, 6), oracle_kw())
    seqs, slot = operate_slot_sequences(shell.sphere)
    assert len(seqs) > 0 and (slot >= shell.sphere.nl).any()
    terms, sm = d3.SphericalEllProduct(fields["s"], coords, se.ellp1)._slot_mix()
    (c0, c1, q), = terms
    assert len(q) == shell.sphere.nl + len(seqs)
    for j, seq in enumerate(seqs):
        assert q[shell.sphere.nl + j] == sum(l + 1 for l in seq)


def test_composition_in_both_orders_gives_real_radial_lists():
    import dedalus_amd.public as d3
    from dedalus_amd.core.shell import EllTermList
    coords, dist, shell, fields = se.build(d3, (16, 8, 8), oracle_kw())
    u, f = fields["v"], fields["s"]
    Ro = se.RADII[1]
    ep = lambda X: d3.SphericalEllProduct(X, coords, se.ELL_FUNCS["llp1"])
    lift = lambda X: d3.Lift(X, shell.derivative_basis(2), -1)
    tau = dist.VectorField(coords, name="tau", bases=shell.outer_surface)
    nodes = [(ep(u)(r=Ro), u), (d3.radial(d3.grad(ep(u))(r=Ro)), u), (d3.radial(ep(d3.grad(u))(r=Ro)), u),
             (d3.lap(ep(u)), u), (ep(d3.lap(u)), u), (d3.grad(ep(f)), f), (ep(d3.grad(f)), f),
             (ep(d3.radial(d3.grad(u))), u), (d3.radial(ep(d3.grad(u))), u), (ep(lift(tau)), tau),
             (ep(u) + d3.lap(u), u), (ep(d3.lap(u)) + d3.lap(ep(u)), u)]
    for node, var in nodes:
        d, isdt = node.lin([var])
        assert isinstance(d[0], EllTermList) and not d[0].rotated and not isdt
        assert all(np.isrealobj(m) and np.isfinite(m).all() for (co, ci, m) in d[0].terms)
    # the product commutes with operators that keep ell + regtotal of every component: lap, and the scalar's convert
    a, b = d3.lap(ep(u)).lin([u])[0][0], ep(d3.lap(u)).lin([u])[0][0]
    assert len(a.terms) == len(b.terms) == 3
    for (co, ci, m), (co2, ci2, m2) in zip(a.terms, b.terms):
        assert (co, ci) == (co2, ci2) and np.allclose(m, m2, rtol=1e-14, atol=0)
    # ... but not with grad, which moves a component from l to l -+ 1
    a, b = d3.grad(ep(f)).lin([f])[0][0], ep(d3.grad(f)).lin([f])[0][0]
    assert any(not np.allclose(m, m2) for (_, _, m), (_, _, m2) in zip(a.terms, b.terms))


def test_boundary_rows_are_real_and_equal_the_references_rows():
    import dedalus_amd.public as d3
    from dedalus_amd.core.shell import EllTermList, regularity_allowed, spin_allowed
    GOLD = gold("shell_ellproduct_ivp.npz")
    solver, f = se.potential_lbvp(d3, oracle_kw())
    Nr = solver.Nr
    differ = 0
    for name, eq in (("outer", solver.problem.equations[3]), ("inner", solver.problem.equations[4])):
        assert sorted(eq["L"]) == [0] and eq["ncomp"] == 3                  # acts on A alone
        tl = eq["L"][0]
        assert isinstance(tl, EllTermList) and not tl.rotated
        assert all(np.isrealobj(m) and not np.any(m[:, 1:, :]) for (co, ci, m) in tl.terms)      # boundary rows: the first row only
        rows = np.zeros((solver.nl, 3, 3 * Nr))
        for (co, ci, m) in tl.terms:
            rows[:, co, ci * Nr:(ci + 1) * Nr] += m[:, 0, :]
        ref = GOLD["rows/" + name]
        for ell in GOLD["rows/ells"]:
            # the solver masks rows and columns of modes that do not exist; the reference's matrices hold zeros there
            mask = np.array([[float(spin_allowed(ell, (co,)) and regularity_allowed(ell, (ci,))) for ci in range(3)] for co in range(3)])
            got = rows[ell] * np.repeat(mask, Nr, axis=1)
            assert np.abs(got - ref[ell]).max() <= 1e-12 * np.abs(ref[ell]).max(), (name, ell)
        differ += sum(not np.allclose(rows[2], rows[l]) for l in (3, 4, 5))
    assert differ == 6                                                  # the rows depend on ell


def test_band_plan_is_computed_per_ell_and_covers_the_potential_walls():
    """The boundary rows differ from ell to ell.  core/ellband.py must band every ell within the device limits with a
    recombination of that ell's own rows, or hand it to the dense path with a reason; no group is left without a solver."""
    import dedalus_amd.public as d3
    from dedalus_amd.core.ellband import EllBandPlan
    s, f = se.potential_induction(d3, "SBDF2", oracle_kw())
    prow = sorted({sc for m in s.emap for (sc, off, nr) in m if nr != s.Nr})
    pcol = sorted({sc for m in s.vmap for (sc, off, nr) in m if nr != s.Nr})
    ells = list(range(s.nl))
    plan = EllBandPlan(lambda g: s._dense(s.M_tl, g), lambda g: s._dense(s.L_tl, g),
                       [s.row_valid[:, g, :] for g in range(s.nl)], [s.col_valid[:, g, :] for g in range(s.nl)],
                       prow, pcol, s.Nr, ells)
    print("band plan: banded ell %s, dense %s, nbc %d, mp %d" % (sorted(plan.per), plan.why_dense, plan.nbc, plan.mp))
    assert sorted(list(plan.per) + list(plan.dense_groups)) == ells
    assert set(plan.why_dense) == set(plan.dense_groups)
    assert all(isinstance(w, str) and w for w in plan.why_dense.values())
    banded = sorted(g for g in plan.per if g >= 1)
    assert len(banded) >= 2, "the potential walls must not push every ell to the dense path at this size"
    for a, b in zip(banded[:-1], banded[1:]):
        assert not np.array_equal(plan.P[a], plan.P[b]), "recombination borrowed from another ell"
    # the plan solves each banded ell's own system: its host restatement against a dense solve of M + dt L
    rng = np.random.default_rng(0)
    for g in banded[:3]:
        A = s._dense(s.M_tl, g) + 0.01 * s._dense(s.L_tl, g)
        rv, cv = s.row_valid[:, g, :].reshape(-1), s.col_valid[:, g, :].reshape(-1)
        rhs = rng.standard_normal(A.shape[0]) * rv
        x = plan.reference_solve(g, 1.0, 0.01, rhs[:, None])[:, 0]
        want = np.zeros(A.shape[0])
        want[cv] = np.linalg.solve(A[np.ix_(rv, cv)], rhs[rv])
        assert np.abs(x - want).max() <= 1e-9 * np.abs(want).max(), g


def test_potential_wall_lbvp_oracle():
    check_lbvp(oracle_kw())


@pytest.mark.parametrize("ts", ["RK222", "SBDF2"])
def test_potential_wall_induction_end_state_oracle(ts):
    check_induction(ts, oracle_kw())


def test_refusals_by_name():
    import dedalus_amd.public as d3
    coords, dist, shell, fields = se.build(d3, (8, 4, 6), oracle_kw())
    u = fields["v"]
    tau_p = dist.Field(name="tau_p")
    er = dist.VectorField(coords, name="er", bases=shell.radial_basis)
    ep = lambda X, func=se.ellp1: d3.SphericalEllProduct(X, coords, func)
    for arg, what in ((er, "SphericalEllProduct of a radial operand"), (tau_p, "SphericalEllProduct of a constant operand"),
                      (d3.integ(fields["s"]), "SphericalEllProduct of a constant operand"),
                      (d3.ave(fields["s"]), "SphericalEllProduct of a reduced operand"),
                      (u(r=se.RADII[1]), "SphericalEllProduct of the surface operand"),
                      (d3.angular(u(r=se.RADII[1])), "SphericalEllProduct of an operand with an S2 index")):
        with pytest.raises(NotImplementedError, match=what):
            ep(arg)
    with pytest.raises(NotImplementedError, match="SphericalEllProduct: ell_func.* is complex"):
        ep(u, lambda l: 1j * l)
    with pytest.raises(NotImplementedError, match="SphericalEllProduct: ell_func.* is complex"):
        ep(u, lambda l: np.complex128(l))
    for bad in (lambda l: np.inf if l == 2 else 1.0, lambda l: np.nan):
        with pytest.raises(ValueError, match="SphericalEllProduct: ell_func.* is not finite"):
            ep(u, bad)
    with pytest.raises(ValueError, match="not the operand's coordinate system"):
        d3.SphericalEllProduct(u, d3.SphericalCoordinates("phi", "theta", "r"), se.ellp1)
    x = d3.CartesianCoordinates("x", "y")
    cart = d3.Distributor(x, dtype=np.float64).Field(name="f", bases=(d3.RealFourier(x["x"], 8, bounds=(0, 1)),
                                                                     d3.RealFourier(x["y"], 8, bounds=(0, 1))))
    with pytest.raises(NotImplementedError, match="SphericalEllProduct of"):
        d3.SphericalEllProduct(cart, x, se.ellp1)
    problem = d3.IVP([u], namespace=dict(u=u, coords=coords, ellp1=se.ellp1))
    with pytest.raises(NotImplementedError, match="SphericalEllProduct of the surface operand"):
        problem.add_equation("SphericalEllProduct(u(r=1.9), coords, ellp1) = 0")
    assert not problem.equations
