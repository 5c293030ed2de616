"""Stress-free walls of the shell on the NumPy oracle executor (no GPU): radial(u(r=R)) = 0 and
angular(radial(strain(r=R), 0), 0) = 0 as boundary rows of an LBVP and of the convection IVP, against the reference's
solution and end states (tests/golden/shell_stressfree_ivp.npz, written by tools/make_golden_shell_stressfree_ivp.py).

Bounds: 1e-10, the project's end-state tolerance, on every variable.  For the LBVP's variables and the fields p, b, u of
the end state it is the relative L2 error of the variable.  A tau variable of the IVP is no field of its own: it exists as
the term factor * lift(tau) of one equation, and what its rounding costs is that term's error against the equation it
corrects.  So a tau's error is measured as factor * |tau - ref| over the norm of the largest term of its equation
(tests/shell_tensor_cases.py::tau_term_scales lists equations, factors and terms), and the same 1e-10 is asked of it.
In its own norm a tau carries the rounding of fields up to 1e4 times larger: measured, relative to |tau|, tau_b1 2.8e-10,
tau_b2 4.9e-11, tau_u1 1.3e-12, tau_u2 6.9e-12 (RK222, oracle executor; 2.3e-10, 5.9e-11, 1.3e-12, 2.3e-12 on the
device), i.e. tau_b1 alone is above 1e-10 there, with an absolute error of 7e-14 beside |b| = 1.5.  The figures in both
norms are printed by the test and kept in profiles/shell_tensor_ops.txt."""
import os

import numpy as np
import pytest

import shell_tensor_cases as st
from test_shell_tensor_ops import oracle_kw, rel_l2

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shell_stressfree_ivp.npz"))
TOL = 1e-10


def check_lbvp(dist_kw):
    import dedalus_amd.public as d3
    solver, f = st.stressfree_lbvp(d3, dist_kw)
    f["f"]["c"] = GOLD["lbvp/in_f"].astype(np.float64)
    solver.solve()
    for k in ("u", "tau_u1", "tau_u2"):
        got, ref = np.array(f[k]["c"]), GOLD["lbvp/" + k]
        assert got.shape == ref.shape
        err = rel_l2(got, ref)
        print("stress-free LBVP %s: %.3e" % (k, err))
        assert err <= TOL, (k, err)
    # the walls hold in the solution: no flow through the inner wall, no tangential stress on it, no slip outside
    u = f["u"]
    strain = d3.grad(u) + d3.trans(d3.grad(u))
    size = np.abs(np.array(d3.radial(strain(r=st.RADII[0]), 0).evaluate()["c"])).max()
    assert np.abs(np.array(d3.radial(u(r=st.RADII[0])).evaluate()["c"])).max() <= 1e-12 * np.abs(GOLD["lbvp/u"]).max()
    assert np.abs(np.array(d3.angular(d3.radial(strain(r=st.RADII[0]), 0), 0).evaluate()["c"])).max() <= 1e-11 * size
    assert np.abs(np.array(u(r=st.RADII[1]).evaluate()["c"])).max() <= 1e-12 * np.abs(GOLD["lbvp/u"]).max()
    return solver


def check_convection(ts, dist_kw):
    import dedalus_amd.public as d3
    solver, res, scales = st.run_stressfree_convection(d3, ts, dist_kw)
    ref = {k: GOLD["%s/%s" % (ts, k)] for k in ("p", "b", "u", "tau_b1", "tau_b2", "tau_u1", "tau_u2")}
    own = {k: rel_l2(res[k], ref[k]) for k in ref}
    errs = {k: (scales[k][0] * float(np.linalg.norm((res[k] - ref[k]).ravel())) / scales[k][1] if k in scales else own[k])
            for k in ref}
    print("stress-free convection %s:" % ts, {k: "%.1e" % v for k, v in errs.items()},
          "taus in their own norm:", {k: "%.1e" % own[k] for k in scales})
    for k, e in errs.items():
        assert res[k].shape == ref[k].shape
        assert e <= TOL, (ts, k, e)
    assert abs(float(res["tau_p"].reshape(-1)[0])) < 1e-10
    assert np.abs(res["u"]).max() > 1e-7
    return solver


def test_stressfree_lbvp_oracle():
    check_lbvp(oracle_kw())


@pytest.mark.parametrize("ts", ["RK222", "SBDF2"])
def test_stressfree_convection_end_state_oracle(ts):
    check_convection(ts, oracle_kw())


def test_stressfree_rows_couple_the_velocity_components_and_stay_real():
    import dedalus_amd.public as d3
    from dedalus_amd.core.shell import EllTermList
    solver, f = st.stressfree_lbvp(d3, oracle_kw())
    eqs = solver.problem.equations
    assert [eq["ncomp"] for eq in eqs] == [3, 1, 2, 3] and eqs[2]["lhs"].sig == (2,)
    L = eqs[2]["L"][0]
    assert isinstance(L, EllTermList) and not L.rotated
    assert sorted({t[0] for t in L.terms}) == [0, 1] and sorted({t[1] for t in L.terms}) == [0, 1, 2]
    # valid rows of the angular condition: spin -, + exist for ell >= 1, as the (-, +) components of the tau they close
    emap = solver.emap[2]
    for (sc, off, nr) in emap:
        assert not solver.row_valid[sc, 0, off] and solver.row_valid[sc, 1:, off].all()


def test_band_plan_covers_the_stressfree_systems():
    """The stress-free rows couple the three velocity components at each wall.  core/ellband.py must either band every
    ell within the device limits (border <= 8, recombination band <= 16) or hand it to the dense path with a reason; a
    group is never left without a solver."""
    import dedalus_amd.public as d3
    from dedalus_amd.core.ellband import EllBandPlan
    s, f = st.stressfree_convection(d3, "SBDF2", oracle_kw())
    prow = sorted({sc for m in s.emap for (sc, off, nr) in m if nr != s.Nr})
    pcol = sorted({sc for m in s.vmap for (sc, off, nr) in m if nr != s.Nr})
    ells = list(range(s.nl))
    plan = EllBandPlan(lambda g: s._dense(s.M_tl, g), lambda g: s._dense(s.L_tl, g),
                       [s.row_valid[:, g, :] for g in range(s.nl)], [s.col_valid[:, g, :] for g in range(s.nl)],
                       prow, pcol, s.Nr, ells)
    print("band plan: banded ell %s, dense %s, nbc %d, mp %d" % (sorted(plan.per), plan.why_dense, plan.nbc, plan.mp))
    assert sorted(list(plan.per) + list(plan.dense_groups)) == ells
    assert set(plan.why_dense) == set(plan.dense_groups)
    assert plan.nbc <= 8 and plan.mp <= 16, "beyond these the solver keeps dense inverses for every ell"


def test_angular_in_the_volume_is_refused_by_name():
    import dedalus_amd.public as d3
    coords, dist, shell, u = st.build(d3, (8, 4, 6), oracle_kw())
    strain = d3.grad(u) + d3.trans(d3.grad(u))
    for arg in (u, d3.radial(strain, 0)):
        with pytest.raises(NotImplementedError, match="angular of the shell"):
            d3.angular(arg)
    a = d3.angular(u(r=0.7))
    assert a.sig == (2,) and a.ncomp == 2 and a.rank == 1
    with pytest.raises(NotImplementedError, match="lift of an operand with an S2 index"):
        d3.Lift(a, shell, -1)
    with pytest.raises(NotImplementedError, match="grid data of a field with an S2 index"):
        a.evaluate()["g"]
    with pytest.raises(ValueError, match="S2 index already"):
        d3.radial(a, 0)
