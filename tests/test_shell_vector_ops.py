"""Cross product and curl of shell vector fields on the NumPy oracle executor (no GPU): term-list algebra with the
rotation flag, vector identities, the reference's results (tests/golden/shell_vector_ops.npz, written by
tools/make_golden_shell_vector_ops.py) and the refusals.

Bound of the fixture comparisons: max |x - ref| <= TOL max |ref| per task, the form and figure tests/test_shell_fields.py
applies to grad and div of shell fields capped by ten times the oracle path's measured error
(profiles/shell_vector_ops.txt); div(curl(u)) and curl(grad(f)) vanish identically, there the scale is that of the
first-order intermediate times the magnitude of one more derivative, see each test."""
import os

import numpy as np
import pytest

import shell_vector_cases as sv
from test_shell_fields import CONV_TOL, _rel as rel

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shell_vector_ops.npz"))
# ten times the worst error of the oracle path measured against the fixtures, rounded down (curl tasks 5.98e-16, cross
# tasks 5.38e-15; profiles/shell_vector_ops.txt), far inside the 1e-10 of tests/test_shell_fields.py::check_operators
TOL = {"curl": 5.9e-15, "cross": 5.3e-14}


def oracle_kw():
    from oracle.np_executor import NumpyExecutor
    return dict(executor=sv.with_rot(NumpyExecutor))


def run_tasks(kind, shape, dist_kw, d3=None):
    """-> {task: (result coefficients, reference)}"""
    if d3 is None:
        import dedalus_amd.public as d3
    coords, dist, shell, u, v = sv.build(d3, shape, dist_kw)
    key = "%s/%s/" % (kind, sv.tag(shape))
    u["c"] = GOLD[key + "in_u"].astype(np.float64)
    if kind == "cross":
        v["c"] = GOLD[key + "in_v"].astype(np.float64)
    tasks = sv.curl_tasks(d3, u) if kind == "curl" else sv.cross_tasks(d3, coords, dist, shell, u, v)
    return {name: (np.array(expr.evaluate()["c"]), GOLD[key + name]) for name, expr in tasks.items()}


def check_tasks(kind, shape, dist_kw, record=None):
    scale = None
    for name, (got, ref) in run_tasks(kind, shape, dist_kw).items():
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        if name == "divcurl":
            # identically zero: what is left is the rounding of curl(u) (relative TOL of its size) carried through one more
            # derivative, whose matrices are as large as those that took u to curl(u)
            scale = np.abs(GOLD["curl/%s/curl" % sv.tag(shape)]).max() ** 2 / np.abs(GOLD["curl/%s/in_u" % sv.tag(shape)]).max()
        else:
            scale = np.abs(ref).max()
        err = np.abs(got - ref).max() / scale
        print("%s %s %s: %.3e" % (kind, sv.tag(shape), name, err))
        if record is not None:
            record.append((kind, sv.tag(shape), name, err))
        assert err <= TOL[kind], (kind, shape, name, err)


def test_termlist_algebra_with_rotation():
    from dedalus_amd.core.shell import EllTermList
    rng = np.random.default_rng(0)
    A, B, C = (rng.standard_normal((3, 4, 4)) for _ in range(3))
    rot = EllTermList(2, 2, [(0, 1, A), (1, 0, B)], [1, 1])
    real = EllTermList(2, 2, [(0, 0, C), (1, 1, C)])
    rr = real.compose(rot)
    assert rr.rot == [1, 1] and [t[:2] for t in rr.terms] == [(0, 1), (1, 0)]
    assert np.array_equal(rr.terms[0][2], np.matmul(C, A))
    assert rot.compose(real).rot == [1, 1]
    sq = rot.compose(rot)                                     # i . i = -1: real terms with the sign flipped
    assert sq.rot == [0, 0] and [t[:2] for t in sq.terms] == [(0, 0), (1, 1)]
    assert np.array_equal(sq.terms[0][2], -np.matmul(A, B)) and np.array_equal(sq.terms[1][2], -np.matmul(B, A))
    both = rot + real + rot                                   # real and rotated terms of one block stay apart
    assert sorted(zip([t[:2] for t in both.terms], both.rot)) == [((0, 0), 0), ((0, 1), 1), ((1, 0), 1), ((1, 1), 0)]
    assert np.array_equal(both.terms[both.rot.index(1)][2], 2 * A)
    assert rot.scaled(-2.0).rot == [1, 1] and rot.embed(1, 0, 4, 4).rot == [1, 1]
    assert not real.rotated and rot.rotated and not sq.rotated


def test_curl_termlist_is_the_reference_table():
    """blocks (-, +) <-> 0 only, all rotated; ell = 0 carries none (no regularity component pair is allowed there)"""
    import dedalus_amd.public as d3
    from dedalus_amd.core.shell import shell_op_termlist
    coords, dist, shell, u, v = sv.build(d3, (8, 4, 6), oracle_kw())
    tl = shell_op_termlist("curl", shell, 1, 0)
    assert sorted(t[:2] for t in tl.terms) == [(0, 2), (1, 2), (2, 0), (2, 1)] and tl.rot == [1, 1, 1, 1]
    assert all(not np.any(t[2][0]) for t in tl.terms)
    assert d3.curl(u).basis.k == 1 and d3.curl(d3.curl(u)).basis.k == 2 and d3.curl(u).rank == 1


@pytest.mark.parametrize("shape", sv.CURL_SHAPES, ids=sv.tag)
def test_curl_matches_reference_oracle(shape):
    check_tasks("curl", shape, oracle_kw())


@pytest.mark.parametrize("shape", sv.CROSS_SHAPES, ids=sv.tag)
def test_cross_matches_reference_oracle(shape):
    check_tasks("cross", shape, oracle_kw())


@pytest.mark.parametrize("shape", [(8, 4, 6), (20, 10, 9)], ids=sv.tag)
def test_curl_of_gradient_vanishes(shape):
    import dedalus_amd.public as d3
    coords, dist, shell, u, v = sv.build(d3, shape, oracle_kw())
    f = d3.div(u)                                             # a full-spectrum scalar
    u["c"] = GOLD["curl/%s/in_u" % sv.tag(shape)].astype(np.float64)
    g = np.array(d3.grad(f).evaluate()["c"])
    cg = np.array(d3.curl(d3.grad(f)).evaluate()["c"])
    big = np.abs(np.array(d3.curl(d3.curl(u)).evaluate()["c"])).max()       # two derivatives of the same field
    assert np.abs(g).max() > 1 and np.abs(cg).max() <= 1e-12 * big, (np.abs(cg).max(), big)


def test_refusals_by_name():
    import dedalus_amd.public as d3
    coords, dist, shell, u, v = sv.build(d3, (8, 4, 6), oracle_kw())
    s = dist.Field(name="s", bases=shell)
    tau = dist.VectorField(coords, name="tau", bases=shell.outer_surface)
    rad = sv.radial_vector(d3, coords, dist, shell)
    for arg, what in ((s, "curl of a scalar"), (d3.grad(u), "curl of a rank-2 tensor"), (tau, "curl of a surface operand"),
                      (rad, "curl of a radial operand")):
        with pytest.raises(NotImplementedError, match=what):
            d3.curl(arg)
    with pytest.raises(NotImplementedError, match="cross product of operands that are not both vectors"):
        d3.cross(u, s)
    problem = d3.IVP([u], namespace=dict(u=u, rad=rad, curl=d3.curl, cross=d3.cross))
    with pytest.raises(NotImplementedError, match="curl in a shell LHS: per-ell systems are real"):
        problem.add_equation("dt(u) + curl(u) = 0")
    with pytest.raises(NotImplementedError, match="cross product with a radial field in a shell LHS"):
        problem.add_equation("dt(u) + cross(rad, u) = 0")
    with pytest.raises(ValueError, match="LHS must be linear"):
        problem.add_equation("dt(u) + cross(u, u) = 0")
    assert not problem.equations


def test_curl_of_curl_is_a_real_left_hand_side():
    """i . i = -1: curl(curl(u)) composes to real per-ell blocks, which a left-hand side accepts: - (curl at k + 1)(curl at k)"""
    import dedalus_amd.public as d3
    from dedalus_amd.core.shell import shell_op_termlist
    coords, dist, shell, u, v = sv.build(d3, (8, 4, 6), oracle_kw())
    problem = d3.IVP([u], namespace=dict(u=u, curl=d3.curl))
    eq = problem.add_equation("dt(u) + curl(curl(u)) = 0")
    L = eq["L"][0]
    assert not L.rotated and sorted(t[:2] for t in L.terms) == [(0, 0), (0, 1), (1, 0), (1, 1), (2, 2)]
    c0, c1 = (shell_op_termlist("curl", shell, 1, k) for k in (0, 1))
    blk = {(co, ci): m for (co, ci, m) in c0.terms}
    blk1 = {(co, ci): m for (co, ci, m) in c1.terms}
    for (co, ci, m) in L.terms:
        want = -sum(np.matmul(blk1[(co, mid)], blk[(mid, ci)]) for mid in range(3) if (co, mid) in blk1 and (mid, ci) in blk)
        assert np.abs(want).max() > 0 and np.array_equal(m, want), (co, ci)


def check_curl_leaves_other_operators_alone(dist_kw):
    """The curl marks the (m, l) = (0, 0) msin slot as a hole in ITS slot map; a rank-2 tensor keeps that slot (the
    reference drops it for scalars and vectors only): operators built after a curl was evaluated give the bits they gave
    before, and the cached slot map of the basis is untouched."""
    import dedalus_amd.public as d3
    from dedalus_amd.core.shell import operate_slot_sequences
    coords, dist, shell, u, v = sv.build(d3, (8, 4, 6), dist_kw)
    u["c"] = GOLD["cross/8x4x6/in_u"].astype(np.float64)
    v["c"] = GOLD["cross/8x4x6/in_v"].astype(np.float64)
    cached = operate_slot_sequences(shell.sphere)[1].copy()
    exprs = lambda: dict(sum=d3.grad(u) + u * v, lap=d3.lap(u * v), grad=d3.grad(d3.curl(u)))
    before = {k: np.array(e.evaluate()["c"]) for k, e in list(exprs().items())[:2]}
    w = np.array(d3.curl(u).evaluate()["c"])
    assert np.abs(w).max() > 0
    assert np.array_equal(operate_slot_sequences(shell.sphere)[1], cached)
    after = {k: np.array(e.evaluate()["c"]) for k, e in exprs().items()}       # new nodes: their term lists are built now
    for k in before:
        assert np.array_equal(before[k].view(np.uint64), after[k].view(np.uint64)), k
    m0 = before["sum"][:, :, 1, 0, :]                                          # packed row 1, column 0: (m, l) = (0, 0), msin
    assert np.abs(m0).max() > 1e-3, "the case must populate the slot the curl leaves out"
    assert np.isfinite(after["grad"]).all()


def test_curl_leaves_other_operators_alone_oracle():
    check_curl_leaves_other_operators_alone(oracle_kw())


def test_meridional_basis_field_is_a_shell_field():
    import dedalus_amd.public as d3
    coords, dist, shell, u, v = sv.build(d3, (8, 4, 6), oracle_kw())
    ez = sv.rotation_axis(d3, coords, dist, shell)
    assert ez.basis is shell and ez["g"].shape == (3, 8, 4, 6)
    assert shell.meridional_basis is shell.meridional_basis


def test_rotating_convection_end_state_oracle():
    """(c) on the oracle executor, through the compat import path rotating-shell scripts use"""
    from dedalus_amd import compat
    compat.install()
    import dedalus.public as d3
    G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shell_vector_ivp.npz"))
    solver, res = sv.run_rotating_convection(d3, oracle_kw())
    tol = dict(CONV_TOL, curl_u=CONV_TOL["u"], enstrophy_sqrt=CONV_TOL["u"])
    errs = {k: rel(res[k], G["end/" + k]) for k in tol}
    print("rotating convection (oracle):", {k: "%.1e" % v for k, v in errs.items()})
    for k, t in tol.items():
        assert res[k].shape == G["end/" + k].shape and errs[k] < t, (k, errs[k])
    assert abs(float(res["tau_p"].reshape(-1)[0])) < 1e-10
