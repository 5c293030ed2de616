"""Host side of the reduced analysis tasks (core/reduced.py; no GPU): the RealFourier reduction vectors against the
reference's results, the hoisting of Fourier reductions to the top of linear subtrees, and what stays refused."""
import os

import numpy as np
import pytest

import dedalus_amd.public as d3
from dedalus_amd.core import operators as ops
from oracle.np_executor import NumpyExecutor

import reduced_cases as rc

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reduced_tasks.npz")


def _case(case):
    return rc.build(d3, case, dist_kw=dict(executor=NumpyExecutor()))


def test_realfourier_vectors_reproduce_the_reference_1d():
    """interpolate_vector / integrate_vector dotted with the stored coefficients = the reference's 'c' results"""
    gold = np.load(GOLD)
    dist, cd, bases, f = _case("f1")
    xb = bases["x"]
    c = gold["f1/in/b"].astype(np.float64)
    p = rc.positions("f1")
    scale = np.abs(c).sum()
    for name, vec in (("b_x_on", xb.interpolate_vector(p["x_on"])), ("b_x_off", xb.interpolate_vector(p["x_off"])),
                      ("b_x_left", xb.interpolate_vector("left")), ("integ_x", xb.integrate_vector()),
                      ("integ_all", xb.integrate_vector()), ("ave_x", xb.integrate_vector() / xb.length)):
        ref = gold["f1/%s/c" % name]
        assert ref.shape == (1,)
        assert abs(vec @ c - ref[0]) <= 64 * 2.0 ** -52 * scale, name
    # the reference's layout: interleaved cos / -sin at the native coordinate, bounds offset included
    v = xb.interpolate_vector(p["x_off"])
    xn = 2 * np.pi * (p["x_off"] - xb.bounds[0]) / xb.length
    m = np.arange(32)
    assert np.array_equal(v[0::2], np.cos(m * xn)) and np.array_equal(v[1::2], -np.sin(m * xn))
    assert v[1] == 0.0                                      # the (invalid) -sin slot of k = 0
    assert np.array_equal(xb.interpolate_vector("right"), xb.interpolate_vector(xb.bounds[1]))
    assert np.array_equal(xb.interpolate_vector("center"), xb.interpolate_vector(6.0))
    iv = xb.integrate_vector()
    assert iv[0] == xb.length and not iv[1:].any()


def test_hoisting_brings_fourier_reductions_to_the_top():
    from dedalus_amd.core import reduced
    dist, cd, bases, f = _case("rb3d")
    b, u, ez = f["b"], f["u"], f["ez"]
    x, y, z = cd["x"], cd["y"], cd["z"]
    ax, ay = dist.coord_axis(x), dist.coord_axis(y)

    # a plain slice / profile: the operand itself is the inner expression
    assert reduced.hoist(b(x=0.5)) == ((("interp", ax, 0.5),), b)
    assert reduced.hoist(d3.Average(b, (x, y))) == ((("ave", ax), ("ave", ay)), b)
    assert reduced.hoist(b(x="left"))[0] == (("interp", ax, 0.0),)

    # reductions below operators that act on other axes / on components move above them
    reds, inner = reduced.hoist(d3.Differentiate(b(x=0.5), z))
    assert reds == (("interp", ax, 0.5),) and isinstance(inner, ops.Differentiate) and inner.operand is b
    reds, inner = reduced.hoist(d3.Average(b, x)(z=0.37))
    assert reds == (("ave", ax),) and isinstance(inner, ops.Interpolate) and inner.operand is b and inner.coord is z
    reds, inner = reduced.hoist(3.0 * (u(x=0.5)(y=0.25) @ ez))
    assert reds == (("interp", ax, 0.5), ("interp", ay, 0.25))
    assert isinstance(inner, ops.Multiply) and inner.number == 3.0 and isinstance(inner.args[1], ops.DotProduct)
    assert inner.args[1].args[0] is u

    # integrals split: the Jacobi part stays inside, the Fourier parts come out
    reds, inner = reduced.hoist(d3.Integrate(b))
    assert reds == (("integ", ax), ("integ", ay)) and isinstance(inner, ops.Integrate) and inner.operand is b
    assert inner.axes == [dist.coord_axis(z)]

    # d/dx above a reduction along x: zero, as in the reference
    reds, inner = reduced.hoist(d3.Differentiate(b(x=0.5), x))
    assert reds == (("interp", ax, 0.5),) and isinstance(inner, ops.Multiply) and inner.number == 0.0

    # sums: equal reductions merge, different ones stay where they are (evaluated as leaves)
    reds, inner = reduced.hoist(d3.Average(b, x) + d3.Average(b, x))
    assert reds == (("ave", ax),) and isinstance(inner, ops.Add) and inner.args == (b, b)
    e = b(x=0.5) + b(x=0.75)
    assert reduced.hoist(e) == ((), e)

    # nonlinear nodes are not crossed; a reduction OF one is hoisted as usual
    prod = b * (u @ ez)
    reds, inner = reduced.hoist(d3.Average(prod, (x, y)))
    assert reds == (("ave", ax), ("ave", ay)) and inner is prod
    e = d3.Average(b, x) * d3.Average(u @ ez, x)
    assert reduced.hoist(e) == ((), e)

    # nothing to hoist: the expression itself
    e = d3.Differentiate(b, z)
    assert reduced.hoist(e) == ((), e)
    e = b(z=0.37)
    assert reduced.hoist(e) == ((), e)
    assert reduced.has_fourier_reduction(prod) is False and reduced.has_fourier_reduction(d3.Average(prod, x))


def test_reduced_domains_have_size_one_axes():
    dist, cd, bases, f = _case("rb3d")
    b, u = f["b"], f["u"]
    assert b(x=0.5).domain.coeff_shape() == (1, 32, 16)
    assert d3.Average(b, ("x", "y")).domain.coeff_shape() == (1, 1, 16)       # names resolve like coordinates
    assert d3.Average(b, ("x", "y")).axes == d3.Average(b, (cd["x"], cd["y"])).axes == d3.ave(b, ("x", "y")).axes
    assert d3.Integrate(b).domain.coeff_shape() == (1, 1, 1)
    assert u(y=0.1).domain.grid_shape((1.5, 1.5, 1.5)) == (48, 1, 24)


def test_lhs_use_of_a_fourier_interpolation_still_raises():
    from dedalus_amd.core.problems import LinCtx
    dist, cd, bases, f = _case("rb3d")
    b = f["b"]
    with pytest.raises(NotImplementedError, match="Fourier axis"):
        b(x=0.5).lin(LinCtx((b,), strict=True))
    with pytest.raises(NotImplementedError, match="Fourier axis"):
        b(x=0.5).lin(None)
    tau = dist.Field(name="tau", bases=(bases["y"], bases["z"]))
    problem = d3.LBVP([b, tau], namespace=dict(b=b, tau=tau, lap=d3.lap))
    problem.add_equation("lap(b) + tau = 0")
    with pytest.raises(NotImplementedError, match="Fourier axis"):
        problem.add_equation("b(x=0.5) = 0")


def test_several_ranks_refuse_fourier_reductions_by_name(monkeypatch):
    import types

    from dedalus_amd.core.output import DictionaryHandler
    monkeypatch.setenv("DDH_EMULATE_RANK", "1/4")
    dist, cd, bases, f = rc.build(d3, "rb3d", dist_kw=dict(executor=NumpyExecutor(), mesh=(4,)))
    assert dist.size == 4
    b = f["b"]
    h = DictionaryHandler(types.SimpleNamespace(dist=dist, problem=None), iter=1)
    with pytest.raises(NotImplementedError, match="'midplane'.*several ranks"):
        h.add_task(b(x=0.5), name="midplane")
    with pytest.raises(NotImplementedError, match="several ranks"):
        d3.Average(b * b, "x").evaluate()
    assert h.tasks == []
    h.add_task(b, name="b")                                 # whole fields are written as before
    assert [t["name"] for t in h.tasks] == ["b"]
