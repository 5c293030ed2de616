"""
Reduced analysis tasks on Cartesian domains: slices, profiles, integrals.

An expression whose domain lacks a Fourier basis -- `b(x=0.3)`, `ave(b, 'x')`, `integ(b)` -- cannot be evaluated pencil by
pencil: interpolation along a Fourier axis couples all its modes, and the result lives on a smaller array.  The reference
applies the (1 x N) matrices of InterpolateRealFourier / IntegrateRealFourier / AverageRealFourier along the axis
(core/basis.py:1227-1300).  Here such an expression is brought into the form

    R_1 ( R_2 ( ... inner ... ))          R_i: reductions along Fourier axes,  inner: everything else

by hoisting the reductions to the top of each linear subtree (`hoist`): a Fourier reduction commutes with every linear
operator that acts on other axes or on tensor components.  `inner` is evaluated on its full domain by the paths that
exist (fused conversion, stage cache, nonlinear grid stage, forward transform) and each R_i is one launch of
ddh_axis_contract on its coefficient data -- the whole axis for an interpolation, the k = 0 slab alone for an integral or
an average.  What cannot be hoisted (a sum of two different slices, a gradient of a slice) keeps its reductions as
leaves of the linear expression above them (Evaluator._eval_reduced_generic).
"""

import numpy as np

from . import operators as ops
from .basis import resolve_position
from .field import Field


def _axes(reds):
    return {r[1] for r in reds}


def _merged(reds, new):
    """reds + new as a canonical tuple: one reduction per axis (a second one along a removed axis acts on a constant),
    sorted by axis -- reductions along different axes commute."""
    out = {r[1]: r for r in reds}
    for r in new:
        out.setdefault(r[1], r)
    return tuple(out[ax] for ax in sorted(out))


def hoist(expr):
    """(reds, inner) with expr == reds applied to inner, reds = tuple of ('interp', axis, position) / ('integ', axis) /
    ('ave', axis) along Fourier axes, as far up as they commute.  reds == () returns expr itself."""
    if isinstance(expr, Field) or not isinstance(expr, ops.Future):
        return (), expr
    dist = expr.dist
    if isinstance(expr, ops.Interpolate):
        reds, inner = hoist(expr.operand)
        b = expr.operand.domain.by_axis[expr.axis]
        if b is None:
            return (reds, inner) if reds else ((), expr)
        if b.separable:
            return _merged(reds, [("interp", expr.axis, resolve_position(b, expr.position))]), inner
        return (reds, ops.Interpolate(inner, expr.coord, expr.position)) if reds else ((), expr)
    if isinstance(expr, ops.Integrate):
        reds, inner = hoist(expr.operand)
        kind = "ave" if expr.average else "integ"
        new, jac = [], []
        for ax in expr.axes:
            b = expr.operand.domain.by_axis[ax]
            if b is None:
                raise ValueError("cannot integrate along an axis without a basis")
            if b.separable:
                new.append((kind, ax))
            else:
                jac.append(dist.coords[ax])
        if not new and not reds:
            return (), expr
        if jac:
            inner = type(expr)(inner, tuple(jac))
        return _merged(reds, new), inner
    if isinstance(expr, ops.Differentiate):
        reds, inner = hoist(expr.operand)
        if not reds:
            return (), expr
        if expr.axis in _axes(reds):
            return reds, ops.Multiply(0.0, inner)           # d/dx of something without x (as in the reference: zero)
        return reds, ops.Differentiate(inner, expr.coord)
    if isinstance(expr, (ops.Component, ops.Trace, ops.TransposeComponents, ops.Skew, ops.Lift)):
        reds, inner = hoist(expr.operand)
        return (reds, type(expr)(inner, *expr.args[1:])) if reds else ((), expr)
    if isinstance(expr, ops.Multiply) and expr.number is not None:
        reds, inner = hoist(expr.args[1])
        return (reds, ops.Multiply(expr.number, inner)) if reds else ((), expr)
    if isinstance(expr, (ops.Multiply, ops.DotProduct)):
        a, b = expr.args
        if ops._is_const_field(a, None):
            reds, inner = hoist(b)
            return (reds, type(expr)(a, inner)) if reds else ((), expr)
        if ops._is_const_field(b, None):
            reds, inner = hoist(a)
            return (reds, type(expr)(inner, b)) if reds else ((), expr)
        return (), expr                                     # nonlinear: evaluated on the grid of its own domain
    if isinstance(expr, ops.Add):
        a, b = expr.args
        ra, ia = hoist(a)
        rb, ib = hoist(b)
        if ra and ra == rb:
            return ra, ops.Add(ia, ib)
        return (), expr
    return (), expr                                         # gradients, divergences, ...: the reductions stay below


def has_fourier_reduction(expr):
    """Does the tree hold a reduction along a Fourier axis of a Cartesian domain?"""
    if isinstance(expr, Field) or not isinstance(expr, ops.Future):
        return False
    if isinstance(expr, ops.Interpolate):
        b = expr.operand.domain.by_axis[expr.axis]
        if b is not None and b.separable:
            return True
    elif isinstance(expr, ops.Integrate):
        for ax in expr.axes:
            b = expr.operand.domain.by_axis[ax]
            if b is not None and b.separable:
                return True
    return any(has_fourier_reduction(a) for a in expr.args if isinstance(a, ops.Future))


def check_single_rank(expr, name=None):
    """Reductions of a sharded axis need a collective: refused on several ranks, before any device work."""
    dist = getattr(expr, "dist", None)
    if dist is None or getattr(dist, "size", 1) == 1 or not isinstance(expr, ops.Future):
        return
    if has_fourier_reduction(expr):
        raise NotImplementedError("task %r reduces along a Fourier axis (interpolation / average / integral): on several "
                                  "ranks this needs a collective, which is not implemented" % (name or repr(expr),))


def reduction_weights(domain, red):
    """(n, host weights [1][n]) of one reduction on coefficient data of `domain`: the full interpolation vector, or the
    single weight of the k = 0 cosine mode for an integral / average (only that slab is read)."""
    b = domain.by_axis[red[1]]
    if red[0] == "interp":
        return b.coeff_size, b.interpolate_vector(red[2])[None, :]
    scale = b.integrate_vector()[0]
    if red[0] == "ave":
        scale = scale / b.length
    return 1, np.array([[scale]])
