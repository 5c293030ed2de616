"""
Operand algebra shared by the expression trees of the sphere (core/sphere.py) and the shell (core/shell.py): the arithmetic
of the operand base, the scaling, sum and time-derivative nodes and the index table of a grid product.  A geometry
subclasses these and adds what really differs: its fields, transforms, linear operators and term lists.

The protocol of a node: dist, basis, rank, args; eval_c() / eval_g() -> device coefficient / grid data; lin(variables) ->
({variable index: term list}, is it a dt term), raising NonlinearError where the node is not linear in the variables.
"""

import numbers

import numpy as np


class NonlinearError(ValueError):
    """raised by an operand's lin(): it is not linear in the problem variables"""


class CurviOperand:
    """Expression node.  A geometry's base class sets scale_type, add_type (its Scale and Add nodes) and product(a, b),
    dot(a, b) (its grid products) once they exist, and gives _result_field()."""
    __array_priority__ = 100.0
    scale_type = add_type = product = dot = None

    def __add__(self, other):
        return self.add_type.make(self, other)

    __radd__ = __add__

    def __sub__(self, other):
        return self.add_type.make(self, -1 * other if isinstance(other, CurviOperand) else -other)

    def __rsub__(self, other):
        return self.add_type.make(-1 * self, other)

    def __neg__(self):
        return self.scale_type(-1.0, self)

    def __mul__(self, other):
        if isinstance(other, numbers.Number):
            return self.scale_type(other, self)
        if isinstance(other, CurviOperand):
            return self.product(self, other)
        return NotImplemented

    def __rmul__(self, other):
        if isinstance(other, numbers.Number):
            return self.scale_type(other, self)
        return NotImplemented

    def __truediv__(self, other):
        if isinstance(other, numbers.Number):
            return self.scale_type(1.0 / other, self)
        return NotImplemented

    def __matmul__(self, other):
        return self.dot(self, other)

    def has_dt(self):
        return any(a.has_dt() for a in getattr(self, "args", ()) if isinstance(a, CurviOperand))

    def evaluate(self):
        f = self._result_field()
        f._set_device_coeff(self.eval_c())
        return f


class Scale(CurviOperand):
    """a * arg"""

    def __init__(self, a, arg):
        self.a, self.arg, self.args = float(a), arg, (arg,)
        self.dist, self.basis, self.rank = arg.dist, arg.basis, arg.rank

    def eval_c(self):
        ex = self.dist.executor
        c = self.arg.eval_c()
        out = ex.empty(tuple(c.shape))
        ex.lincomb(out, [c], [self.a])
        return out

    def lin(self, variables):
        d, dt = self.arg.lin(variables)
        return {i: tl.scaled(self.a) for i, tl in d.items()}, dt


class Add(CurviOperand):
    """a + b.  The geometry's node sets `geometry` (its word in the refusal of a number), the basis of the sum and how the
    sum is evaluated."""
    geometry = None

    @classmethod
    def make(cls, a, b):
        for x, y in ((a, b), (b, a)):
            if isinstance(x, numbers.Number):
                if x == 0:
                    return y
                raise NotImplementedError("adding a number to a %s field" % cls.geometry)
        return cls(a, b)

    def __init__(self, a, b):
        if a.rank != b.rank:
            raise ValueError("cannot add tensors of different rank")
        self.dist, self.rank, self.args = a.dist, a.rank, (a, b)

    def lin(self, variables):
        out, anydt = {}, None
        for a in self.args:
            d, dt = a.lin(variables)
            if anydt is None:
                anydt = dt
            elif anydt != dt:
                raise NonlinearError("cannot mix dt and non-dt terms inside one sum node; write them as separate terms")
            for i, tl in d.items():
                out[i] = out[i] + tl if i in out else tl
        return out, bool(anydt)


class Dt(CurviOperand):
    """dt(arg): exists on a left-hand side only"""

    def __init__(self, arg):
        self.arg, self.args = arg, (arg,)
        self.dist, self.basis, self.rank = arg.dist, arg.basis, arg.rank

    def has_dt(self):
        return True

    def lin(self, variables):
        d, dt = self.arg.lin(variables)
        if dt:
            raise NonlinearError("nested time derivatives")
        return d, True

    def eval_c(self):
        raise ValueError("dt() cannot be evaluated")


def bilinear_terms(ncomp_per_index, rank_a, rank_b, contract):
    """((out, ia, ib, coef) list, number of output components) of the grid-space product of coordinate components: outer
    product (contract False) or contraction of the last index of a with the first of b (DotProduct, core/arithmetic.py:
    246-251, 855-866).  The order of the list is the summation order on the device."""
    indices = lambda rank: list(np.ndindex(*((ncomp_per_index,) * rank)))
    ia_list, ib_list = indices(rank_a), indices(rank_b)
    out_list = indices(rank_a + rank_b - (2 if contract else 0))
    terms = []
    for ia, ta in enumerate(ia_list):
        for ib, tb in enumerate(ib_list):
            if contract:
                if ta[-1] != tb[0]:
                    continue
                tc = tuple(ta[:-1]) + tuple(tb[1:])
            else:
                tc = tuple(ta) + tuple(tb)
            terms.append((out_list.index(tc), ia, ib, 1.0))
    return terms, len(out_list)
