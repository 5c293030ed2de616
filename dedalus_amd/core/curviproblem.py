"""
Problem front end shared by the sphere (core/sphere.py) and the shell (core/shell.py): the namespace, equation parsing
and the split of a linear LHS into dt-terms (M) and the rest (L), {variable index: term list} each.  The expression
nodes it walks are those of core/curvioperand.py; a geometry declares its operand base class and operator names and the
few places where the two really differ.
"""

import numbers

import numpy as np

from .curvioperand import NonlinearError
from .packbase import PackBase
from .problems import _split_equation


class MatvecPack(PackBase):
    """matvec interface the shared timesteppers use (pack.matvec(id, x, y)) over device term lists; no capability
    of core/packbase.py beyond that"""

    def __init__(self):
        self.mats = []

    def add(self, dev_terms):
        self.mats.append(dev_terms)
        return len(self.mats) - 1

    def matvec(self, mid, x, y):
        self.mats[mid].apply(x, y)


class CurvilinearProblem:
    operand_type = None                              # the geometry's operand base class (core/curvioperand.py)
    operators = {}                                   # names the equations may use

    def __init__(self, variables, namespace=None, time="t"):
        self.variables = list(variables)
        self.dist = self.variables[0].dist
        self.equations = []
        self.namespace = dict(self.operators, np=np, numpy=np)
        if namespace:
            self.namespace.update(namespace)
        for v in self.variables:
            if v.name:
                self.namespace[v.name] = v

    # ---- what differs between the geometries -------------------------------------------------------------------------
    def _lin(self, node):
        """({variable index: term list}, is it a dt term) of one term of a left-hand side"""
        return node.lin(self.variables)

    def _numeric_rhs(self, rhs):
        """F of a right-hand side that is a number"""
        raise NotImplementedError

    def _operand_rhs(self, lhs, rhs):
        """F of a right-hand side that is an operand"""
        return rhs

    def _equation_keys(self, lhs):
        """the geometry's own entries of the equation dict"""
        return {}

    # -------------------------------------------------------------------------------------------------------------------
    def _parse(self, side):
        if isinstance(side, (self.operand_type, numbers.Number)):
            return side
        return eval(side, dict(self.namespace))

    def add_equation(self, equation, condition=None):
        if isinstance(equation, str):
            lhs_s, rhs_s = _split_equation(equation)
            lhs, rhs = self._parse(lhs_s), self._parse(rhs_s)
        else:
            lhs, rhs = [self._parse(s) for s in equation]
        if not isinstance(lhs, self.operand_type):
            raise ValueError("LHS must involve the problem variables")
        if isinstance(rhs, self.operand_type) and rhs.has_dt():
            raise ValueError("time derivatives must be on the LHS")
        M, L = self._linearize(lhs)
        if isinstance(rhs, numbers.Number):
            F = self._numeric_rhs(rhs)
        else:
            if rhs.rank != lhs.rank:
                raise ValueError("LHS and RHS tensor signatures differ")
            F = self._operand_rhs(lhs, rhs)
        eq = dict(lhs=lhs, rank=lhs.rank, ncomp=lhs.ncomp, M=M, L=L, F=F,
                  string=equation if isinstance(equation, str) else None, **self._equation_keys(lhs))
        self.equations.append(eq)
        return eq

    def _linearize(self, lhs):
        """Split the LHS sum into dt-terms (M) and the rest (L): {variable index: term list} each."""
        terms = []

        def flatten(node, scale):
            if isinstance(node, self.operand_type.add_type):
                for a in node.args:
                    flatten(a, scale)
            elif isinstance(node, self.operand_type.scale_type):
                flatten(node.arg, scale * node.a)
            else:
                terms.append((scale, node))
        flatten(lhs, 1.0)
        M, L = {}, {}
        for scale, node in terms:
            try:
                d, isdt = self._lin(node)
            except NonlinearError as e:
                raise ValueError("LHS must be linear in the problem variables: %s" % e)
            tgt = M if isdt else L
            for i, tl in d.items():
                tl = tl.scaled(scale)
                tgt[i] = tgt[i] + tl if i in tgt else tl
        return M, L

    def build_solver(self, *args, **kw):
        return self.solver_class(self, *args, **kw)
