"""CFL and global flow properties (dedalus/extras/flow_tools.py:49-233).

The CFL frequency max_x sum_i |u_i| / dx_i is reduced on the device (ddh_grid_cfl) from the
dealias-scale grid velocity, with the reference's spacings (CartesianAdvectiveCFL,
core/basis.py:6078-6111) and the reference's scheduling: frequencies are sampled at the start of a step
whenever iteration % cadence == 0 (the dictionary handler of flow_tools.py:176) and consumed by
compute_timestep() one step later (flow_tools.py:183-207).  Several velocities and scalar frequencies (add_velocity
more than once, add_frequency; flow_tools.py:199-204, 216-233) are summed per grid point and reduced in one launch
(ddh_grid_cfl_sum), on boxes, shells and the sphere; one velocity alone keeps the single-velocity reductions."""

import numpy as np


def _nan_max(a, b):
    """max that keeps a NaN (np.max semantics, the reducer of flow_tools.py:32-47): Python's max(0.0, nan) is 0.0, and a
    dropped NaN frequency would turn a blown-up velocity into the largest timestep instead of leaving dt unchanged."""
    return a if a != a else (b if (b != b or b > a) else a)


class GlobalFlowProperty:
    """Reductions of grid-space expressions every `cadence` iterations (flow_tools.py:49-111)."""

    def __init__(self, solver, cadence=1):
        self.solver = solver
        self.cadence = cadence
        self.properties = {}
        self._cache = {}
        self._cache_iter = None
        self._sampled = {}
        # the reference evaluates the properties with a dictionary handler scheduled at iter % cadence == 0, i.e. at
        # the START of those steps (flow_tools.py:60-63, core/solvers.py evaluate_scheduled); max()/min()/... read the
        # last scheduled evaluation
        if hasattr(solver, "_step_hooks"):
            solver._step_hooks.append(self._sample)

    def add_property(self, property, name, precompute_integral=False):
        self.properties[name] = property

    def _evaluate(self, name):
        """(min, max, sum, count) of the property's grid data.  The reduction runs on the device (ddh_grid_reduce, the
        local part of GlobalArrayReducer, flow_tools.py:32-47): 24 bytes reach the host, not the grid."""
        expr = self.properties[name]
        f = expr.evaluate() if hasattr(expr, "evaluate") else expr
        ex = self.solver.ex
        if hasattr(f, "require_grid_space") and hasattr(ex, "reduce3"):
            g = f.require_grid_space(f.scales)
            n = int(g.numel()) if hasattr(g, "numel") else int(np.size(g))
            mn, mx, sm = ex.reduce3(g)
            return (mn, mx, sm, n)
        g = np.asarray(f["g"])                       # operands evaluated on the host (analysis-only expressions)
        return (float(g.min()), float(g.max()), float(g.sum()), int(g.size))

    def _sample(self, solver):
        if solver.iteration % self.cadence == 0:
            for name in self.properties:
                self._sampled[name] = self._evaluate(name)

    def _stats(self, name):
        if name in self._sampled:
            return self._sampled[name]
        it = self.solver.iteration
        if self._cache_iter != it:
            self._cache, self._cache_iter = {}, it
        if name not in self._cache:
            self._cache[name] = self._evaluate(name)
        return self._cache[name]

    def _reduce(self, val, op):
        pc = getattr(self.solver.dist, "pcomm", None)
        if pc is None:
            return float(val)
        return pc.allreduce_max(val) if op == "max" else (-pc.allreduce_max(-val) if op == "min" else pc.allreduce_sum(val))

    def min(self, name):
        return self._reduce(self._stats(name)[0], "min")

    def max(self, name):
        return self._reduce(self._stats(name)[1], "max")

    def grid_average(self, name):
        st = self._stats(name)
        return self._reduce(st[2], "sum") / self._reduce(st[3], "sum")

    def volume_integral(self, name):
        from ..core.operators import Integrate
        f = Integrate(self.properties[name]).evaluate()
        return float(np.asarray(f["g"]).ravel()[0])


class CFL:
    """Adaptive timestep from the sum of advective and scalar CFL frequencies (flow_tools.py:113-233)."""

    def __init__(self, solver, initial_dt, cadence=1, safety=1.0, max_dt=np.inf, min_dt=0.0, max_change=np.inf,
                 min_change=0.0, threshold=0.0):
        self.solver = solver
        self.stored_dt = initial_dt
        self.cadence, self.safety = cadence, safety
        self.max_dt, self.min_dt = max_dt, min_dt
        self.max_change, self.min_change, self.threshold = max_change, min_change, threshold
        self.velocities = []
        self.frequencies = []         # ("velocity" | "scalar", operand) in the order added: the order of the sum
        self._max_freq = None
        self._setup = {}
        self._terms = None
        solver._step_hooks.append(self._sample)

    def add_velocity(self, velocity):
        """Adds the grid-crossing frequency of a vector field (flow_tools.py:220-233: one more frequency)."""
        if len(velocity.tensorsig) != 1:
            raise ValueError("Velocity must be a vector")
        self.velocities.append(velocity)
        self.frequencies.append(("velocity", velocity))
        self._terms = None

    def add_frequency(self, freq):
        """Adds an on-grid scalar frequency, a field or an expression (flow_tools.py:216-218)."""
        if len(getattr(freq, "tensorsig", ())) != 0:
            raise ValueError("Frequency must be a scalar")
        self.frequencies.append(("scalar", freq))
        self._terms = None

    def _spacings(self, u):
        """Device arrays 1/dx per velocity component at the dealias grid (basis.py:6083-6106); None for a component
        along an axis without a basis (infinite spacing, basis.py:6103-6104)."""
        key = id(u)
        if key in self._setup:
            return self._setup[key]
        dist, ex = self.solver.dist, self.solver.ex
        scales = u.domain.dealias
        inv, comp_axis = [], []
        for c in u.tensorsig[0].coords:
            ax = dist.coord_axis(c)
            b = u.domain.by_axis[ax]
            if b is None:
                inv.append(None)
                comp_axis.append(None)
                continue
            N = b.grid_size(b.dealias)
            if b.separable:
                dx = np.full(N, b.dealias * b.length / N)
            elif b.a0 == b.b0 == -0.5 and b.a == b.b == -0.5:
                theta = np.pi * (np.arange(N) + 0.5) / N
                dx = b.dealias * b.stretch * np.sin(theta) * np.pi / N
            else:
                dx = np.gradient(b.global_grid(b.dealias), edge_order=2) * b.dealias
            if ax == dist.shard_grid_axis:
                lo, hi = dist.local_block(N)
                dx = dx[lo:hi]
            inv.append(ex.from_host(1.0 / dx))
            comp_axis.append(list(dist.storage_order).index(ax))
        self._setup[key] = (inv, comp_axis, scales)
        return self._setup[key]

    def _sample(self, solver):
        """Called at the start of every step (the reference evaluates its frequency handler there)."""
        if solver.iteration % self.cadence != 0 or not self.frequencies:
            return
        ex = solver.ex
        fmax = None
        if len(self.frequencies) == 1 and self.frequencies[0][0] == "velocity":
            # one velocity: the single-velocity reductions (ddh_grid_cfl, ddh_grid_cfl_spherical)
            u = self.velocities[0]
            if hasattr(u, "cfl_frequency_max"):             # shell fields carry their own CFL reduction
                fmax = _nan_max(0.0, u.cfl_frequency_max())
            elif not hasattr(u, "cfl_term"):
                f = u if hasattr(u, "grid_data") else u.evaluate()
                inv, comp_axis, scales = self._spacings(f)
                if None not in comp_axis:
                    g = f.grid_data(scales)
                    shape = f.domain.storage_grid_shape(scales)
                    fmax = 0.0 + ex.cfl_max(g, f.ncomp, shape, inv, comp_axis)
        if fmax is None:
            fmax = self._sample_sum(ex)
        if getattr(solver.dist, "pcomm", None) is not None:
            fmax = solver.dist.pcomm.allreduce_max(fmax)
        self._max_freq = fmax

    def _cartesian_term(self, kind, op):
        """(static part of the term, own storage grid shape, function giving the current device data) of a Cartesian
        operand; an expression is evaluated on the device at every sample, at its dealias scales (flow_tools.py:218)."""
        field = (lambda: op) if hasattr(op, "grid_data") else op.evaluate
        f = field()
        scales = f.domain.dealias
        shape = tuple(int(n) for n in f.domain.storage_grid_shape(scales))
        if kind == "velocity":
            inv, comp_axis, _ = self._spacings(f)
            term = dict(kind="velocity", comp_axis=list(comp_axis), inv=list(inv))
        else:
            if f.tensorsig:
                raise ValueError("Frequency must be a scalar")
            term = dict(kind="scalar")
        return term, shape, lambda: field().grid_data(scales)

    def _build_terms(self):
        """The term list of ddh_grid_cfl_sum for the operands added so far, in the order added: built once, only the data
        pointers change from sample to sample.  Operands on different domains follow NumPy broadcasting over the
        storage axes, as the reference's sum of grid arrays does; an operand with one point along an axis where the
        others have more is flagged as broadcast there and never expanded."""
        if len(self.frequencies) > 8:
            raise ValueError("at most 8 CFL frequencies")
        parts = []
        for kind, op in self.frequencies:
            if hasattr(op, "cfl_term"):                      # sphere and shell operands describe themselves
                parts.append(op.cfl_term(kind == "velocity"))
            else:
                parts.append(self._cartesian_term(kind, op))
        shapes = [shape for _, shape, _ in parts]
        if len(set(len(s) for s in shapes)) != 1:
            raise ValueError("CFL frequencies on grids of different dimension: %r" % (shapes,))
        try:
            common = tuple(int(n) for n in np.broadcast_shapes(*shapes))
        except ValueError:
            raise ValueError("CFL frequencies on incompatible grids: %r" % (shapes,)) from None
        terms, getters = [], []
        for term, shape, data in parts:
            term["bcast"] = [int(own == 1 and full != 1) for own, full in zip(shape, common)]
            terms.append(term)
            getters.append(data)
        return terms, getters, common

    def _sample_sum(self, ex):
        """max over the grid of the sum of all frequencies: one ddh_grid_cfl_sum launch."""
        if not hasattr(ex, "cfl_sum_max"):
            raise NotImplementedError("executor %r has no fused CFL reduction (cfl_sum_max)" % getattr(ex, "name", ex))
        if self._terms is None:
            self._terms = self._build_terms()
        terms, getters, shape = self._terms
        return ex.cfl_sum_max([dict(t, data=data()) for t, data in zip(terms, getters)], shape)

    def compute_timestep(self):
        """flow_tools.py:183-207"""
        it = self.solver.iteration
        if (it - 1) % self.cadence == 0:
            if (it - 1) <= self.solver.initial_iteration or self._max_freq is None:
                return self.stored_dt
            dt = np.inf if self._max_freq == 0.0 else 1.0 / self._max_freq
            dt *= self.safety
            dt = min(dt, self.max_dt, self.max_change * self.stored_dt)
            dt = max(dt, self.min_dt, self.min_change * self.stored_dt)
            if abs(dt - self.stored_dt) > self.threshold * self.stored_dt:
                self.stored_dt = dt
        return self.stored_dt

    compute_dt = compute_timestep
