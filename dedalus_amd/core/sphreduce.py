"""
Reduced analysis tasks of the curvilinear field systems (core/shell.py, core/sphere.py): the parts both share.

Reference (core/basis.py): InterpolateAzimuth :5578-5634, InterpolateColatitude :5637-5736, SphereAzimuthalAverage /
SphericalAzimuthalAverage :5238-5293, SphereAverage / SphericalAverage :5296-5350.  There the two interpolations act on
grid data (a forward matrix, then the interpolation row) and return fields locked to the scales they were formed at; the
averages are spectral operators (the m = 0 / ell = 0 coefficients).  Here every one of them is a contraction of data a
transform stage already holds on the device:

* f(phi = phi0): the azimuthal coefficients [comp][2 m + part][rest] contracted with interleaved cos m phi0, -sin m phi0
  (the convention of RealFourier.interpolate_vector; no Nyquist mode is stored) -- ddh_axis_contract.
* f(theta = theta0): the spin components [comp][2 m + part][ell][rest] contracted along ell with Y_l^{m,s}(theta0), one
  weight row per (spin weight, m), read from l = max(m, |s|) on -- ddh_axis_contract_rows.
* ave(f, phi): the m = 0 slab, gathered by pointer and stride (ddh_axis_contract, n = 1), transformed alone.

An executor without the two contraction entry points (the NumPy oracle of the tests) takes the NumPy expressions below
for the contraction step only; everything around it is the same code.
"""

import numbers

import numpy as np

from ..tools import sphere as sph
from .curvioperand import NonlinearError


def azimuth_weights(nm, phi0):
    """[1][2 nm]: interleaved cos(m phi0), -sin(m phi0), m = 0 .. nm - 1"""
    m = np.arange(nm)
    w = np.zeros((1, 2 * nm))
    w[0, 0::2] = np.cos(m * phi0)
    w[0, 1::2] = -np.sin(m * phi0)
    return w


def colatitude_rows(sb, spins, m0, nml, theta0):
    """Weight rows of f(theta = theta0) for data [component][2 ml + part][ell]: (w [nrows][nl], row [ncomp * 2 nml] int32,
    kmin [nrows] int32), one row per (spin weight, m), kmin the first ell that holds data (nl where there is none)."""
    z = np.cos(theta0)
    index, w, kmin = {}, [], []
    row = np.zeros((len(spins), nml, 2), dtype=np.int32)
    for i, s in enumerate(spins):
        for ml in range(nml):
            m = m0 + ml
            if (s, m) not in index:
                index[(s, m)] = len(w)
                lmin = min(max(m, abs(s)), sb.nl)
                v = np.zeros(sb.nl)
                if lmin < sb.nl:
                    v[lmin:] = np.asarray(sph.harmonics(sb.Lmax, m, s, z)[:, 0], dtype=np.float64)
                w.append(v)
                kmin.append(lmin)
            row[i, ml, :] = index[(s, m)]
    return np.array(w), np.ascontiguousarray(row.reshape(-1)), np.array(kmin, dtype=np.int32)


def _cached(store, ex, key, make):
    key = ("sphreduce", id(ex)) + key
    if key not in store:
        store[key] = make()
    return store[key]


def contract(ex, store, x, outer, n, inner, w, ostride=None):
    """out[o][j][i] = sum_k w[j][k] x[o][k][i] with host weights w [nw][n] (device copies cached in `store`)"""
    ostride = n * inner if ostride is None else int(ostride)
    if getattr(ex, "axis_contract", None) is None:
        h = np.asarray(ex.download(x)).reshape(-1)
        blocks = np.stack([h[o * ostride:o * ostride + n * inner].reshape(n, inner) for o in range(outer)])
        return ex.from_host(np.ascontiguousarray(np.einsum("jk,oki->oji", w, blocks)))
    w_d = _cached(store, ex, ("w", w.shape, w.tobytes()), lambda: ex.from_host(w))
    return ex.axis_contract(x, outer, n, inner, w_d, ostride=ostride)


def contract_rows(ex, store, key, x, outer, n, inner, make_rows):
    """out[o][i] = sum_{k >= kmin[row[o]]} w[row[o]][k] x[o][k][i]; make_rows() -> host (w, row, kmin), cached under key"""
    w, row, kmin = _cached(store, None, ("rows",) + key, make_rows)
    if getattr(ex, "axis_contract_rows", None) is None:
        h = np.asarray(ex.download(x)).reshape(outer, n, inner)
        live = np.arange(n)[None, :] >= kmin[row][:, None]
        h = np.where(live[:, :, None], h, 0.0)                  # (entries below kmin are not read on the device)
        return ex.from_host(np.ascontiguousarray(np.einsum("ok,oki->oi", w[row], h)))
    dev = _cached(store, ex, ("rows_d",) + key,
                  lambda: (ex.from_host(w), ex.from_host_int32(row), ex.from_host_int32(kmin)))
    return ex.axis_contract_rows(x, outer, n, inner, *dev)


def reduction_refused(what, inner):
    """the error of a reduction (`what`) of an operand that is a reduced task already (`inner`: its name)"""
    return NotImplementedError("%s of a reduced operand (%s): reductions of reductions are not supported" % (what, inner))


class ReducedResult:
    """What the reduced tasks of both systems share: an ANALYSIS-ONLY operand whose grid data keep the reduced axes with
    size one (constant axes of an output file).  Subclasses set `what`, `const_axes`, and give `_device(scales)` -> device
    array [ncomp][axes ...] at the requested scales; evaluate() returns a copy bound to the operand's data."""

    what = "reduction"
    const_axes = ()
    dim = 3

    def _init(self, arg, **params):
        if isinstance(arg, ReducedResult):
            raise reduction_refused(self.what, arg.what)
        self.args, self.params = (arg,), params
        self.dist, self.basis, self.rank = arg.dist, arg.basis, arg.rank
        self.scales = (1.0,) * self.dim
        self._field = self._grid = None
        self._bound = False
        self._host = {}

    def __call__(self, **kw):
        raise reduction_refused("interpolation", self.what)

    def _remedy(self, scales):
        if scales is None:
            return (1.0,) * self.dim
        if isinstance(scales, numbers.Number):
            return (float(scales),) * self.dim
        return tuple(float(s) for s in scales)

    def evaluate(self):
        out = type(self).__new__(type(self))
        out._init(self.args[0], **self.params)
        arg = self.args[0]
        out._bound = True
        g = self._native_grid(arg) if self.from_grid else None
        if g is not None:
            out._grid = g                                       # formed on the dealiased grid: reduced from there
        elif isinstance(arg, self.field_type):
            out._field = arg                                    # a field: its own (current) data
        else:
            out._field = arg.evaluate()
        return out

    # The interpolations act on grid data in the reference: an operand formed on the dealiased grid (a product) is reduced
    # from there at the dealias scales, truncated along the interpolated axis (and the azimuth) only; at other scales, and
    # for the averages (spectral operators), it passes through its truncated coefficients.
    from_grid = False

    def _coeff_field(self):
        """the operand as a field with coefficient data (a grid-formed operand: transformed, i.e. truncated, on demand)"""
        if self._field is None:
            self._field = self._field_from_grid(self._grid)
        return self._field

    def require_coeff_space(self):
        if self._field is not None:
            self._field.require_coeff_space()

    def change_scales(self, scales):
        self.scales = self._remedy(scales)

    preset_scales = change_scales

    def __getitem__(self, key):
        if isinstance(key, tuple):
            key, scales = key
            self.change_scales(scales)
        if key not in ("g", "grid"):
            raise NotImplementedError("coefficient data of a reduced task (%s)" % self.what)
        if not self._bound:
            return self.evaluate()[("g", self.scales)]
        if self.scales not in self._host:
            d = self._device(self.scales)
            ex = self.dist.executor
            self._host[self.scales] = np.array(ex.download(d)).reshape(self._tensor_shape() + tuple(d.shape[1:]))
        return self._host[self.scales]

    def eval_c(self):
        raise NotImplementedError("%s is an output task, not a term of an equation" % self.what)

    def eval_g(self):
        raise NotImplementedError("%s is an output task, not a factor of a product" % self.what)

    def has_dt(self):
        return False

    def lin(self, variables):
        raise NonlinearError("%s in an equation" % self.what)
