"""
Spherical shells: SphericalCoordinates, ShellBasis and tensor fields with their device transforms
(the field-level transform path of BASELINE config 5).

Reference sequence (core/basis.py): backward = ShellBasis.backward_transform_radius (:4488-4508: radial Jacobi
transform per regularity component, regularity -> spin recombination Q(ell), radial factor (dR/r)^k), then the
colatitude step of the angular basis (SWSH per spin weight + spin -> coordinate recombination, :3134-3153, with
the 3 x 3 U of SphericalCoordinates core/coords.py:338-351), then the azimuthal FFT; forward is the mirror.

On the device a field is [component][2 m + part][ell][n] with n the radial index (contiguous); the angular
(m, ell) bookkeeping and the user-facing packed coefficient layout are those of core/sphere.py.  Every step is one
launch over the whole field: ddh_cheb_* / ddh_mmt_apply (radius), ddh_regularity_recombine with the radial
factor fused, ddh_grouped_mmt_* with the radial points as GEMM columns, ddh_spin_recombine, ddh_rfft_*.
Operators and the per-ell radial solves of the shell are not built yet.
"""

import logging
import numbers
import time as _time

import numpy as np

from ..tools import sphere as sph
from . import curvilinear, sphreduce
from .basis import Jacobi
from .coords import Coordinate, SpinCoordinates
from .curvioperand import Add, CurviOperand, Dt, NonlinearError, Scale, bilinear_terms
from .curviproblem import CurvilinearProblem, MatvecPack
from .ivp_common import LUSlotSolver
from .mirror import HostMirror
from .sphere import S2Coordinates, SphereBasis


logger = logging.getLogger(__name__)


class SphericalCoordinates(SpinCoordinates):
    """(azimuth, colatitude, radius); spin and regularity component ordering (-, +, 0)  (core/coords.py:300-390)."""
    dim = 3
    spin_ordering = (-1, +1, 0)
    reg_ordering = (-1, +1, 0)
    # coordinate (phi, theta, r) -> spin (-, +, 0) components: u[+-] = (u[theta] +- i u[phi]) / sqrt 2, u[0] = u[r]
    U = np.array([[-1j, 1, 0], [+1j, 1, 0], [0, 0, np.sqrt(2)]]) / np.sqrt(2)

    def __init__(self, azimuth, colatitude, radius):
        self.names = (azimuth, colatitude, radius)
        self.azimuth = Coordinate(azimuth, cs=self)
        self.colatitude = Coordinate(colatitude, cs=self)
        self.radius = Coordinate(radius, cs=self)
        self.coords = (self.azimuth, self.colatitude, self.radius)
        self.S2coordsys = S2Coordinates(azimuth, colatitude)


class ShellBasis:
    """Shell: SWSH in angle x Jacobi(alpha + k) in radius on [Ri, Ro]  (core/basis.py:4380-4440, 3682-3816)."""

    def __init__(self, coordsys, shape, dtype=np.float64, radii=(1, 2), alpha=(-0.5, -0.5), dealias=(1, 1, 1), k=0,
                 azimuth_library=None, colatitude_library=None, radius_library=None):
        if not isinstance(coordsys, SphericalCoordinates):
            raise ValueError("Shell coordsys must be SphericalCoordinates.")
        if np.dtype(dtype) != np.float64:
            raise NotImplementedError("shell fields: float64 only")
        if min(radii) <= 0:
            raise ValueError("Radii must be positive.")
        if isinstance(dealias, numbers.Number):
            dealias = (dealias,) * 3
        self.coordsys, self.shape, self.dtype = coordsys, tuple(int(s) for s in shape), np.dtype(dtype)
        self.radii, self.alpha, self.k = tuple(radii), tuple(alpha), int(k)
        self.dealias = tuple(float(d) for d in dealias)
        self.Nr = self.shape[2]
        self.dR = self.radii[1] - self.radii[0]
        self.rho = (self.radii[1] + self.radii[0]) / self.dR
        self.sphere = SphereBasis(coordsys.S2coordsys, self.shape[:2], dtype=dtype, radius=1, dealias=self.dealias[:2])
        # radial Jacobi basis: coefficients in (alpha + k), grid of alpha
        self.radial = Jacobi(coordsys.radius, size=self.Nr, bounds=self.radii, a=alpha[0] + k, b=alpha[1] + k,
                             a0=alpha[0], b0=alpha[1], dealias=self.dealias[2])
        self._plans = {}

    @property
    def outer_surface(self):
        return self.S2_basis(self.radii[1])

    @property
    def inner_surface(self):
        return self.S2_basis(self.radii[0])

    @property
    def radial_basis(self):
        """Tag for fields that depend on the radius only (NCCs: er, rvec; core/basis.py ShellRadialBasis)."""
        key = ("radial",)
        if key not in self._plans:
            self._plans[key] = RadialBasis(self)
        return self._plans[key]

    @property
    def meridional_basis(self):
        """Tag for axisymmetric fields (the reference's clone with one azimuthal point, core/basis.py:4470-4472), which
        rotating-shell scripts use for the rotation axis: ez['g'][1] = -sin(theta), ez['g'][2] = cos(theta).  A field
        built on it is STORED ON THE FULL SHELL BASIS (its grid data has the full azimuthal size, and values assigned
        from (1, Ntheta, Nr) arrays broadcast along phi); it can be used wherever a shell field can, in particular as
        a factor of cross()."""
        key = ("meridional",)
        if key not in self._plans:
            self._plans[key] = MeridionalBasis(self)
        return self._plans[key]

    def S2_basis(self, radius=1):
        key = ("surf", float(radius))
        if key not in self._plans:
            self._plans[key] = SurfaceBasis(self, radius)
        return self._plans[key]

    def derivative_basis(self, order=1):
        return self.clone_with(k=self.k + order)

    def clone_with(self, **kw):
        args = dict(shape=self.shape, radii=self.radii, alpha=self.alpha, dealias=self.dealias, k=self.k)
        args.update(kw)
        key = ("clone", args["k"], tuple(args["shape"]))
        root = getattr(self, "_root", self)
        if key not in root._plans:
            b = ShellBasis(self.coordsys, dtype=self.dtype, **args)
            b._root = root
            if tuple(args["shape"]) == tuple(root.shape):
                b.sphere = root.sphere
            root._plans[key] = b
        return root._plans[key]

    def grid_shape(self, scales):
        return self.sphere.grid_shape(scales[:2]) + (int(np.ceil(scales[2] * self.Nr)),)

    def grids(self, scales):
        phi, theta = self.sphere.grids(scales[:2])
        return phi, theta, self.radius_grid(scales[2])

    def radius_grid(self, scale):
        from ..tools import jacobi
        N = int(np.ceil(scale * self.Nr))
        z, _ = jacobi.quadrature(N, self.alpha[0], self.alpha[1])
        return (self.dR / 2 * (np.asarray(z, dtype=np.float64) + self.rho))

    @staticmethod
    def spin_indices(rank):
        return list(np.ndindex(*((3,) * rank)))

    @staticmethod
    def spin_totals(rank):
        return [sum((-1, +1, 0)[a] for a in idx) for idx in np.ndindex(*((3,) * rank))]

    def recombination_matrix(self, rank, forward):
        U = SphericalCoordinates.U_forward(rank)
        if not forward:
            U = U.T.conj()
        return np.kron(U.real, np.eye(2)) + np.kron(U.imag, np.array([[0.0, -1.0], [1.0, 0.0]]))

    def colatitude_plan(self, ex, Ntheta_g, rank):
        """grouped SWSH plan over all (component, m) of a rank-`rank` tensor (as SphereBasis.colatitude_plan)"""
        key = ("swsh", id(ex), Ntheta_g, rank)
        store = getattr(self, "_root", self)._plans        # shared by the derivative bases (same angular part)
        if key not in store:
            sb = self.sphere
            groups, keys, fwd, bwd, cache = [], [], [], [], {}
            for i, s in enumerate(self.spin_totals(rank)):
                for ml in range(sb.nml):
                    m = sb.m0 + ml
                    mk = m + 4096 * (s + 8)
                    ne = max(sb.Lmax + 1 - m, 0)
                    row = i * 2 * sb.nml + 2 * ml
                    groups.append((mk if ne > 0 else -1 - m, row, row, 2, m, 1, ne))
                    if ne > 0 and mk not in cache:
                        cache[mk] = sph.swsh_matrices(Ntheta_g, sb.Lmax, m, s)
                        keys.append(mk)
                        fwd.append(cache[mk][0])
                        bwd.append(cache[mk][1])
            store[key] = ex.make_grouped_mmt(Ntheta_g, np.array(groups, dtype=np.int64), keys, fwd, bwd)
        return store[key]

    def regularity_plan(self, ex, rank):
        """Q(ell) tables on the natural (2 m + part, ell) slots.  Built from the reference's ell_maps of the packed
        layout (bounding boxes that overlap: a slot covered by several boxes is recombined by each of them in
        turn, core/basis.py:3595-3626) and gathered to the natural slots, so every mode sees exactly the
        matrix product the reference applies to it."""
        key = ("reg", id(ex), rank)
        store = getattr(self, "_root", self)._plans
        if key not in store:
            sb = self.sphere
            slot_p, fwd, bwd = curvilinear.recombination_tables(sb.packed_ell_rows(), sb.packed_shape(), rank)
            rows, cols, ok = sb.pack_index()
            slot = -np.ones((2 * sb.nm, sb.nl), dtype=np.int32)
            slot[rows[ok], cols[ok]] = slot_p[ok]
            slot = np.ascontiguousarray(slot[2 * sb.m0:2 * (sb.m0 + sb.nml)])
            store[key] = (ex.make_recombination(slot, fwd) if rank > 0 else None,
                          ex.make_recombination(slot, bwd) if rank > 0 else None)
        return store[key]

    def zonal_plans(self, ex, Ntheta_g, rank):
        """The m = 0 rows of colatitude_plan and of the backward regularity_plan, for data [nc][2][nl][Nr_g] (zonal
        means): (grouped SWSH plan, Q(ell) table or None)."""
        key = ("zonal", id(ex), Ntheta_g, rank)
        store = getattr(self, "_root", self)._plans
        if key not in store:
            sb = self.sphere
            groups, keys, fwd, bwd = [], [], [], []
            for i, s in enumerate(self.spin_totals(rank)):
                mk = 4096 * (s + 8)
                groups.append((mk, 2 * i, 2 * i, 2, 0, 1, sb.Lmax + 1))
                if mk not in keys:
                    f, b = sph.swsh_matrices(Ntheta_g, sb.Lmax, 0, s)
                    keys.append(mk)
                    fwd.append(f)
                    bwd.append(b)
            plan = ex.make_grouped_mmt(Ntheta_g, np.array(groups, dtype=np.int64), keys, fwd, bwd)
            table = None
            if rank > 0:
                slot_p, _, bwd_q = curvilinear.recombination_tables(sb.packed_ell_rows(), sb.packed_shape(), rank)
                rows, cols, ok = sb.pack_index()
                slot = -np.ones((2 * sb.nm, sb.nl), dtype=np.int32)
                slot[rows[ok], cols[ok]] = slot_p[ok]
                table = ex.make_recombination(np.ascontiguousarray(slot[0:2]), bwd_q)
            store[key] = (plan, table)
        return store[key]

    def radial_factor(self, ex, scale, power):
        key = ("fac", id(ex), scale, power)
        if key not in self._plans:
            r = self.radius_grid(scale)
            self._plans[key] = ex.from_host(np.ascontiguousarray((self.dR / r) ** power))
        return self._plans[key]


class ShellDistributor:
    def __init__(self, coordsys, comm=None, mesh=None, dtype=None, executor=None):
        self.coordsystems = (coordsys,)
        self.coordsys = coordsys
        self.coords = coordsys.coords
        self.dim = 3
        self.dtype = np.dtype(np.float64 if dtype is None else dtype)
        P = int(np.prod(mesh)) if mesh is not None and len(tuple(mesh)) else 1
        self.mesh, self.size, self.rank, self.comm, self.pcomm = (), 1, 0, comm, None
        if P > 1:
            # one process per GPU on a 1-D mesh: azimuthal wavenumbers block-distributed in coefficient space,
            # colatitudes in grid space (the reference's layouts for a 1-D mesh, core/distributor.py:60-70)
            from ..parallel import Comm
            self.pcomm = Comm(P)
            self.mesh, self.size, self.rank = (P,), P, self.pcomm.rank
        coordsys.dist = self
        coordsys.S2coordsys.dist = self
        self._executor = executor

    def theta_range(self, Nt):
        """(first local colatitude index, number of local colatitudes) of a grid with Nt colatitudes"""
        if Nt % self.size:
            raise ValueError("%d colatitudes do not divide over %d ranks" % (Nt, self.size))
        n = Nt // self.size
        return self.rank * n, n

    @property
    def executor(self):
        if self._executor is None:
            from ..executor import HipExecutor
            self._executor = HipExecutor()       # raises without a gfx950 device: no CPU fallback
        return self._executor

    def Field(self, name=None, bases=None, tensorsig=None, dtype=None):
        if isinstance(bases, (tuple, list)):
            bases = bases[0] if bases else None
        rank = len(tensorsig) if tensorsig else 0
        if bases is None:
            if rank:
                raise NotImplementedError("constant tensor fields in spherical coordinates")
            return ConstField(self, name=name)
        if isinstance(bases, RadialBasis):
            return RadialField(self, bases.shell, rank=rank, name=name)
        if isinstance(bases, MeridionalBasis):
            bases = bases.shell
        if not isinstance(bases, (ShellBasis, SurfaceBasis)):
            raise NotImplementedError("fields in spherical coordinates need a ShellBasis, one of its surfaces or its radial basis")
        return ShellField(self, bases, rank=rank, name=name)

    ScalarField = Field

    def VectorField(self, coordsys, name=None, bases=None, dtype=None):
        return self.Field(name=name, bases=bases, tensorsig=(coordsys,))

    def TensorField(self, coordsys, name=None, bases=None, order=2, dtype=None):
        sig = tuple(coordsys) if isinstance(coordsys, (tuple, list)) else (coordsys,) * order
        return self.Field(name=name, bases=bases, tensorsig=sig)

    def local_grids(self, *bases, scales=None):
        basis = bases[0]
        if scales is None:
            scales = (1, 1, 1)
        elif isinstance(scales, numbers.Number):
            scales = (scales,) * 3
        phi, theta, r = basis.grids(scales)
        t0, nt = self.theta_range(theta.size)
        return phi[:, None, None], theta[None, t0:t0 + nt, None], r[None, None, :]


class RadialBasis:
    def __init__(self, shell):
        self.shell = shell
        self.k = shell.k


class MeridionalBasis:
    """ShellBasis.meridional_basis: fields built on it live on the full shell basis `shell`."""

    def __init__(self, shell):
        self.shell = shell
        self.k = shell.k


class SurfaceBasis:
    """A SphereBasis used by fields of a SphericalCoordinates distributor (shell.outer_surface / inner_surface, tau
    fields): 3^rank spin components (-, +, 0) per (m, ell), one radial point (core/basis.py SphereBasis with a
    SphericalCoordinates coordsys, :2683-2686)."""

    def __init__(self, shell, radius):
        self.shell, self.radius = shell, float(radius)
        self.sphere = shell.sphere
        self.dealias = shell.dealias
        self.Nr = 1
        self.k = 0
        self.coordsys = shell.coordsys

    def grid_shape(self, scales):
        return self.sphere.grid_shape(scales[:2]) + (1,)

    def grids(self, scales):
        phi, theta = self.sphere.grids(scales[:2])
        return phi, theta, np.array([self.radius])

    def colatitude_plan(self, ex, Nt, rank):
        return self.shell.colatitude_plan(ex, Nt, rank)

    def recombination_matrix(self, rank, forward):
        return self.shell.recombination_matrix(rank, forward)

    def __eq__(self, other):
        # the sphere r = R of a shell and of its derivative bases (k + 1, ...) is one basis, as in the reference, whose
        # S2 basis does not know k: radial(grad(A)(r=R)) + SphericalEllProduct(A, ...)(r=R) is a sum on one surface
        root = lambda b: getattr(b.shell, "_root", b.shell)
        return isinstance(other, SurfaceBasis) and root(other) is root(self) and other.radius == self.radius

    def __hash__(self):
        return hash((id(getattr(self.shell, "_root", self.shell)), self.radius))


def _radial_gemm(dist, basis, scale, nc, forward_dir):
    """The radial Jacobi transform of all (component, m, ell) lines as ONE dense GEMM with the (Ng x Ng, zero-padded)
    transform matrix (JacobiMMT, core/transforms.py:114-158) shared by every ell: `ddh_ell_terms_apply` runs it on the
    FP64 MFMA path.  OPT-IN (DDH_RADIAL_GEMM=1 when the radial grid size tiles by 64, =2 always): measured at config
    H it is slower than the LDS FFT kernel (step 13.4 ms against 10.3 ms) -- the per-ell GEMM tiles are mostly empty at
    low ell and the padded copies cost two more passes -- so the FFT path stays the default; the parity tests keep the
    matrix path alive as the independent check of the fast transform (the reference's own fast-vs-matrix test)."""
    import os
    mode = int(os.environ.get("DDH_RADIAL_GEMM", "0"))
    Ng = basis.grid_shape((1.0, 1.0, scale))[2]
    if mode == 0 or dist.size > 1 or Ng < basis.Nr or (mode == 1 and (Ng % 64 != 0 or basis.Nr < 64)):
        return None
    ex = dist.executor
    key = ("rgemm", id(ex), scale, nc, forward_dir)
    if key not in basis._plans:
        sb = basis.sphere
        fwd, bwd = basis.radial.mmt_matrices(Ng)              # (Nr x Ng), (Ng x Nr)
        A = np.zeros((1, Ng, Ng))
        if forward_dir:
            A[0, :basis.Nr, :] = fwd
        else:
            A[0, :, :basis.Nr] = bwd
        live = (np.arange(2 * sb.nml)[:, None] // 2) <= np.arange(sb.nl)[None, :]
        slot_map = np.where(live, 0, -1).astype(np.int32)
        basis._plans[key] = ex.make_ell_terms(sb.nml, sb.nl, Ng, nc, [(c, c, A) for c in range(nc)], slot_map)
    return basis._plans[key]


def backward(dist, basis, rank, c, scales, upto=None):
    """coefficients [nc][2 nml][nl][Nr] (regularity components, local m) -> grid [nc][Nphi_g][Ntheta_g / P][Nr_g]
    (coordinate components, local colatitudes).  On P ranks the only exchange is the all-to-all between "m local
    block, all colatitudes" and "all m, colatitude block" that replaces the reference's (azimuth, colatitude)
    transpose (core/distributor.py:770-924), placed before the azimuthal FFT.
    upto (reduced analysis tasks): "spin" stops at the spin components [nc][2 nml][nl][Nr_g], "azimuth" at the coordinate
    components [nc][2 nm][Ntheta_g / P * Nr_g] in front of the azimuthal FFT (all m local)."""
    ex = dist.executor
    sb = basis.sphere
    nc = 3 ** rank
    nml = sb.nml
    Np, Nt, Ng = basis.grid_shape(scales)
    nslots = nc * 2 * nml * sb.nl
    if isinstance(basis, SurfaceBasis):
        t0 = c                                             # spin components, no radial axis
    else:
        t0 = ex.empty((nc, 2 * nml, sb.nl, Ng))
        gemm = _radial_gemm(dist, basis, scales[2], nc, False)
        if gemm is not None:
            gemm.apply(_padded(ex, c, Ng), t0)
        else:
            ex.transform(basis.radial.plan_spec(scales[2]), basis.radial, "backward", c, t0, nslots, 1)
        ex.regularity_recombine(t0, basis.regularity_plan(ex, rank)[1],
                                basis.radial_factor(ex, scales[2], basis.k) if basis.k > 0 else None)
    if upto == "spin":
        return t0
    t1 = ex.empty((nc, 2 * nml, Nt, Ng))
    basis.colatitude_plan(ex, Nt, rank).backward(t0.reshape(1, nc * 2 * nml, sb.nl, Ng),
                                                 t1.reshape(1, nc * 2 * nml, Nt, Ng))
    if rank > 0:
        t2 = ex.empty((nc, 2 * nml, Nt * Ng))
        ex.spin_recombine(t1.reshape(nc, 2 * nml, Nt * Ng), t2, basis.recombination_matrix(rank, forward=False))
    else:
        t2 = t1
    P = dist.size
    Ntl = Nt
    if P > 1:
        # [nc][2 nml][Nt][Ng] -> [nc][2 nm][Nt / P][Ng]
        Ntl = dist.theta_range(Nt)[1]
        n_el = nc * 2 * nml * Nt * Ng
        send, recv = ex.empty((n_el,)), ex.empty((n_el,))
        ex.a2a_pack(t2, send, nc * 2 * nml, Nt, 1, Ng, P)
        dist.pcomm.all_to_all(recv, send)
        t2 = ex.empty((nc, 2 * sb.nm, Ntl * Ng))
        ex.a2a_unpack(recv, t2, nc, 1, 2 * nml * P, Ntl * Ng, P)
    if upto == "azimuth":
        return t2
    g = ex.empty((nc, Np, Ntl, Ng))
    ex.transform(("rfft", Np, sb.Nphi), None, "backward", t2, g, nc, Ntl * Ng)
    return g


def forward(dist, basis, rank, g, scales, upto=None):
    """the mirror of backward; upto "azimuth" / "spin" stop at the same two stages"""
    ex = dist.executor
    sb = basis.sphere
    nc = 3 ** rank
    nml = sb.nml
    Np, Nt, Ng = basis.grid_shape(scales)
    P = dist.size
    Ntl = dist.theta_range(Nt)[1] if P > 1 else Nt
    t1 = ex.empty((nc, 2 * sb.nm, Ntl * Ng))
    ex.transform(("rfft", Np, sb.Nphi), None, "forward", g, t1, nc, Ntl * Ng)
    if upto == "azimuth":
        return t1
    if P > 1:
        # [nc][2 nm][Nt / P][Ng] -> [nc][2 nml][Nt][Ng]
        n_el = nc * 2 * sb.nm * Ntl * Ng
        send, recv = ex.empty((n_el,)), ex.empty((n_el,))
        ex.a2a_pack(t1, send, nc, 2 * sb.nm, Ntl, Ng, P)
        dist.pcomm.all_to_all(recv, send)
        t1 = ex.empty((nc, 2 * nml, Nt * Ng))
        ex.a2a_unpack(recv, t1, nc, 2 * nml, Ntl * P, Ng, P)
    if rank > 0:
        t2 = ex.empty((nc, 2 * nml, Nt * Ng))
        ex.spin_recombine(t1, t2, basis.recombination_matrix(rank, forward=True))
    else:
        t2 = t1
    t3 = ex.zeros((nc, 2 * nml, sb.nl, Ng))
    basis.colatitude_plan(ex, Nt, rank).forward(t2.reshape(1, nc * 2 * nml, Nt, Ng),
                                                t3.reshape(1, nc * 2 * nml, sb.nl, Ng))
    if isinstance(basis, SurfaceBasis) or upto == "spin":
        return t3
    ex.regularity_recombine(t3, basis.regularity_plan(ex, rank)[0],
                            basis.radial_factor(ex, scales[2], -basis.k) if basis.k > 0 else None)
    gemm = _radial_gemm(dist, basis, scales[2], nc, True)
    if gemm is not None:
        full = ex.empty((nc, 2 * nml, sb.nl, Ng))
        gemm.apply(t3, full)
        return _unpadded(ex, full, basis.Nr)
    c = ex.empty((nc, 2 * nml, sb.nl, basis.Nr))
    ex.transform(basis.radial.plan_spec(scales[2]), basis.radial, "forward", t3, c, nc * 2 * nml * sb.nl, 1)
    return c



# ==================================================================================================
# ell-dependent radial term lists and operands
# ==================================================================================================

class EllTermList:
    """Linear map between shell coefficient arrays: out[co][i1][ell][:] = sum A[ell] in[ci][i1][ell][:], matrices
    stored as [nl][Nr][Nr] (sphere-surface operands use the leading 1 x Nr / Nr x 1 / 1 x 1 block).
    rot (optional, one 0 / 1 per term): a term with rot = 1 is i A on the complex number cos + i msin of every azimuthal
    mode, i.e. out[2m] += -A in[2m + 1], out[2m + 1] += +A in[2m] (the curl); i . i = -1 when two
    such terms are composed."""

    def __init__(self, nco, nci, terms=None, rot=None):
        self.nco, self.nci = nco, nci
        self.terms = list(terms or [])          # (co, ci, mats [nl][Nr][Nr])
        self.rot = [int(r) for r in rot] if rot is not None else [0] * len(self.terms)
        assert len(self.rot) == len(self.terms)

    @property
    def rotated(self):
        return any(self.rot)

    @staticmethod
    def identity(nc, nl, Nr, nr):
        m = np.zeros((nl, Nr, Nr))
        m[:, np.arange(nr), np.arange(nr)] = 1.0
        return EllTermList(nc, nc, [(c, c, m.copy()) for c in range(nc)])

    def scaled(self, a):
        return EllTermList(self.nco, self.nci, [(co, ci, a * m) for (co, ci, m) in self.terms], self.rot)

    def __add__(self, other):
        assert (self.nco, self.nci) == (other.nco, other.nci)
        return EllTermList(self.nco, self.nci, self.terms + other.terms, self.rot + other.rot).merged()

    def merged(self):
        acc = {}
        for (co, ci, m), r in zip(self.terms, self.rot):
            acc[(co, ci, r)] = acc[(co, ci, r)] + m if (co, ci, r) in acc else np.array(m, dtype=np.float64)
        keep = [(key, m) for key, m in sorted(acc.items()) if np.any(m != 0)]
        return EllTermList(self.nco, self.nci, [(co, ci, m) for (co, ci, r), m in keep], [r for (co, ci, r), m in keep])

    def compose(self, inner):
        assert self.nci == inner.nco
        if isinstance(inner, EllMixList):                  # matrix-list o mix: the columns of A[ell] scaled by q[ell]
            out = [(co, ci, A * q[:, None, None]) for (co, cm, A) in self.terms for (cm2, ci, q) in inner.terms if cm2 == cm]
            rot = [ra for (co, cm, A), ra in zip(self.terms, self.rot) for (cm2, ci, q) in inner.terms if cm2 == cm]
            return EllTermList(self.nco, inner.nci, out, rot).merged()
        out, rot = [], []
        for (co, cm, A), ra in zip(self.terms, self.rot):
            for (cm2, ci, B), rb in zip(inner.terms, inner.rot):
                if cm2 == cm:
                    out.append((co, ci, -np.matmul(A, B) if (ra and rb) else np.matmul(A, B)))
                    rot.append(ra ^ rb)
        return EllTermList(self.nco, inner.nci, out, rot).merged()

    def embed(self, row0, col0, nrows, ncols):
        return EllTermList(nrows, ncols, [(co + row0, ci + col0, m) for (co, ci, m) in self.terms], self.rot)


class EllMixList:
    """Linear map between shell coefficient arrays that is the identity along n: out[co][i1][ell][:] = sum q[ell] in[ci][i1][ell][:],
    one real scalar per term and ell (transpose, radial and angular components: DESIGN.md section 9).  Composes with itself
    and, in both orders, with EllTermList, where it scales the radial matrices per ell."""

    def __init__(self, nco, nci, terms=None):
        self.nco, self.nci = nco, nci
        self.terms = [(int(co), int(ci), np.asarray(q, dtype=np.float64)) for (co, ci, q) in (terms or [])]

    rotated = False

    @staticmethod
    def from_matrices(mats):
        """mats [nl][nco][nci] -> the list of its non-zero (co, ci) entries"""
        mats = np.asarray(mats, dtype=np.float64)
        nco, nci = mats.shape[1:]
        return EllMixList(nco, nci, [(co, ci, mats[:, co, ci].copy()) for co in range(nco) for ci in range(nci)
                                     if np.any(mats[:, co, ci] != 0)])

    def matrices(self, nl):
        out = np.zeros((nl, self.nco, self.nci))
        for (co, ci, q) in self.terms:
            out[:, co, ci] += q
        return out

    def scaled(self, a):
        return EllMixList(self.nco, self.nci, [(co, ci, a * q) for (co, ci, q) in self.terms])

    def merged(self):
        acc = {}
        for (co, ci, q) in self.terms:
            acc[(co, ci)] = acc[(co, ci)] + q if (co, ci) in acc else np.array(q, dtype=np.float64)
        return EllMixList(self.nco, self.nci, [(co, ci, q) for (co, ci), q in sorted(acc.items()) if np.any(q != 0)])

    def __add__(self, other):
        assert isinstance(other, EllMixList) and (self.nco, self.nci) == (other.nco, other.nci)
        return EllMixList(self.nco, self.nci, self.terms + other.terms).merged()

    def compose(self, inner):
        assert self.nci == inner.nco
        if isinstance(inner, EllMixList):
            return EllMixList(self.nco, inner.nci, [(co, ci, qa * qb) for (co, cm, qa) in self.terms
                                                    for (cm2, ci, qb) in inner.terms if cm2 == cm]).merged()
        out, rot = [], []                                  # mix o matrix-list: the rows of B[ell] scaled by q[ell]
        for (co, cm, q) in self.terms:
            for (cm2, ci, B), rb in zip(inner.terms, inner.rot):
                if cm2 == cm:
                    out.append((co, ci, q[:, None, None] * B))
                    rot.append(rb)
        return EllTermList(self.nco, inner.nci, out, rot).merged()

    def as_termlist(self, Nr, nr=None):
        """the same map as radial matrices q[ell] * identity (leading nr x nr block)"""
        nl = len(self.terms[0][2]) if self.terms else 1
        return self.compose(EllTermList.identity(self.nci, nl, Nr, Nr if nr is None else nr))


REG = (-1, +1, 0)


def reg_indices(rank):
    return list(np.ndindex(*((3,) * rank)))


def regtotal(idx):
    return sum(REG[a] for a in idx)


def regularity_allowed(ell, idx):
    """RegularityBasis.regularity_allowed (core/basis.py:3531-3535, vectorised form :3585-3593)."""
    walk = ell
    for a in idx[::-1]:
        dr = REG[a]
        walk = walk + dr
        if walk < 0 or (dr == 0 and walk == 0):
            return False
    return True


def spin_allowed(ell, idx):
    return ell >= abs(sum(REG[a] for a in idx))


def shell_op_termlist(kind, shell, rank_in, k, **kw):
    """Term list of one operator of the reference's SphericalEllOperator family acting on a rank-`rank_in` tensor
    in the k-th shell basis: lap (core/operators.py:4109-4152), grad (:3240-3288), div (:3546-3600), curl (:3838-3901), convert
    (ConvertSpherical3D, core/basis.py:4822-4842), lift (LiftShell :5155-5199), interp (ShellRadialInterpolate
    :5823-5889)."""
    from ..tools import shellops as so
    sb = shell.sphere
    nl, Nr, radii, alpha = sb.nl, shell.Nr, shell.radii, shell.alpha
    idx_in = reg_indices(rank_in)

    def stack(fn, allow_in, allow_out):
        m = np.zeros((nl, Nr, Nr))
        for ell in range(nl):
            if allow_in(ell) and allow_out(ell):
                a = np.asarray(fn(ell))
                m[ell, :a.shape[0], :a.shape[1]] = a
        return m

    terms = []
    if kind == "lap":
        for ci, t in enumerate(idx_in):
            rt = regtotal(t)
            terms.append((ci, ci, stack(lambda ell: so.operator_matrix("L", ell, rt, Nr, k, radii, alpha),
                                        lambda ell: regularity_allowed(ell, t), lambda ell: True)))
        return EllTermList(len(idx_in), len(idx_in), terms)
    if kind == "convert":
        dk = kw["dk"]
        E = so.E_power(Nr, k, dk, radii, alpha)
        for ci, t in enumerate(idx_in):
            terms.append((ci, ci, stack(lambda ell: E, lambda ell: regularity_allowed(ell, t), lambda ell: True)))
        return EllTermList(len(idx_in), len(idx_in), terms)
    if kind == "grad":
        idx_out = reg_indices(rank_in + 1)
        for ci, t in enumerate(idx_in):
            rt = regtotal(t)
            for a, (mu, name) in enumerate(((-1, "D-"), (+1, "D+"))):
                to = (a,) + tuple(t)
                co = idx_out.index(to)
                terms.append((co, ci, stack(lambda ell: so.xi(mu, ell + rt) * so.operator_matrix(name, ell, rt, Nr, k, radii, alpha),
                                            lambda ell: regularity_allowed(ell, t), lambda ell: regularity_allowed(ell, to))))
        return EllTermList(len(idx_out), len(idx_in), terms)
    if kind == "div":
        idx_out = reg_indices(rank_in - 1)
        for ci, t in enumerate(idx_in):
            if t[0] == 2:
                continue
            rt = regtotal(t)
            to = tuple(t[1:])
            co = idx_out.index(to)
            if t[0] == 0:
                fn = lambda ell: so.xi(-1, ell + rt + 1) * so.operator_matrix("D+", ell, rt, Nr, k, radii, alpha)
            else:
                fn = lambda ell: so.xi(+1, ell + rt - 1) * so.operator_matrix("D-", ell, rt, Nr, k, radii, alpha)
            terms.append((co, ci, stack(fn, lambda ell: regularity_allowed(ell, t), lambda ell: regularity_allowed(ell, to))))
        return EllTermList(len(idx_out), len(idx_in), terms)
    if kind == "curl":
        # SphericalCurl (core/operators.py:3838-3901): purely imaginary radial matrices between the regularity components
        # (-, +) <-> 0 -- stored as the real factor with rot = 1.  The sign of the factor and the blocks are those of
        # _radial_matrix (:3889-3901); regindex_out (:3870-3877).
        if rank_in != 1:
            raise NotImplementedError("curl of a rank-%d tensor" % rank_in)
        blocks = ((0, 2, -1.0, +1, +1, "D+"), (1, 2, +1.0, -1, -1, "D-"),       # (in, out, sign, xi mu, xi shift, D)
                  (2, 0, -1.0, +1, 0, "D-"), (2, 1, +1.0, -1, 0, "D+"))
        for (ci, co, sign, mu, shift, name) in blocks:
            rt = REG[ci]
            terms.append((co, ci, stack(lambda ell: sign * so.xi(mu, ell + rt + shift) * so.operator_matrix(name, ell, rt, Nr, k, radii, alpha),
                                        lambda ell: regularity_allowed(ell, (ci,)), lambda ell: regularity_allowed(ell, (co,)))))
        return EllTermList(3, 3, terms, [1] * len(terms)).merged()
    if kind == "trace":              # SphericalTrace (core/operators.py:1783-1826): Q_out^T trace_spin Q_in, identity in n
        if rank_in != 2:
            raise NotImplementedError("trace of a rank-%d tensor" % rank_in)
        tr = np.zeros(9)
        tr[[1, 3, 8]] = 1.0
        for ci, t in enumerate(idx_in):
            def fn(ell, ci=ci):
                return float(tr @ sph.intertwiner(ell, 2)[:, ci]) * np.eye(Nr)
            m = stack(fn, lambda ell: regularity_allowed(ell, t), lambda ell: True)
            if np.any(m != 0):
                terms.append((0, ci, m))
        return EllTermList(1, len(idx_in), terms)
    if kind == "integ":              # IntegrateShell (core/basis.py:5555-5575): ell = 0 only -> a constant
        from ..tools import jacobi
        z0, w0 = jacobi.quadrature(2 * Nr, 0, 0)
        z0, w0 = np.asarray(z0, dtype=np.float64), np.asarray(w0, dtype=np.float64)
        dR = radii[1] - radii[0]
        r0 = dR / 2 * (z0 + (radii[1] + radii[0]) / dR)
        Qk = np.asarray(jacobi.polynomials(Nr, alpha[0] + k, alpha[1] + k, z0))
        row = (r0 ** 2 * w0 * (r0 / dR) ** (-k)) @ Qk.T * (dR / 2) * (4 * np.pi / np.sqrt(2))
        m = np.zeros((nl, Nr, Nr))
        m[0, 0, :] = row
        return EllTermList(1, 1, [(0, 0, m)])
    if kind == "convert_const":      # ConvertConstantShell (core/basis.py:4782-4819): constant -> ell = 0, k-th basis
        from ..tools import jacobi
        cmv = float(np.asarray(jacobi.polynomials(1, alpha[0], alpha[1], np.array([0.0])))[0, 0]) / np.sqrt(2)
        col = so.E_power(Nr, 0, k, radii, alpha)[:, 0] / cmv
        m = np.zeros((nl, Nr, Nr))
        m[0, :, 0] = col
        return EllTermList(1, 1, [(0, 0, m)])
    if kind == "lift":               # sphere-surface spin components -> regularity components, radial mode n
        n = kw["n"]
        n_idx = n if n >= 0 else Nr + n
        for co, to in enumerate(idx_in):
            for ci, ti in enumerate(idx_in):
                def fn(ell):
                    q = sph.intertwiner(ell, rank_in)[ci, co] if rank_in else 1.0      # Q^T[co, ci]
                    a = np.zeros((Nr, 1))
                    a[n_idx, 0] = q
                    return a
                m = stack(fn, lambda ell: spin_allowed(ell, ti), lambda ell: regularity_allowed(ell, to))
                if np.any(m != 0):
                    terms.append((co, ci, m))
        return EllTermList(len(idx_in), len(idx_in), terms)
    if kind == "interp":             # regularity components -> spin components on the sphere r = position
        vec = so.interpolation(kw["position"], Nr, k, radii, alpha)
        for co, to in enumerate(idx_in):
            for ci, ti in enumerate(idx_in):
                def fn(ell):
                    q = sph.intertwiner(ell, rank_in)[co, ci] if rank_in else 1.0      # Q[co, ci]
                    return q * vec.reshape(1, Nr)
                m = stack(fn, lambda ell: regularity_allowed(ell, ti), lambda ell: spin_allowed(ell, to))
                if np.any(m != 0):
                    terms.append((co, ci, m))
        return EllTermList(len(idx_in), len(idx_in), terms)
    raise ValueError(kind)


def operate_slot_sequences(sb):
    """(extra sequences, slot map [2 nm][nl]) for operator EVALUATION: matrix index ell for a slot covered by its own
    ell_maps box only, nl + j for a slot covered by the boxes listed in seqs[j]; -1 where there is no mode."""
    key = "operate_slots"
    if key not in sb._plans:
        rows_p = sb.packed_ell_rows()
        ps = sb.packed_shape()
        cover = [[[] for _ in range(ps[1])] for _ in range(ps[0])]
        for (ell, i0, i1, j0, j1) in rows_p:
            for i in range(i0, i1):
                for j in range(j0, j1):
                    cover[i][j].append(int(ell))
        rows, cols, ok = sb.pack_index()
        slot = -np.ones((2 * sb.nm, sb.nl), dtype=np.int32)
        seqs, index = [], {}
        for i in range(ps[0]):
            for j in range(ps[1]):
                if not ok[i, j]:
                    continue
                r, l = int(rows[i, j]), int(cols[i, j])
                seq = tuple(cover[i][j])
                if seq == (l,):
                    slot[r, l] = l
                else:
                    if seq not in index:
                        index[seq] = len(seqs)
                        seqs.append(seq)
                    slot[r, l] = sb.nl + index[seq]
        sb._plans[key] = (seqs, slot)
    return sb._plans[key]


class ShOperand(CurviOperand):
    """Expression node in spherical coordinates (the algebra: core/curvioperand.py).  basis: ShellBasis (k), SurfaceBasis
    or None."""

    def __array_ufunc__(self, ufunc, method, *inputs, **kw):
        """numpy scalars and ufuncs applied to operands (np.sqrt(u@u), np.float64(2) * u, ...)"""
        if method != "__call__" or kw:
            return NotImplemented
        if len(inputs) == 1:
            return ShUnary(ufunc, inputs[0])
        a, b = inputs
        if ufunc is np.multiply:
            return a * b if isinstance(a, ShOperand) else b * a
        if ufunc is np.add:
            return a + b if isinstance(a, ShOperand) else b + a
        if ufunc is np.subtract:
            return a - b if isinstance(a, ShOperand) else (-1 * b) + a
        if ufunc is np.true_divide and isinstance(b, numbers.Number):
            return a * (1.0 / b)
        if ufunc is np.matmul:
            return ShProduct(a, b, contract=True)
        return NotImplemented

    @property
    def sig(self):
        """components per tensor index: 3 (phi, theta, r / -, +, 0), or 2 for an S2 index (-, +), which angular() makes"""
        return getattr(self, "_sig", None) or (3,) * self.rank

    @property
    def ncomp(self):
        return int(np.prod(self.sig, dtype=np.int64))

    @staticmethod
    def dot(a, b):
        return ShProduct(a, b, contract=True)

    def eval_g(self):
        return _eval_grid(self)

    def __call__(self, **kw):
        """T(r=Ri): interpolation along the radius (core/operators.py interpolate dispatch)."""
        if len(kw) != 1:
            raise ValueError("one coordinate at a time")
        (name, pos), = kw.items()
        if name == self.dist.coordsys.coords[0].name:
            return ShAzimuthalInterp(self, float(pos))
        if name == self.dist.coordsys.colatitude.name:
            return ShColatitudeInterp(self, float(pos))
        if name != self.dist.coordsys.radius.name:
            return ShUnsupported("interpolation along %r" % name, self)
        return ShLinear("interp", self, position=float(pos))

    def cfl_term(self, velocity):
        """(term, own grid shape, function giving the device grid data) of this operand in the fused CFL reduction
        (HipExecutor.cfl_sum_max): a vector on a shell basis as a velocity (Spherical3DAdvectiveCFL, core/basis.py:
        6183-6204), a scalar as a frequency, both at the dealias scales."""
        shell = self.basis
        if not isinstance(shell, ShellBasis):
            raise NotImplementedError("CFL frequencies of operands without a shell basis")
        if velocity:
            if tuple(self.sig) != (3,):
                raise ValueError("CFL velocity must be a vector field on a shell")
            term = dict(kind="shell", inv=_cfl_spacings(shell, self.dist.executor))
        else:
            if self.rank != 0:
                raise ValueError("Frequency must be a scalar")
            term = dict(kind="scalar")
        Np, Nt, Ng = shell.grid_shape(shell.dealias)
        return term, (int(Np), int(self.dist.theta_range(Nt)[1]), int(Ng)), self.eval_g

    def grid_native(self):
        """Grid data when the operand is formed in grid space (products), else None."""
        return None

    def is_grid_native(self):
        """True when grid_native() gives data (asked before evaluating anything)"""
        return False

    def _result_field(self):
        return ShellField(self.dist, self.basis, rank=self.rank, sig=self.sig)


def _no_s2_index(what, *args):
    for a in args:
        if isinstance(a, ShOperand) and any(d != 3 for d in a.sig):
            raise NotImplementedError("%s of an operand with an S2 index (%r)" % (what, a))


class ShReduced(sphreduce.ReducedResult, ShOperand):
    """Reduced analysis tasks of shell operands (core/sphreduce.py): contractions of the stages backward() / forward()
    produce, on the device; ['g'] downloads the reduced result only."""

    dim = 3
    from_grid = False

    def __init__(self, arg, **params):
        if not isinstance(arg, ShOperand) or isinstance(arg, (RadialField, ConstField)) or arg.basis is None:
            raise NotImplementedError("%s of an operand without an angular basis" % self.what)
        _no_s2_index(self.what, arg)
        if isinstance(arg, ShLinear) and arg.kind in ("interp", "integ"):
            raise sphreduce.reduction_refused(self.what, arg.kind)
        self._init(arg, **params)

    @property
    def field_type(self):
        return ShellField

    def _native_grid(self, arg):
        return arg.grid_native()

    def _field_from_grid(self, g):
        f = ShellField(self.dist, self.basis, rank=self.rank)
        f._set_device_coeff(forward(self.dist, self.basis, self.rank, g, self.basis.dealias))
        return f

    def _tensor_shape(self):
        return (3,) * self.rank

    def _store(self):
        b = self.basis.shell if isinstance(self.basis, SurfaceBasis) else self.basis
        return getattr(b, "_root", b)._plans

    def _single_rank(self):
        if self.dist.size > 1:
            raise NotImplementedError("%s on several ranks: the azimuthal wavenumbers are distributed where it is formed"
                                      % self.what)


class ShAzimuthalInterp(ShReduced):
    """f(phi=phi0) (InterpolateAzimuth, core/basis.py:5578-5634): the coordinate components in front of the azimuthal FFT,
    [nc][2 nm][colatitudes * radii] with all m local (on several ranks: after the m <-> theta exchange), contracted with
    cos m phi0, -sin m phi0 in one ddh_axis_contract launch.  The result keeps a phi axis of size one."""

    what = "azimuthal interpolation"
    const_axes = (0,)
    from_grid = True

    def __init__(self, arg, position):
        ShReduced.__init__(self, arg, position=float(position))
        self.position = float(position)

    def _init(self, arg, **params):
        ShReduced._init(self, arg, **params)
        self.position = params["position"]

    def _device(self, scales):
        ex, sb = self.dist.executor, self.basis.sphere
        nc = self.ncomp
        if self._grid is not None and scales == tuple(self.basis.dealias):
            t = forward(self.dist, self.basis, self.rank, self._grid, scales, upto="azimuth")
        else:
            t = backward(self.dist, self.basis, self.rank, self._coeff_field().require_coeff_space(), scales, upto="azimuth")
        Np, Nt, Ng = self.basis.grid_shape(scales)
        Ntl = self.dist.theta_range(Nt)[1]
        out = sphreduce.contract(ex, self._store(), t, nc, 2 * sb.nm, Ntl * Ng, sphreduce.azimuth_weights(sb.nm, self.position))
        return out.reshape(nc, 1, Ntl, Ng)


class ShColatitudeInterp(ShReduced):
    """f(theta=theta0) (InterpolateColatitude, core/basis.py:5637-5736): the spin components [nc][2 nml][nl][Nr_g]
    contracted along ell with Y_l^{m,s}(theta0) (ddh_axis_contract_rows: one weight row per (spin weight, m), read from
    l = max(m, |s|) on), then the spin recombination and the azimuthal FFT of backward() on [nc][2 nm][Nr_g]."""

    what = "colatitude interpolation"
    const_axes = (1,)
    from_grid = True

    def __init__(self, arg, position):
        ShReduced.__init__(self, arg, position=float(position))

    def _init(self, arg, **params):
        ShReduced._init(self, arg, **params)
        self.position = params["position"]

    def _device(self, scales):
        self._single_rank()
        ex, basis, rank = self.dist.executor, self.basis, self.rank
        sb = basis.sphere
        nc, nml = self.ncomp, sb.nml
        if self._grid is not None and scales == tuple(basis.dealias):
            t0 = forward(self.dist, basis, rank, self._grid, scales, upto="spin")
        else:
            t0 = backward(self.dist, basis, rank, self._coeff_field().require_coeff_space(), scales, upto="spin")
        Np, Nt, Ng = basis.grid_shape(scales)
        t1 = sphreduce.contract_rows(ex, self._store(), ("theta", rank, self.position), t0, nc * 2 * nml, sb.nl, Ng,
                                     lambda: sphreduce.colatitude_rows(sb, basis.spin_totals(rank), sb.m0, nml, self.position))
        t1 = t1.reshape(nc, 2 * nml, Ng)
        if rank > 0:
            t2 = ex.empty((nc, 2 * nml, Ng))
            ex.spin_recombine(t1, t2, basis.recombination_matrix(rank, forward=False))
        else:
            t2 = t1
        g = ex.empty((nc, Np, 1, Ng))
        ex.transform(("rfft", Np, sb.Nphi), None, "backward", t2, g, nc, Ng)
        return g


class ShAzimuthalAverage(ShReduced):
    """ave(f, phi) (SphericalAzimuthalAverage, core/basis.py:5267-5293: the m = 0 coefficients): the m = 0 slab of the
    coefficient data, gathered by pointer and stride, through the radial and colatitude backward transforms and the spin
    recombination on its own; no FFT."""

    what = "zonal mean"
    const_axes = (0,)

    def __init__(self, arg):
        ShReduced.__init__(self, arg)

    def _device(self, scales):
        self._single_rank()
        ex, basis, rank, store = self.dist.executor, self.basis, self.rank, self._store()
        sb = basis.sphere
        nc, nl, Nr = self.ncomp, sb.nl, basis.Nr
        Np, Nt, Ng = basis.grid_shape(scales)
        one = np.ones((1, 1))
        c = self._coeff_field().require_coeff_space()
        c0 = sphreduce.contract(ex, store, c, nc, 1, 2 * nl * Nr, one, ostride=sb.nml * 2 * nl * Nr).reshape(nc, 2, nl, Nr)
        plan, table = basis.zonal_plans(ex, Nt, rank)
        if isinstance(basis, SurfaceBasis):
            t0 = c0
        else:
            t0 = ex.empty((nc, 2, nl, Ng))
            ex.transform(basis.radial.plan_spec(scales[2]), basis.radial, "backward", c0, t0, nc * 2 * nl, 1)
            ex.regularity_recombine(t0, table, basis.radial_factor(ex, scales[2], basis.k) if basis.k > 0 else None)
        t1 = ex.empty((nc, 2, Nt, Ng))
        plan.backward(t0.reshape(1, nc * 2, nl, Ng), t1.reshape(1, nc * 2, Nt, Ng))
        if rank > 0:
            t2 = ex.empty((nc, 2, Nt * Ng))
            ex.spin_recombine(t1.reshape(nc, 2, Nt * Ng), t2, basis.recombination_matrix(rank, forward=False))
        else:
            t2 = t1
        out = sphreduce.contract(ex, store, t2, nc, 1, Nt * Ng, one, ostride=2 * Nt * Ng)     # the cos part of m = 0
        return out.reshape(nc, 1, Nt, Ng)


class ShSphereAverage(ShReduced):
    """ave(f, S2) of a scalar (SphericalAverage, core/basis.py:5321-5350: the ell = 0 coefficients): the (m, ell) = (0, 0)
    line of the coefficient data through the radial backward transform, times Y_00 -- a radial profile."""

    what = "shell average"
    const_axes = (0, 1)

    def __init__(self, arg):
        if getattr(arg, "rank", 0):
            raise NotImplementedError("shell average of a tensor")
        ShReduced.__init__(self, arg)
        if not isinstance(self.basis, ShellBasis):
            raise NotImplementedError("shell average of an operand without a shell basis")

    def _device(self, scales):
        self._single_rank()
        ex, basis = self.dist.executor, self.basis
        Ng = basis.grid_shape(scales)[2]
        c = self._coeff_field().require_coeff_space()
        line = ex.empty((1, 1, 1, basis.Nr))
        ex.assign(line, c[0:1, 0:1, 0:1, :])
        t0 = ex.empty((1, 1, 1, Ng))
        ex.transform(basis.radial.plan_spec(scales[2]), basis.radial, "backward", line, t0, 1, 1)
        if basis.k > 0:
            ex.regularity_recombine(t0, None, basis.radial_factor(ex, scales[2], basis.k))
        out = ex.empty((1, 1, 1, Ng))
        ex.lincomb(out, [t0], [float(sph.harmonics(0, 0, 0, 0.0)[0, 0])])
        return out


class ShUnsupported(ShOperand):
    """Placeholder for expressions that scripts build for output tasks but that nothing evaluates here."""

    def __init__(self, what, arg):
        self.what, self.args = what, (arg,)
        self.dist, self.basis, self.rank = arg.dist, arg.basis, arg.rank

    def eval_c(self):
        raise NotImplementedError(self.what)

    def lin(self, variables):
        raise NonlinearError(self.what)


class ShUnary(ShOperand):
    """ufunc(operand) point by point on the dealiased grid (UnaryGridFunction, core/operators.py:505-566): one map
    kernel on the operand's device grid (ddh_grid_map)."""

    def __init__(self, func, arg):
        if arg.rank:
            raise NotImplementedError("ufuncs of tensor fields")
        self.func, self.args = func, (arg,)
        self.dist, self.basis, self.rank = arg.dist, arg.basis, 0

    def grid_native(self):
        ex = self.dist.executor
        g = self.args[0].eval_g()
        if getattr(ex, "grid_map", None) is None:               # the NumPy oracle of the tests: through the host
            return ex.from_host(np.ascontiguousarray(self.func(np.asarray(ex.download(g)))))
        from .evaluator import Evaluator
        g = g if g.is_contiguous() else g.contiguous()
        out = ex.empty(tuple(g.shape))
        ex.grid_map(out, g, Evaluator._map_op(self.func))
        return out

    def is_grid_native(self):
        return True

    def eval_g(self):
        return self.grid_native()

    def eval_c(self):
        return forward(self.dist, self.basis, 0, self.grid_native(), self.basis.dealias)

    def lin(self, variables):
        raise NonlinearError("grid functions are nonlinear")


class ShScale(Scale, ShOperand):
    def __init__(self, a, arg):
        Scale.__init__(self, a, arg)
        self._sig = arg.sig

    def is_grid_native(self):
        return self.arg.is_grid_native()

    def grid_native(self):
        g = self.arg.grid_native()
        if g is None:
            return None
        ex = self.dist.executor
        out = ex.empty(tuple(g.shape))
        ex.lincomb(out, [g], [self.a])
        return out


def _common_basis(a, b):
    """Sum basis: shells of the same geometry meet in the larger k (core/basis.py ShellBasis.__add__ :4415-4424)."""
    if isinstance(a.basis, ShellBasis) and isinstance(b.basis, ShellBasis):
        return a.basis if a.basis.k >= b.basis.k else b.basis
    if a.basis is None and isinstance(b.basis, ShellBasis):
        return b.basis
    if b.basis is None and isinstance(a.basis, ShellBasis):
        return a.basis
    if a.basis == b.basis:
        return a.basis
    raise NotImplementedError("sum of operands on different bases")


def _converted(x, basis):
    if isinstance(basis, ShellBasis) and x.basis is None:
        return ShLinear("convert_const", x, basis=basis)
    if isinstance(basis, ShellBasis) and x.basis.k != basis.k:
        return ShLinear("convert", x, dk=basis.k - x.basis.k)
    return x


class ShAdd(Add, ShOperand):
    geometry = "shell"

    def __init__(self, a, b):
        Add.__init__(self, a, b)
        if a.sig != b.sig:
            raise ValueError("cannot add tensors of different signature: components per index %s and %s" % (a.sig, b.sig))
        self._sig = a.sig
        self.basis = _common_basis(a, b)
        self.args = (_converted(a, self.basis), _converted(b, self.basis))

    def is_grid_native(self):
        return isinstance(self.basis, ShellBasis) and all(x.is_grid_native() for x in self.args)

    def grid_native(self):
        """AddFields.operate adds in the layout its arguments share (core/arithmetic.py:226-251): two operands formed on the
        grid (products, e.g. - u@grad(u) - cross(ez, u)/Ekman) are added THERE, and the sum is transformed once, in the
        basis it ends up in."""
        if not self.is_grid_native():
            return None
        ex = self.dist.executor
        gs = [x.grid_native() for x in self.args]
        out = ex.empty(tuple(gs[0].shape))
        ex.lincomb(out, gs, [1.0, 1.0])
        return out

    def eval_c(self):
        ex = self.dist.executor
        if self.is_grid_native():
            return forward(self.dist, self.basis, self.rank, self.grid_native(), self.basis.dealias)
        cs = [x.eval_c() for x in self.args]
        out = ex.empty(tuple(cs[0].shape))
        ex.lincomb(out, cs, [1.0, 1.0])
        return out

    def eval_g(self):
        return self.grid_native() if self.is_grid_native() else _eval_grid(self)


class ShLinear(ShOperand):
    """lap / grad / div / curl / convert / lift / interp of an operand."""

    def __init__(self, kind, arg, **kw):
        if not isinstance(arg, ShOperand):
            raise ValueError("%s needs a field operand" % kind)
        _no_s2_index(kind, arg)
        self.kind, self.arg, self.args, self.kw = kind, arg, (arg,), kw
        self.dist = arg.dist
        ab = arg.basis
        if kind == "curl":
            if isinstance(arg, RadialField):
                raise NotImplementedError("curl of a radial operand")
            if isinstance(ab, SurfaceBasis):
                raise NotImplementedError("curl of a surface operand")
            if arg.rank != 1:
                raise NotImplementedError("curl of a scalar" if arg.rank == 0 else "curl of a rank-%d tensor" % arg.rank)
        if kind in ("lap", "grad", "div", "curl", "convert", "interp", "trace", "integ") and not isinstance(ab, ShellBasis):
            raise NotImplementedError("%s of an operand without a shell basis" % kind)
        if kind == "lap":
            self.basis, self.rank = ab.derivative_basis(2), arg.rank
        elif kind == "grad":
            self.basis, self.rank = ab.derivative_basis(1), arg.rank + 1
        elif kind == "div":
            if arg.rank < 1:
                raise ValueError("div needs a tensor of rank >= 1")
            self.basis, self.rank = ab.derivative_basis(1), arg.rank - 1
        elif kind == "curl":
            self.basis, self.rank = ab.derivative_basis(1), 1
        elif kind == "convert":
            self.basis, self.rank = ab.derivative_basis(kw["dk"]), arg.rank
        elif kind == "interp":
            self.basis, self.rank = ab.S2_basis(kw["position"]), arg.rank
        elif kind == "trace":
            self.basis, self.rank = ab, arg.rank - 2
        elif kind == "integ":
            if arg.rank:
                raise NotImplementedError("integ of a tensor")
            self.basis, self.rank = None, 0
        elif kind == "convert_const":
            self.basis, self.rank = kw["basis"], 0
        elif kind == "lift":
            if not isinstance(ab, SurfaceBasis):
                raise NotImplementedError("Lift of an operand that is not a surface field")
            self.basis, self.rank = kw["basis"], arg.rank
        else:
            raise ValueError(kind)
        self._dev = None

    @property
    def shell(self):
        if self.kind in ("lift", "convert_const"):
            return self.kw["basis"]
        b = self.arg.basis
        return b.shell if isinstance(b, SurfaceBasis) else b

    def termlist(self):
        kw = {k: v for k, v in self.kw.items() if k != "basis"}
        k = self.kw["basis"].k if self.kind in ("lift", "convert_const") else self.arg.basis.k
        return shell_op_termlist(self.kind, self.shell, self.arg.rank, k, **kw)

    def eval_c(self):
        ex = self.dist.executor
        shell = self.shell
        sb = shell.sphere
        if self.kind == "convert":
            # Convert.operate (core/operators.py:1627-1638): an argument that sits in grid space is copied and then
            # transformed straight into the output basis; only coefficient-space arguments see the E matrices
            g = self.arg.grid_native()
            if g is not None:
                return forward(self.dist, self.basis, self.rank, g, self.basis.dealias)
        if self._dev is None or self._dev[0] is not ex:
            # evaluation follows SphericalEllOperator.operate (core/operators.py:3132-3160), which loops over the
            # ell_maps bounding boxes and ACCUMULATES: a slot covered by several boxes receives the sum of their
            # matrices (the per-group subproblem matrices used by the solvers do not have this overlap)
            tl = self.termlist()
            seqs, slot_map = operate_slot_sequences(sb)
            terms = [(co, ci, np.concatenate([m] + [sum(m[l] for l in seq)[None] for seq in seqs])) for (co, ci, m) in tl.terms]
            slot_map = np.array(slot_map[2 * sb.m0:2 * (sb.m0 + sb.nml)])       # a copy: the cached map is shared by all operators
            if tl.rotated and sb.m0 == 0:
                # the msin part of (m, ell) = (0, 0) is no mode of a vector (valid_elements, core/basis.py:4299-4305): the
                # rotation must not carry it into the cos part
                slot_map[1, 0] = -1
            rot = dict(rot=tl.rot) if tl.rotated else {}        # (the NumPy oracle executor knows no rotated terms)
            self._dev = (ex, ex.make_ell_terms(sb.nml, sb.nl, shell.Nr, tl.nco, terms, slot_map, **rot))
        x = _padded(ex, self.arg.eval_c(), shell.Nr)
        y = ex.empty((self.ncomp, 2 * sb.nml, sb.nl, shell.Nr))
        self._dev[1].apply(x, y)
        return _unpadded(ex, y, self.basis.Nr if self.basis is not None else 1)

    def is_grid_native(self):
        return self.kind == "convert" and self.arg.is_grid_native()

    def grid_native(self):
        return self.arg.grid_native() if self.kind == "convert" else None      # Convert.operate copies grid data

    def eval_g(self):
        return self.grid_native() if self.is_grid_native() else _eval_grid(self)

    def lin(self, variables):
        d, dt = self.arg.lin(variables)
        tl = self.termlist()
        return {i: tl.compose(t) for i, t in d.items()}, dt


class ShDt(Dt, ShOperand):
    pass


def _padded(ex, c, Nr):
    """[nc][2 nm][nl][nr] -> [nc][2 nm][nl][Nr] (surface operands have nr = 1)"""
    if int(c.shape[-1]) == Nr:
        return c
    out = ex.zeros(tuple(c.shape[:-1]) + (Nr,))
    ex.assign(out[..., :int(c.shape[-1])], c)
    return out


def _unpadded(ex, c, nr):
    if int(c.shape[-1]) == nr:
        return c
    out = ex.empty(tuple(c.shape[:-1]) + (nr,))
    ex.assign(out, c[..., :nr])
    return out


def _eval_grid(x):
    """grid data [nc][Nphi_g][Ntheta_g][Nr_g] of an operand at the dealias scales"""
    return backward(x.dist, x.basis, x.rank, x.eval_c(), x.basis.dealias)


class ShProduct(ShOperand):
    """a * b (tensor product), a @ b (contraction of the last index of a with the first of b) or cross(a, b) of two
    vectors (CrossProduct, core/arithmetic.py:678-742; grid evaluation only).  With a radial NCC
    (RadialField) as one factor the product is linear in the other one (LHS terms: rvec*lift(tau), b*er); otherwise
    it is evaluated on the dealiased grid (MultiplyFields / DotProduct, core/arithmetic.py:586-674)."""

    def __init__(self, a, b, contract=False, cross=False):
        _no_s2_index("product", a, b)
        self.args, self.contract, self.cross = (a, b), contract, cross
        self.dist = a.dist
        if contract and (a.rank < 1 or b.rank < 1):
            raise ValueError("dot product needs tensors of rank >= 1")
        if cross and (a.rank != 1 or b.rank != 1):
            raise NotImplementedError("cross product of operands that are not both vectors")
        self.rank = 1 if cross else a.rank + b.rank - (2 if contract else 0)
        ncc = [x for x in (a, b) if isinstance(x, RadialField)]
        other = [x for x in (a, b) if not isinstance(x, RadialField)]
        if len(ncc) == 1:
            self.basis = other[0].basis              # k_ncc = 0: the operand's basis
        elif not ncc:
            if not (isinstance(a.basis, ShellBasis) and isinstance(b.basis, ShellBasis)):
                raise NotImplementedError("grid products of operands without shell bases")
            self.basis = a.basis.clone_with(k=a.basis.k + b.basis.k)
        else:
            raise NotImplementedError("product of two radial fields")

    def grid_native(self):
        """grid data of the product at the dealias scales (the layout the product is formed in)"""
        a, b = self.args
        ex = self.dist.executor
        Np, Nt, Ng = self.basis.grid_shape(self.basis.dealias)
        Nt = self.dist.theta_range(Nt)[1]
        ga = a.grid_broadcast(ex, self.basis, (Np, Nt, Ng)) if isinstance(a, RadialField) else a.eval_g()
        gb = b.grid_broadcast(ex, self.basis, (Np, Nt, Ng)) if isinstance(b, RadialField) else b.eval_g()
        terms, nout = (CROSS_TERMS, 3) if self.cross else bilinear_terms(3, a.rank, b.rank, self.contract)
        out = ex.empty((nout, Np, Nt, Ng))
        ex.bilinear(out, nout, ga, gb, Np * Nt * Ng, terms)
        return out

    def is_grid_native(self):
        return True

    def eval_c(self):
        return forward(self.dist, self.basis, self.rank, self.grid_native(), self.basis.dealias)

    def eval_g(self):
        return self.grid_native()

    def lin(self, variables):
        a, b = self.args
        if isinstance(a, RadialField):
            ncc, arg, ncc_first = a, b, True
        elif isinstance(b, RadialField):
            ncc, arg, ncc_first = b, a, False
        else:
            raise NonlinearError("products of fields are nonlinear")
        if self.cross:
            raise NotImplementedError("cross product with a radial field in a shell LHS")
        if not isinstance(arg.basis, ShellBasis):
            raise NotImplementedError("NCC product with an operand that has no shell basis")
        d, isdt = arg.lin(variables)
        tl = ncc_termlist(ncc, arg.basis, arg.rank, ncc_first, self.contract)
        return {i: tl.compose(t) for i, t in d.items()}, isdt


# a x b in the component order (phi, theta, r), which is LEFT-handed (SphericalCoordinates.right_handed = False,
# core/coords.py:326): CrossProduct.operate_left_handed (core/arithmetic.py:719-728), as (out, ia, ib, sign)
CROSS_TERMS = [(0, 2, 1, 1.0), (0, 1, 2, -1.0), (1, 0, 2, 1.0), (1, 2, 0, -1.0), (2, 1, 0, 1.0), (2, 0, 1, -1.0)]


ShOperand.scale_type, ShOperand.add_type, ShOperand.product = ShScale, ShAdd, ShProduct


def ncc_termlist(ncc, arg_basis, rank_arg, ncc_first, contract):
    """LHS matrix blocks of a product with a radial NCC (Basis._last_axis_field_ncc_matrix, core/basis.py:283-330, with
    ShellRadialBasis._last_axis_component_ncc_matrix :3879-3910): block (gamma <- beta) at ell =
    sum_alpha Gamma_ell[alpha, beta, gamma] * Mult(a_alpha), Mult = multiplication by the NCC's regularity component
    alpha as a function of r in the operand's Jacobi family (exact Gauss quadrature; the reference's Clenshaw sum
    of the same polynomial)."""
    from ..tools import jacobi
    shell = arg_basis
    sb = shell.sphere
    nl, Nr, k = sb.nl, shell.Nr, arg_basis.k
    a_fam, b_fam = k + shell.alpha[0], k + shell.alpha[1]
    # NCC regularity components as functions of z: coefficients in the k = 0 family, evaluated at the quadrature nodes
    coef = ncc.regularity_coefficients()                     # [3^rank_ncc][Nr]
    nq = Nr + coef.shape[1] + 2
    zq, wq = jacobi.quadrature(nq, a_fam, b_fam)
    zq, wq = np.asarray(zq, dtype=np.float64), np.asarray(wq, dtype=np.float64)
    P = np.asarray(jacobi.polynomials(Nr, a_fam, b_fam, zq))                         # [Nr][nq]
    P0 = np.asarray(jacobi.polynomials(coef.shape[1], shell.alpha[0], shell.alpha[1], zq))
    mult = []
    for alpha_c in range(coef.shape[0]):
        f = coef[alpha_c] @ P0
        if np.any(np.abs(coef[alpha_c]) > 1e-14):
            M = (P * (wq * f)) @ P.T
            M[np.abs(M) < 1e-13 * np.abs(M).max()] = 0.0         # quadrature round-off outside the band of the polynomial
            mult.append(M)
        else:
            mult.append(None)
    rank_ncc = ncc.rank
    rank_out = rank_ncc + rank_arg - (2 if contract else 0)
    idx_arg, idx_out = reg_indices(rank_arg), reg_indices(rank_out)
    acc = {}
    for ell in range(nl):
        if ncc_first:
            G = gamma_regularity(rank_ncc, rank_arg, 0, ell, ell, contract)          # [alpha, beta, gamma]
        else:
            G = gamma_regularity(rank_arg, rank_ncc, ell, 0, ell, contract).transpose(1, 0, 2)
        if np.abs(G.imag).max() > 1e-12:
            raise NotImplementedError("complex product coefficients for real fields")
        G = G.real
        for be, tb in enumerate(idx_arg):
            if not regularity_allowed(ell, tb):
                continue
            for ga, tg in enumerate(idx_out):
                if not regularity_allowed(ell, tg):
                    continue
                for al in range(G.shape[0]):
                    if mult[al] is None or abs(G[al, be, ga]) <= 1e-6:             # ncc_cutoff of the reference
                        continue
                    m = acc.setdefault((ga, be), np.zeros((nl, Nr, Nr)))
                    m[ell] += G[al, be, ga] * mult[al]
    return EllTermList(len(idx_out), len(idx_arg), [(co, ci, m) for (co, ci), m in sorted(acc.items())])


def lap(a):
    return ShLinear("lap", a)


def trace(a):
    return ShLinear("trace", a)


def integ(a, *coords):
    return ShLinear("integ", a)


def ave(a, *coords):
    """Average(f, coords['phi']) -> zonal mean; Average(f, coords.S2coordsys) or ave(f) -> the average over the spheres
    r = const, a radial profile.  Coordinates by object or by name, as the reference accepts them."""
    if len(coords) == 1 and isinstance(coords[0], (tuple, list)):
        coords = tuple(coords[0])
    cs = a.dist.coordsys
    if isinstance(a, ShReduced):
        raise sphreduce.reduction_refused("average", a.what)
    if not coords:
        return ShSphereAverage(a)
    names = [c if isinstance(c, str) else getattr(c, "name", None) for c in coords]
    if len(coords) == 1 and (coords[0] is cs.azimuth or names[0] == cs.azimuth.name):
        return ShAzimuthalAverage(a)
    if (len(coords) == 1 and isinstance(coords[0], S2Coordinates)) or \
            (len(coords) == 2 and set(names) == {cs.azimuth.name, cs.colatitude.name}):
        return ShSphereAverage(a)
    raise NotImplementedError("average of a shell operand over %r" % (coords,))


Average = ave


def grad(a):
    return ShLinear("grad", a)


def div(a):
    return ShLinear("div", a)


def curl(a):
    """curl of a vector operand on a ShellBasis; the result lives in the k + 1 basis (SphericalCurl._output_basis)"""
    if not isinstance(a, ShOperand):
        raise ValueError("curl needs a field operand")
    return ShLinear("curl", a)


def cross(a, b):
    """a x b of two vector operands, formed on the dealiased grid; a RadialField factor is broadcast to the grid"""
    if not (isinstance(a, ShOperand) and isinstance(b, ShOperand)):
        raise ValueError("cross needs two field operands")
    return ShProduct(a, b, cross=True)


Curl, CrossProduct = curl, cross


def _spin_selection(kind, sig, **kw):
    """(P [ncomp_out][ncomp_in], sig_out) on spin (equally: coordinate) components, index tuples over `sig` in C order:
    the permutation of TransposeComponents (core/operators.py:1916-1934), the selection of S2RadialComponent
    (core/basis.py:5896-5911: the components whose index `index` is 2, the radial one) or that of S2AngularComponent
    (:5937-5950: the components whose index is - or +, which becomes an S2 index of two components)."""
    idx_in = list(np.ndindex(*sig))
    if kind == "trans":
        i, j = kw["indices"]
        sig_out = list(sig)
        sig_out[i], sig_out[j] = sig[j], sig[i]
        keep = lambda t: True
        image = lambda t: tuple(t[j] if a == i else t[i] if a == j else t[a] for a in range(len(t)))
    elif kind == "radial":
        index = kw["index"]
        sig_out = list(sig[:index] + sig[index + 1:])
        keep = lambda t: t[index] == 2
        image = lambda t: tuple(t[:index] + t[index + 1:])
    else:
        index = kw["index"]
        sig_out = list(sig[:index] + (2,) + sig[index + 1:])
        keep = lambda t: t[index] < 2
        image = lambda t: tuple(t)
    idx_out = list(np.ndindex(*sig_out))
    P = np.zeros((len(idx_out), len(idx_in)))
    for ci, t in enumerate(idx_in):
        if keep(t):
            P[idx_out.index(image(t)), ci] = 1.0
    return P, tuple(sig_out)


class ShMix(ShOperand):
    """trans(T, indices) / radial(T, index) / angular(T, index): a mix of the components of every (m, ell) line, the identity along n.  On the
    spin components of a surface operand it is the permutation / selection P itself, on the regularity components of a shell
    operand Q_out(ell)^T P Q_in(ell) (SphericalTransposeComponents, core/operators.py:1984-2045).  The result keeps the
    operand's basis."""

    def __init__(self, kind, arg, **kw):
        name = kind
        if not isinstance(arg, ShOperand):
            raise ValueError("%s needs a field operand" % name)
        if isinstance(arg, RadialField):
            raise NotImplementedError("%s of a radial operand %r" % (name, arg))
        if isinstance(arg, ConstField) or arg.basis is None:
            raise NotImplementedError("%s of a constant operand %r" % (name, arg))
        if isinstance(arg, ShReduced):
            raise NotImplementedError("%s of a reduced operand (%s)" % (name, arg.what))
        self.kind, self.arg, self.args, self.kw = kind, arg, (arg,), kw
        self.dist, self.basis = arg.dist, arg.basis
        if kind == "trans":
            i, j = kw["indices"]
            if arg.rank < 2 or not (0 <= i < arg.rank and 0 <= j < arg.rank):
                raise ValueError("trans needs a tensor of rank >= 2 and two of its indices")
            self.rank = arg.rank
        else:
            if not 0 <= kw["index"] < arg.rank:
                raise ValueError("index greater than rank")
            if arg.sig[kw["index"]] != 3:
                raise ValueError("%s of an index that is an S2 index already" % kind)
            self.rank = arg.rank - 1 if kind == "radial" else arg.rank
        if not isinstance(self.basis, SurfaceBasis) and (kind == "angular" or any(d != 3 for d in arg.sig)):
            # the reference has AngularComponent on surface operands only (S2AngularComponent, basis_type = SphereBasis), and
            # there are no Q(ell) for a tensor with an S2 index in the volume
            raise NotImplementedError("%s of the shell (volume) operand %r: an S2 index exists on surface operands, "
                                      "take u(r=R0) first" % (kind, arg))
        self.P, self._sig = _spin_selection(kind, arg.sig, **kw)
        self._dev = None

    def mixlist(self):
        """per ell (the subproblem matrices of a left-hand side)"""
        sb = self.basis.sphere
        if isinstance(self.basis, SurfaceBasis):
            mats = np.broadcast_to(self.P, (sb.nl,) + self.P.shape)
        else:
            Qo = [sph.intertwiner(ell, self.rank) if self.rank else np.eye(1) for ell in range(sb.nl)]
            mats = np.array([Qo[ell].T @ self.P @ sph.intertwiner(ell, self.arg.rank) for ell in range(sb.nl)])
            mats[np.abs(mats) < 1e-14] = 0.0
        return EllMixList.from_matrices(mats)

    def _slot_mix(self):
        """(terms (co, ci, q [nq]), slot map [2 nml][nl]) for EVALUATION: a slot that the packed layout covers with several
        ell boxes is recombined by each of them in turn (ShellBasis.regularity_plan), so its mix is F_out P B_in with the
        products F, B of those Q(ell)^T, Q(ell)."""
        sb = self.basis.sphere
        rows, cols, ok = sb.pack_index()
        slot_p, _, bwd = curvilinear.recombination_tables(sb.packed_ell_rows(), sb.packed_shape(), self.arg.rank)
        if isinstance(self.basis, SurfaceBasis):
            mats = np.broadcast_to(self.P, (len(bwd),) + self.P.shape)
        else:
            fwd = curvilinear.recombination_tables(sb.packed_ell_rows(), sb.packed_shape(), self.rank)[1] if self.rank \
                else np.ones((len(bwd), 1, 1))
            mats = np.array([fwd[i] @ self.P @ bwd[i] for i in range(len(bwd))])
            mats[np.abs(mats) < 1e-14] = 0.0
        slot = -np.ones((2 * sb.nm, sb.nl), dtype=np.int32)
        slot[rows[ok], cols[ok]] = slot_p[ok]
        return EllMixList.from_matrices(mats).terms, np.ascontiguousarray(slot[2 * sb.m0:2 * (sb.m0 + sb.nml)])

    def is_grid_native(self):
        return self.kind != "angular" and self.arg.is_grid_native()

    def grid_native(self):
        """operands formed on the grid are permuted there (TransposeComponents.operate, core/operators.py:2033-2035)"""
        if not self.is_grid_native():
            return None
        ex = self.dist.executor
        g = self.arg.grid_native()
        out = ex.empty((self.ncomp,) + tuple(g.shape[1:]))
        for co, ci in zip(*np.nonzero(self.P)):
            ex.assign(out[int(co):int(co) + 1], g[int(ci):int(ci) + 1])
        return out

    def eval_g(self):
        return self.grid_native() if self.is_grid_native() else _eval_grid(self)

    def eval_c(self):
        if self.is_grid_native():
            return forward(self.dist, self.basis, self.rank, self.grid_native(), self.basis.dealias)
        ex = self.dist.executor
        sb = self.basis.sphere
        if getattr(ex, "make_ell_mix", None) is None:
            raise NotImplementedError("the executor %r has no component mix (make_ell_mix)" % (ex,))
        if self._dev is None or self._dev[0] is not ex:
            terms, slot_map = self._slot_mix()
            self._dev = (ex, ex.make_ell_mix(sb.nml, sb.nl, self.basis.Nr, self.ncomp, self.arg.ncomp, terms, slot_map))
        y = ex.empty((self.ncomp, 2 * sb.nml, sb.nl, self.basis.Nr))
        self._dev[1].apply(self.arg.eval_c(), y)
        return y

    def lin(self, variables):
        d, isdt = self.arg.lin(variables)
        ml = self.mixlist()
        return {i: ml.compose(t) for i, t in d.items()}, isdt


def _tensor_index(a, index):
    """negative indices count from the last one (Component.__init__, core/operators.py:2201)"""
    index = int(index)
    return index + getattr(a, "rank", 0) if index < 0 else index


def trans(a, indices=(0, 1)):
    """TransposeComponents of a shell or surface tensor of rank >= 2 (both indices spherical); the result keeps the basis"""
    i, j = (_tensor_index(a, i) for i in indices)
    return ShMix("trans", a, indices=(i, j))


def radial(a, index=0):
    """RadialComponent: drops the tensor index `index`.  The reference defines it on surface operands (u(r=R0)) only; on a
    shell (volume) operand it is an extension of this code, the same selection between the Q(ell) of the operand and of
    the result (its test data is the reference's coordinate component, not a reference operator: DESIGN.md section 9)."""
    return ShMix("radial", a, index=_tensor_index(a, index))


def angular(a, index=0):
    """AngularComponent of a surface operand (u(r=R0)): the index becomes an S2 index of the two components (-, +).  The
    result serves as boundary rows and as a coefficient-space task; it has no grid data here."""
    return ShMix("angular", a, index=_tensor_index(a, index))


transpose, TransposeComponents, RadialComponent, AngularComponent = trans, trans, radial, angular


class ShEllProduct(ShOperand):
    """SphericalEllProduct(T, coordsys, ell_func) of a shell (volume) operand (SphericalEllProductField, core/operators.py:
    4169-4214): every regularity component times ell_func(ell + regtotal), the identity along n, no mixing between
    components; basis, rank and sig are those of the operand.  A diagonal EllMixList.  `parts` is a list of
    (factor, ell_func): scalar multiples and sums of ell products of one operand stay one node and one mix.
    ell_func is called on the host, once per distinct ell + regtotal of an existing mode, when the node is made."""

    name = "SphericalEllProduct"

    def __init__(self, arg, coordsys, ell_func, _parts=None):
        name = self.name
        if not isinstance(arg, ShOperand):
            raise ValueError("%s needs a field operand" % name)
        if coordsys is not arg.dist.coordsys:
            raise ValueError("%s: %r is not the operand's coordinate system" % (name, coordsys))
        if isinstance(arg, RadialField):
            raise NotImplementedError("%s of a radial operand %r" % (name, arg))
        if isinstance(arg, ConstField) or arg.basis is None:
            raise NotImplementedError("%s of a constant operand %r" % (name, arg))
        if isinstance(arg, ShReduced):
            raise NotImplementedError("%s of a reduced operand (%s)" % (name, arg.what))
        _no_s2_index(name, arg)
        if isinstance(arg.basis, SurfaceBasis):
            # the reference dispatches to SphericalEllProductField alone, whose radial matrices need the operand's radial
            # basis: a surface operand (u(r=R0)) fails there.  Take the product first: SphericalEllProduct(u, ...)(r=R0)
            raise NotImplementedError("%s of the surface operand %r: multiply in the volume, then interpolate" % (name, arg))
        parts = [(1.0, ell_func)] if _parts is None else list(_parts)
        if not all(callable(f) for (a, f) in parts):
            raise ValueError("%s needs a function of ell" % name)
        self.arg, self.args, self.coordsys, self.parts = arg, (arg,), coordsys, parts
        self.dist, self.basis, self.rank, self._sig = arg.dist, arg.basis, arg.rank, arg.sig
        self.q = self._table()
        self._dev = None

    def _table(self):
        """q [ncomp][nl]: sum of factor * ell_func(ell + regtotal) on the modes that exist, 0 elsewhere"""
        nl = self.basis.sphere.nl
        idx = reg_indices(self.rank)
        q = np.zeros((len(idx), nl))
        for a, func in self.parts:
            seen = {}
            for c, t in enumerate(idx):
                rt = regtotal(t)
                for ell in range(nl):
                    if not regularity_allowed(ell, t):
                        continue                                  # no mode: ell_func is not asked, the entry stays 0
                    if ell + rt not in seen:
                        v = func(ell + rt)
                        if isinstance(v, numbers.Complex) and not isinstance(v, numbers.Real) or np.iscomplexobj(v):
                            raise NotImplementedError("%s: ell_func(%d) = %r is complex; the per-ell systems are real"
                                                      % (self.name, ell + rt, v))
                        v = float(v)
                        if not np.isfinite(v):
                            raise ValueError("%s: ell_func(%d) = %r is not finite" % (self.name, ell + rt, v))
                        seen[ell + rt] = v
                    q[c, ell] += a * seen[ell + rt]
        return q

    def _like(self, parts):
        return ShEllProduct(self.arg, self.coordsys, None, _parts=parts)

    def __mul__(self, other):
        if isinstance(other, numbers.Number):
            return self._like([(float(other) * a, f) for (a, f) in self.parts])
        return ShOperand.__mul__(self, other)

    __rmul__ = __mul__

    def __neg__(self):
        return self * -1.0

    def __truediv__(self, other):
        if isinstance(other, numbers.Number):
            return self * (1.0 / other)
        return NotImplemented

    def __add__(self, other):
        if isinstance(other, ShEllProduct) and other.arg is self.arg:
            return self._like(self.parts + other.parts)
        return ShOperand.__add__(self, other)

    __radd__ = __add__

    def __sub__(self, other):
        if isinstance(other, ShEllProduct) and other.arg is self.arg:
            return self + (-other)
        return ShOperand.__sub__(self, other)

    def mixlist(self):
        """per ell (the subproblem matrices of a left-hand side)"""
        return EllMixList(self.ncomp, self.ncomp, [(c, c, self.q[c]) for c in range(self.ncomp) if np.any(self.q[c] != 0)])

    def _slot_mix(self):
        """(terms (c, c, q [nq]), slot map [2 nml][nl]) for EVALUATION: SphericalEllOperator.operate (core/operators.py:
        3136-3167) loops over the ell_maps boxes and accumulates, so a slot that the packed layout covers with several
        boxes gets the sum of their scalars (the extra ids of operate_slot_sequences, as for the radial operators)."""
        sb = self.basis.sphere
        seqs, slot = operate_slot_sequences(sb)
        terms = [(c, c, np.concatenate([q, [sum(q[l] for l in seq) for seq in seqs]])) for (c, _, q) in self.mixlist().terms]
        return terms, np.ascontiguousarray(slot[2 * sb.m0:2 * (sb.m0 + sb.nml)])

    def eval_c(self):
        ex = self.dist.executor
        sb = self.basis.sphere
        if getattr(ex, "make_ell_mix", None) is None:
            raise NotImplementedError("the executor %r has no component mix (make_ell_mix)" % (ex,))
        if self._dev is None or self._dev[0] is not ex:
            terms, slot_map = self._slot_mix()
            self._dev = (ex, ex.make_ell_mix(sb.nml, sb.nl, self.basis.Nr, self.ncomp, self.ncomp, terms, slot_map))
        y = ex.empty((self.ncomp, 2 * sb.nml, sb.nl, self.basis.Nr))
        self._dev[1].apply(self.arg.eval_c(), y)
        return y

    def lin(self, variables):
        d, isdt = self.arg.lin(variables)
        ml = self.mixlist()
        return {i: ml.compose(t) for i, t in d.items()}, isdt


def SphericalEllProduct(a, coordsys, ell_func):
    """d3.SphericalEllProduct of a shell operand; a number gives 0 as in the reference's dispatch (core/operators.py:4160-4163)"""
    if isinstance(a, numbers.Number):
        return 0
    return ShEllProduct(a, coordsys, ell_func)


def dt(a):
    return ShDt(a)


def Lift(a, basis, n):
    return ShLinear("lift", a, basis=basis, n=int(n))


class ConstField(ShOperand):
    """A field without bases in a SphericalCoordinates distributor (tau_p): one number."""

    def __init__(self, dist, name=None):
        self.dist, self.name, self.basis, self.rank = dist, name, None, 0
        self._value = np.zeros((1, 1, 1))
        self._host_dirty = True          # the host copy has to reach the solver's state vector before the next step
        self._pull = None                # set by the solver after a step: fetches the solved value when somebody asks
        self.args = ()

    def __repr__(self):
        return self.name or "<ConstField %d>" % id(self)

    @property
    def value(self):
        """The number, as a (1, 1, 1) array.  While a solver steps, the solved value stays on the device (no host round
        trip per step); it is fetched here, on demand -- and since the caller may write into the array it gets, the
        host copy counts as modified from then on (one small upload before the next step)."""
        if self._pull is not None:
            pull, self._pull = self._pull, None
            self._value[...] = pull()
        self._host_dirty = True
        return self._value

    def __getitem__(self, key):
        return self.value

    def __setitem__(self, key, data):
        self._pull = None
        self._value[...] = data
        self._host_dirty = True

    def change_scales(self, scales):
        pass

    def has_dt(self):
        return False

    def lin(self, variables):
        for i, v in enumerate(variables):
            if v is self:
                shell = [x.shell for x in variables if hasattr(x, "shell")][0]
                sb = shell.sphere
                return {i: EllTermList.identity(1, sb.nl, getattr(shell, "_root", shell).Nr, 1)}, False
        raise NonlinearError("%r is not a problem variable" % (self,))

    def eval_c(self):
        raise NotImplementedError("constants are converted to a shell basis before evaluation")

    def cfl_term(self, velocity):
        """A constant as a CFL frequency (ShOperand.cfl_term): one point along every axis"""
        if velocity:
            raise ValueError("CFL velocity must be a vector field on a shell")
        ex = self.dist.executor
        return dict(kind="scalar"), (1, 1, 1), lambda: ex.from_host(np.array(self.value, dtype=np.float64).reshape(1, 1, 1, 1))

    # solver interface
    def _cshape_in(self, shell):
        sb = shell.sphere
        return (1, 2 * sb.nml, sb.nl, 1)


class RadialField(ShOperand):
    """Tensor field that depends on r only (NCC: er, rvec): coordinate components on the radial Gauss grid, kept on the
    host (it only enters the LHS matrices)."""

    def __init__(self, dist, shell, rank=0, name=None):
        self.dist, self.shell_basis, self.rank, self.name = dist, shell, rank, name
        self.basis = shell
        self.args = ()
        self._g = np.zeros((3,) * rank + (1, 1, shell.Nr))

    def __getitem__(self, key):
        if key not in ("g", "grid"):
            raise NotImplementedError("coefficient access of radial fields")
        return self._g

    def __setitem__(self, key, data):
        self._g[...] = data

    def has_dt(self):
        return False

    def lin(self, variables):
        raise NonlinearError("a radial field is a coefficient, not a variable")

    def grid_profile(self, Ng):
        """[3^rank][Ng]: the radial profile re-sampled spectrally on the radial Gauss grid of Ng points"""
        from ..tools import jacobi
        shell = self.shell_basis
        nc = 3 ** self.rank
        z, w = jacobi.quadrature(shell.Nr, shell.alpha[0], shell.alpha[1])
        P = np.asarray(jacobi.polynomials(shell.Nr, shell.alpha[0], shell.alpha[1], z))
        coef = self._g.reshape(nc, shell.Nr) @ (P * np.asarray(w, dtype=np.float64)).T
        zg, _ = jacobi.quadrature(Ng, shell.alpha[0], shell.alpha[1])
        Pg = np.asarray(jacobi.polynomials(shell.Nr, shell.alpha[0], shell.alpha[1], zg), dtype=np.float64)
        return coef @ Pg

    def cfl_term(self, velocity):
        """A radial profile as a CFL frequency (ShOperand.cfl_term): [1][1][1][Nr_g] on the device, one point along both
        angles -- the fused reduction reads it with stride 0 there."""
        if velocity or self.rank != 0:
            raise ValueError("a radial field enters the CFL sum as a scalar frequency only")
        shell = self.shell_basis
        Ng = int(shell.grid_shape(shell.dealias)[2])
        ex = self.dist.executor
        store = getattr(shell, "_root", shell)._plans
        key = ("cfl_profile", id(ex), id(self))

        def data():
            if key not in store or store[key][0] != self._g.tobytes():
                store[key] = (self._g.tobytes(), ex.from_host(np.ascontiguousarray(self.grid_profile(Ng).reshape(1, 1, 1, Ng))))
            return store[key][1]
        return dict(kind="scalar"), (1, 1, Ng), data

    def grid_broadcast(self, ex, basis, shape):
        """coordinate components on the dealiased grid [3^rank][Nphi_g][Ntheta_local][Nr_g] (analysis products such as
        er @ flux): the radial profile is re-sampled spectrally on the finer radial grid and repeated over the angles"""
        shell = self.shell_basis
        Np, Nt, Ng = shape
        key = ("ncc_grid", id(ex), id(self), shape)
        store = getattr(shell, "_root", shell)._plans
        if key not in store or store[key][0] != self._g.tobytes():
            nc = 3 ** self.rank
            prof = self.grid_profile(Ng)                       # [nc][Ng]
            full = np.ascontiguousarray(np.broadcast_to(prof[:, None, None, :], (nc, Np, Nt, Ng)))
            store[key] = (self._g.tobytes(), ex.from_host(full))
        return store[key][1]

    def regularity_coefficients(self):
        """[3^rank][Nr]: Jacobi (k = 0 family) coefficients of the regularity components at ell = 0."""
        from ..tools import jacobi
        shell = self.shell_basis
        nc = 3 ** self.rank
        g = self._g.reshape(nc, shell.Nr)
        if self.rank:
            U = SphericalCoordinates.U_forward(self.rank)
            spin = U @ g
            if np.abs(spin.imag).max() > 1e-14:
                raise NotImplementedError("radial NCC with angular components")
            reg = sph.intertwiner(0, self.rank).T @ spin.real
        else:
            reg = g
        z, w = jacobi.quadrature(shell.Nr, shell.alpha[0], shell.alpha[1])
        P = np.asarray(jacobi.polynomials(shell.Nr, shell.alpha[0], shell.alpha[1], z))
        return reg @ (P * np.asarray(w, dtype=np.float64)).T


class ShellField(HostMirror, ShOperand):
    """Tensor field on a ShellBasis (or one of its surfaces): device-resident data with lazily synchronised host mirrors, `['g']` / `['c']`
    in the reference's shapes (packed (m, ell) coefficient layout, core/basis.py:2839-2891)."""

    def __init__(self, dist, basis, rank=0, name=None, sig=None):
        self.dist, self.basis, self.rank, self.name = dist, basis, rank, name
        if sig is not None and tuple(sig) != (3,) * rank:
            self._sig = tuple(sig)                  # a task with an S2 index (angular): coefficient data only
        self._init_mirror(3)
        self.args = ()

    @property
    def shell(self):
        return self.basis.shell if isinstance(self.basis, SurfaceBasis) else self.basis

    @property
    def k(self):
        return self.basis.k

    @property
    def tensorsig(self):
        return (self.dist.coordsys,) * self.rank

    # ---- expression protocol ---------------------------------------------------------------------------------------
    def eval_c(self):
        return self.require_coeff_space()

    def lin(self, variables):
        for i, v in enumerate(variables):
            if v is self:
                sb = self.basis.sphere
                return {i: EllTermList.identity(self.ncomp, sb.nl, self.shell.Nr, self.basis.Nr)}, False
        raise NonlinearError("%r is not a problem variable" % (self,))

    def has_dt(self):
        return False

    def evaluate(self):
        return self

    def __repr__(self):
        return self.name or "<ShellField %d>" % id(self)

    @property
    def ex(self):
        return self.dist.executor

    def _cshape(self):
        sb = self.basis.sphere
        return (self.ncomp, 2 * sb.nml, sb.nl, self.basis.Nr)

    def _set_device_coeff(self, c):
        """the solver wrote the coefficients on the device.  Deliberately drops _g, which a sphere field keeps here."""
        self._c = c
        self.layout = "c"
        self._authority = "device"
        self._g = None

    def _global_shape(self, layout, scales):
        t = tuple(self.sig)
        if layout == "g":
            if t != (3,) * self.rank:
                raise NotImplementedError("grid data of a field with an S2 index (angular)")
            return t + self.basis.grid_shape(scales)
        return t + self.basis.sphere.packed_shape() + (self.basis.Nr,)

    def _local_slices(self, layout, scales):
        """slices of the global user array held by this rank: colatitude block in grid space, block of the packed
        azimuthal axis in coefficient space (Layout.local_chunks of the reference, core/distributor.py:357-385)"""
        sl = [slice(None)] * (self.rank + 3)
        d = self.dist
        if d.size > 1:
            if layout == "g":
                t0, nt = d.theta_range(self.basis.grid_shape(scales)[1])
                sl[self.rank + 1] = slice(t0, t0 + nt)
            else:
                n = self.basis.sphere.packed_shape()[0]
                if n % (2 * d.size):
                    raise ValueError("packed azimuthal axis of %d does not divide over %d ranks" % (n, d.size))
                sl[self.rank] = slice(d.rank * (n // d.size), (d.rank + 1) * (n // d.size))
        return tuple(sl)

    def _user_shape(self, layout, scales):
        g = self._global_shape(layout, scales)
        return tuple(len(range(*sl.indices(n))) for sl, n in zip(self._local_slices(layout, scales), g))

    def _natural_from_packed(self, h):
        """user (packed, local block) coefficients -> natural [ncomp][2 nml][nl][Nr] of the local wavenumbers.  On several
        ranks the folded part of the packed layout belongs to other ranks' wavenumbers: the blocks are all-gathered
        (user access is a synchronisation point, not part of the step)."""
        sb = self.basis.sphere
        rows, cols, ok = sb.pack_index()
        h = h.reshape((self.ncomp, -1, rows.shape[1], self.basis.Nr))
        if self.dist.size > 1:
            h = self.dist.pcomm.all_gather_host(h, axis=1)
        nat = np.zeros((self.ncomp, 2 * sb.nm, sb.nl, self.basis.Nr))
        for c in range(self.ncomp):
            nat[c][rows[ok], cols[ok], :] = h[c][ok]
        return np.ascontiguousarray(nat[:, 2 * sb.m0:2 * (sb.m0 + sb.nml)])

    def _packed_from_natural(self, nat):
        sb = self.basis.sphere
        if self.dist.size > 1:
            nat = self.dist.pcomm.all_gather_host(np.ascontiguousarray(nat), axis=1)
        rows, cols, ok = sb.pack_index()
        out = np.zeros((self.ncomp,) + rows.shape + (self.basis.Nr,))
        for c in range(self.ncomp):
            out[c][ok] = nat[c][rows[ok], cols[ok], :]
        out = out.reshape(self._global_shape("c", self.scales))
        return np.ascontiguousarray(out[self._local_slices("c", self.scales)])

    # ---- hooks of the mirror protocol (core/mirror.py) -------------------------------------------------------------
    def _host_to_device(self, layout, scales, host):
        if layout == "c":
            self.ex.upload(self._coeff_array(), self._natural_from_packed(host))
        else:
            shape = (self.ncomp,) + self._user_shape("g", scales)[self.rank:]
            if self._g is None or self._g_scales != scales:
                self._g = self.ex.empty(shape)
                self._g_scales = scales
            self.ex.upload(self._g, np.ascontiguousarray(host.reshape(shape)))
            self.scales = scales
        self.layout = layout

    def _device_to_host(self, layout, scales):
        shape = self._user_shape(layout, scales)
        if layout == "c":
            nat = np.asarray(self.ex.download(self.require_coeff_space()))
            return self._packed_from_natural(nat).reshape(shape)
        return np.array(self.ex.download(self.require_grid_space(scales))).reshape(shape)

    def _forward_transform(self):
        self._c = forward(self.dist, self.basis, self.rank, self._g, self._g_scales)

    def _backward_transform(self, c, scales):
        self._g = backward(self.dist, self.basis, self.rank, c, scales)       # (deliberate: the transform's own array)
        self._g_scales = scales

    def _coeff_array(self):
        if self._c is None:
            self._c = self.ex.zeros(self._cshape())
        return self._c

    def cfl_frequency_max(self):
        """max over the dealiased grid of the advective CFL frequency of this velocity field (Spherical3DAdvectiveCFL,
        core/basis.py:6183-6204), reduced on the device."""
        if self.rank != 1 or not isinstance(self.basis, ShellBasis):
            raise ValueError("CFL velocity must be a vector field on a shell")
        ex = self.ex
        inv_h, inv_dr = _cfl_spacings(self.basis, ex)
        g = self.eval_g()
        return ex.cfl_max_spherical(g, inv_h, inv_dr)


def _cfl_spacings(shell, ex):
    """device arrays (1 / horizontal spacing, 1 / radial spacing) over the dealiased radial grid (Spherical3DAdvectiveCFL.
    cfl_spacing, core/basis.py:6187-6198)"""
    key = ("cfl", id(ex))
    store = getattr(shell, "_root", shell)._plans
    if key not in store:
        sc = shell.dealias
        r = shell.radius_grid(sc[2])
        Lmax = shell.sphere.Lmax
        h = r / np.sqrt(Lmax * (Lmax + 1)) if Lmax > 0 else np.full_like(r, np.inf)
        dr = np.gradient(r, edge_order=2) * sc[2]
        store[key] = (ex.from_host(np.ascontiguousarray(1.0 / h)), ex.from_host(np.ascontiguousarray(1.0 / np.abs(dr))))
    return store[key]


# ==================================================================================================
# problems and solvers (per-ell systems)
# ==================================================================================================

class ShellProblem(CurvilinearProblem):
    operand_type = ShOperand
    operators = dict(lap=lap, grad=grad, div=div, dt=dt, Lift=Lift, lift=Lift, trace=trace, integ=integ,
                     Laplacian=lap, Gradient=grad, Divergence=div, TimeDerivative=dt, Trace=trace,
                     Integrate=integ, ave=ave, Average=ave, curl=curl, Curl=curl, cross=cross, CrossProduct=cross,
                     trans=trans, transpose=trans, TransposeComponents=trans, radial=radial, RadialComponent=radial,
                     angular=angular, AngularComponent=angular, SphericalEllProduct=SphericalEllProduct)

    def __init__(self, variables, namespace=None, time="t"):
        super().__init__(variables, namespace, time)
        shells = [v.shell for v in self.variables if hasattr(v, "shell")]
        self.shell = getattr(shells[0], "_root", shells[0])

    def _lin(self, node):
        d, isdt = node.lin(self.variables)
        # a rotated term (the curl: i A on cos + i msin) makes the per-ell systems complex: only where the executor
        # solves such systems (csrc/ddh_ellband.hip, complex instances)
        if any(t.rotated for t in d.values()) and not getattr(self.dist.executor, "complex_ell_systems", False):
            raise NotImplementedError("curl in a shell LHS: per-ell systems are real")
        return d, isdt

    def _numeric_rhs(self, rhs):
        return None if rhs == 0 else float(rhs)         # (deliberate: the sphere refuses a non-zero number)

    def _operand_rhs(self, lhs, rhs):
        return _converted(rhs, lhs.basis) if isinstance(lhs.basis, ShellBasis) else rhs

    def _equation_keys(self, lhs):
        return dict(basis=lhs.basis)


class ShellIVP(ShellProblem):
    @property
    def solver_class(self):
        return ShellInitialValueSolver


class ShellLBVP(ShellProblem):
    @property
    def solver_class(self):
        return ShellBoundaryValueSolver


def _valid_modes(basis, sig, nl, Nr):
    """[ncomp][nl][Nr] validity of (component, ell, n): regularity components of a shell field, spin components of
    a surface field (n = 0 only; an S2 index has the components -, + alone)."""
    out = np.zeros((int(np.prod(sig, dtype=np.int64)), nl, Nr), dtype=bool)
    if basis is None:                       # constants: the (ell = 0, n = 0) mode only
        out[0, 0, 0] = True
        return out
    for c, idx in enumerate(np.ndindex(*sig)):
        for ell in range(nl):
            if isinstance(basis, SurfaceBasis):
                out[c, ell, 0] = spin_allowed(ell, idx)
            else:
                out[c, ell, :] = regularity_allowed(ell, idx)
    return out


class ShellSolverBase:
    """Per-ell systems: the matrices depend on ell only (matrix_dependence of the reference), every
    (m, part) slot of that ell is a right-hand-side column.  System vectors are [R][2 nm][nl][Nr]: one system component
    per component of a shell-basis variable / equation, while the components that have a single radial point (surface
    tau fields, constants, boundary rows) are PACKED along n of shared components, so that the system stays a small
    number of full Nr x Nr blocks (dense GEMM blocks for the inverse) instead of many single-row / single-column ones."""

    def __init__(self, problem):
        self.problem, self.dist = problem, problem.dist
        self.ex = self.dist.executor
        self.shell = shell = problem.shell
        self.variables = problem.variables
        sb = shell.sphere
        self.nm, self.nl, self.Nr = sb.nml, sb.nl, shell.Nr          # nm: LOCAL azimuthal wavenumbers
        self.m0 = sb.m0
        self.vmap = self._pack_layout([(v.basis, v.ncomp) for v in self.variables])
        self.emap = self._pack_layout([(eq["basis"], eq["ncomp"]) for eq in problem.equations])
        self.R = max(sc for m in self.vmap for (sc, off, nr) in m) + 1
        Re = max(sc for m in self.emap for (sc, off, nr) in m) + 1
        nv = sum(nr for m in self.vmap for (sc, off, nr) in m)
        ne = sum(nr for m in self.emap for (sc, off, nr) in m)
        if nv != ne or Re != self.R:
            raise ValueError("the problem is not square: %d equation rows for %d unknowns per (m, ell)" % (ne, nv))
        self.nx, self.ny = 2 * self.nm, self.nl * self.Nr          # timestepper buffers: (R, nx, ny) elements
        self.col_valid = self._packed_valid([(v.basis, v.sig) for v in self.variables], self.vmap)
        self.row_valid = self._packed_valid([(eq["basis"], eq["lhs"].sig) for eq in problem.equations], self.emap)
        self.M_tl = self._system_termlist("M")
        self.L_tl = self._system_termlist("L")
        self.pack = MatvecPack()
        self.cx = self.M_tl.rotated or self.L_tl.rotated          # complex per-ell systems on (cos, msin) pairs
        self._assert_real_ell0()
        mk = lambda tl: self.ex.make_ell_terms(self.nm, self.nl, self.Nr, self.R, tl.terms,
                                               **(dict(rot=tl.rot) if tl.rotated else {}))
        self.M_id = self.pack.add(_Reshaped(self, mk(self.M_tl)))
        self.L_id = self.pack.add(_Reshaped(self, mk(self.L_tl)))
        self.X = self.ex.zeros((self.R, self.nx, self.ny))
        self.X4 = self.X.reshape(self.R, 2 * self.nm, self.nl, self.Nr)

    def _pack_layout(self, items):
        """items: (basis, ncomp) per variable / equation -> per item a list over its components of
        (system component, n offset, radial size)."""
        out, sc = [None] * len(items), 0
        for i, (basis, nc) in enumerate(items):           # full-radius components first
            if isinstance(basis, ShellBasis):
                out[i] = [(sc + c, 0, self.Nr) for c in range(nc)]
                sc += nc
        off = self.Nr                                      # then the single-point ones, packed along n
        for i, (basis, nc) in enumerate(items):
            if out[i] is None:
                lst = []
                for c in range(nc):
                    if off >= self.Nr:                     # open a new packed component
                        sc, off = sc + 1, 0
                    lst.append((sc - 1, off, 1))
                    off += 1
                out[i] = lst
        return out

    def _packed_valid(self, items, maps):
        valid = np.zeros((self.R, self.nl, self.Nr), dtype=bool)
        for (basis, sig), m in zip(items, maps):
            v = _valid_modes(basis, sig, self.nl, self.Nr)
            for c, (sc, off, nr) in enumerate(m):
                valid[sc, :, off:off + nr] = v[c, :, :nr]
        return valid

    def _system_termlist(self, which):
        """real blocks and rotated blocks (i A on cos + i msin: a curl) of one (co, ci) are kept apart"""
        blocks = {}
        Nr = self.Nr
        for eq, em in zip(self.problem.equations, self.emap):
            for i, t in eq[which].items():
                vm = self.vmap[i]
                for (co, ci, m), r in zip(t.terms, t.rot):
                    (so, oo, nro), (si, oi, nri) = em[co], vm[ci]
                    blk = blocks.setdefault((r, so, si), np.zeros((self.nl, Nr, Nr)))
                    blk[:, oo:oo + nro, oi:oi + nri] += m[:, :nro, :nri]
        out, rot = [], []
        for (r, co, ci), m in sorted(blocks.items()):
            m = m * self.row_valid[co][:, :, None] * self.col_valid[ci][:, None, :]
            m[np.abs(m) < 1e-12] = 0.0          # entry_cutoff of the reference's subproblem matrices (core/subsystems.py:536)
            if np.any(m != 0):
                out.append((co, ci, m))
                rot.append(r)
        return EllTermList(self.R, self.R, out, rot)

    def _dense(self, tl, ell):
        """A_r + i A_i where the list has rotated terms, a float64 matrix where it has none"""
        A = np.zeros((self.R * self.Nr, self.R * self.Nr), dtype=np.complex128 if tl.rotated else np.float64)
        for (co, ci, m), r in zip(tl.terms, tl.rot):
            A[co * self.Nr:(co + 1) * self.Nr, ci * self.Nr:(ci + 1) * self.Nr] += (1j * m[ell]) if r else m[ell]
        return A

    def _assert_real_ell0(self):
        """The curl's blocks vanish at ell = 0 (a vector has no 0 regularity component there), so the only validity hole
        of the real storage, (m, ell, part) = (0, 0, 1) (reference core/basis.py:4299-4305), stays where it is and every
        ell >= 1 system has both parts of every variable: the complex systems are exactly the reference's real-form ones."""
        for which, tl in (("M", self.M_tl), ("L", self.L_tl)):
            for (co, ci, m), r in zip(tl.terms, tl.rot):
                if r and np.any(m[0] != 0):
                    k = [i for i, em in enumerate(self.emap) if any(sc == co for (sc, off, nr) in em)][0]
                    raise ValueError("equation %d (%s): the ell = 0 system has an imaginary part in %s"
                                     % (k, self.problem.equations[k].get("string") or "no string", which))

    _dinv = None

    def _inverse_terms(self, a, b, old=None):
        """Per-ell inverse of (a M + b L) on the valid modes, formed and inverted on the device
        (executor.make_dense_inverse: M_ell and L_ell are uploaded once; a change of the timestep costs no host work),
        then applied as a term list of dense blocks.  Complex systems (self.cx): the inverse B_r + i B_i is downloaded and a
        new term list of real plus rotated blocks is built at every call -- a device-to-host copy per change of the timestep
        on this path (LBVP once; IVP only with DDH_SHELL_DENSE=1, the band path keeps everything on the device)."""
        if self._dinv is None:
            ells = range(self.nl)
            Ms = [self._dense(self.M_tl, ell) for ell in ells]
            Ls = [self._dense(self.L_tl, ell) for ell in ells]
            # ell < first local m: no local modes -> everything invalid -> a zero block
            rvs = [self.row_valid[:, ell, :].reshape(-1) & (ell >= self.m0) for ell in ells]
            cvs = [self.col_valid[:, ell, :].reshape(-1) & (ell >= self.m0) for ell in ells]
            for ell, (rv, cv) in enumerate(zip(rvs, cvs)):
                if rv.sum() != cv.sum():
                    raise ValueError("ell = %d: %d valid equation modes for %d valid variable modes" % (ell, rv.sum(), cv.sum()))
            self._dinv = self.ex.make_dense_inverse(Ms, Ls, rvs, cvs, complex_=self.cx)
        flat = self._dinv.compute(a, b)
        if self.cx:                        # B_r + i B_i: real blocks plus rotated blocks, one term list
            return _Reshaped(self, self.ex.make_ell_terms_from_dense(self.nm, self.nl, self.Nr, self.R, flat, complex_=True))
        inner = old.dev if isinstance(old, _Reshaped) else None
        return _Reshaped(self, self.ex.make_ell_terms_from_dense(self.nm, self.nl, self.Nr, self.R, flat, old=inner))

    # ---- state <-> variables -----------------------------------------------------------------------------------------
    def sync_state_to_device(self):
        for v, m in zip(self.variables, self.vmap):
            if isinstance(v, ConstField):
                if not v._host_dirty:                      # untouched since the last step: the state vector holds it
                    continue
                sc, off, nr = m[0]
                col = np.zeros((1, 2 * self.nm, self.nl, 1))
                if self.m0 == 0:                           # the (m = 0, ell = 0) slot lives on the first rank
                    col[0, 0, 0, 0] = float(v.value.reshape(-1)[0])
                self.ex.assign(self.X4[sc:sc + 1, :, :, off:off + 1], self.ex.from_host(col))
                v._host_dirty = False
                continue
            c = v.require_coeff_space()
            for comp, (sc, off, nr) in enumerate(m):
                self.ex.assign(self.X4[sc:sc + 1, :, :, off:off + nr], c[comp:comp + 1])

    def mark_state_current(self):
        for v, m in zip(self.variables, self.vmap):
            if isinstance(v, ConstField):
                sc, off, nr = m[0]

                src = self.X4[sc:sc + 1, 0:1, 0:1, off:off + 1]
                if self.dist.size > 1:
                    # every rank gets the value INSIDE the step (all ranks are here together): a later read by one rank
                    # alone -- `if rank == 0: print(tau_p['g'])` -- then needs no collective, as in the reference, where a
                    # constant field's data is replicated
                    src = self.dist.pcomm.bcast_scalar(src, self.ex, src_rank=0)

                def pull(src=src):                         # (on demand: a download per step would serialize host and device)
                    return float(np.asarray(self.ex.download(src)).reshape(-1)[0])
                v._pull = pull
                v._host_dirty = False
                continue
            # one coefficient buffer per variable for the life of the solver: a step graph (core/ivp_common.py) replays the
            # copies into the very tensors the fields hold, whichever rotation phase of a multistep scheme recorded them
            bufs = self.__dict__.setdefault("_coeff_bufs", {})
            c = bufs.get(id(v))
            if c is None:
                c = bufs[id(v)] = self.ex.empty(v._cshape())
            for comp, (sc, off, nr) in enumerate(m):
                self.ex.assign(c[comp:comp + 1], self.X4[sc:sc + 1, :, :, off:off + nr])
            v._set_device_coeff(c)

    def evaluate_F(self, out, persistent=False):
        ex = self.ex
        ex.fill_zero(out)
        out4 = out.reshape(self.R, 2 * self.nm, self.nl, self.Nr)
        for eq, m in zip(self.problem.equations, self.emap):
            F = eq["F"]
            if F is None:
                continue
            if isinstance(F, float):
                # constant right-hand side of a scalar equation (e.g. "T(r=Ri) = 1"): the ell = 0 mode, sqrt(2) amplitude
                if eq["rank"] != 0:
                    raise NotImplementedError("constant right-hand side of a tensor equation")
                sc, off, nr = m[0]
                cache = self.__dict__.setdefault("_const_F_cols", {})
                key = (id(eq), sc, off, nr)
                if key not in cache:                       # (uploaded once: no host-to-device copy inside a step)
                    col = np.zeros((1, 2 * self.nm, self.nl, nr))
                    if self.m0 == 0:
                        col[0, 0, 0, 0] = F / SphereBasis.constant_mode_value * \
                            (1.0 if isinstance(eq["basis"], SurfaceBasis) else 1.0 / self._radial_constant(eq["basis"]))
                    cache[key] = ex.from_host(col)
                ex.assign(out4[sc:sc + 1, :, :, off:off + nr], cache[key])
            else:
                c = F.eval_c()
                for comp, (sc, off, nr) in enumerate(m):
                    ex.assign(out4[sc:sc + 1, :, :, off:off + nr], c[comp:comp + 1])

    def _radial_constant(self, basis):
        from ..tools import jacobi
        return float(jacobi.polynomials(1, basis.k + basis.alpha[0], basis.k + basis.alpha[1], np.array([0.0]))[0, 0])


class _Reshaped:
    """device term list applied to the timesteppers' (R, nx, ny) buffers"""

    def __init__(self, solver, dev):
        self.solver, self.dev = solver, dev

    def apply(self, x, y):
        s = self.solver
        shape = (s.R, 2 * s.nm, s.nl, s.Nr)
        self.dev.apply(x.reshape(shape), y.reshape(shape))


class ShellBoundaryValueSolver(ShellSolverBase):
    def __init__(self, problem, **kw):
        super().__init__(problem)
        if self.M_tl.terms:
            raise ValueError("LBVP equations cannot contain time derivatives")
        self._inv = None

    def solve(self):
        if self._inv is None:
            self._inv = self._inverse_terms(0.0, 1.0)
        F = self.ex.zeros((self.R, self.nx, self.ny))
        self.evaluate_F(F)
        self._inv.apply(F, self.X)
        self.mark_state_current()


class ShellInitialValueSolver(LUSlotSolver, ShellSolverBase):
    """IMEX timestepping of M.dt(X) + L.X = F in a shell with the shared schemes of core/timesteppers.py and the shared
    life cycle and LU slots of core/ivp_common.py (stop conditions incl. stop_wall_time, world clocks, evolve)."""

    def __init__(self, problem, timestepper, enforce_real_cadence=100, warmup_iterations=10, **kw):
        t0 = _time.time()
        ShellSolverBase.__init__(self, problem)
        self._init_ivp(t0, timestepper, enforce_real_cadence, warmup_iterations)
        self.total_modes = int(self.col_valid.sum()) * 2 * self.nm

    def _hermitian_round_trip(self, f):
        """the state makes a round trip through the dealiased grid (core/solvers.py:675-681)"""
        if isinstance(f, ShellField):
            f.require_grid_space(f.basis.dealias)
            f.require_coeff_space()

    # ---- LHS systems: band LU per ell where the matrices allow it, dense inverses for the rest ---------------------------
    _band = None                 # None: undecided; False: dense inverses only; dict: the band path

    def _band_setup(self):
        """Decide once how a M + b L is solved.  core/ellband.py finds the permutation / recombination that makes the
        per-ell matrices narrow bands; the groups it covers are factorized and swept by csrc/ddh_ellband.hip, the others
        (the ell = 0 system with its dense gauge row) keep a dense inverse.  DDH_SHELL_DENSE=1: dense inverses for all."""
        if self._band is None:
            self._band = False
            import os
            if hasattr(self.ex, "make_ell_band") and os.environ.get("DDH_SHELL_DENSE", "0") != "1":
                from .ellband import EllBandPlan
                prow = sorted({sc for m in self.emap for (sc, off, nr) in m if nr != self.Nr})
                pcol = sorted({sc for m in self.vmap for (sc, off, nr) in m if nr != self.Nr})
                ells = [ell for ell in range(self.nl) if ell >= self.m0]
                plan = EllBandPlan(lambda g: self._dense(self.M_tl, g), lambda g: self._dense(self.L_tl, g),
                                   [self.row_valid[:, g, :] for g in range(self.nl)],
                                   [self.col_valid[:, g, :] for g in range(self.nl)], prow, pcol, self.Nr, ells)
                if plan.per and plan.nbc <= 8 and plan.mp <= 16:
                    limit = [2 * min(max(g - self.m0 + 1, 0), self.nm) for g in range(self.nl)]
                    dev = self.ex.make_ell_band(plan, self.R, 2 * self.nm, self.nl, self.Nr, limit)
                    dinv = None
                    if plan.dense_groups:
                        gs = plan.dense_groups
                        dinv = self.ex.make_dense_inverse([self._dense(self.M_tl, g) for g in gs],
                                                          [self._dense(self.L_tl, g) for g in gs],
                                                          [self.row_valid[:, g, :].reshape(-1) for g in gs],
                                                          [self.col_valid[:, g, :].reshape(-1) for g in gs], complex_=self.cx)
                    self._band = dict(plan=plan, dev=dev, dinv=dinv)
                    logger.info("shell LHS: band LU for %d of %d ell (kl %d, ku %d); dense inverse for ell in %s" % (
                        len(plan.per), len(ells), plan.kl, plan.ku, plan.dense_groups))
        return self._band

    def factor(self, a, b, reuse=-1):
        # (deliberate: reuse >= 0 alone; the sphere also checks that the slot exists)
        old = self._lus[reuse] if (reuse is not None and reuse >= 0) else None
        band = self._band_setup()
        if band:
            index = band["dev"].factor(a, b, index=old["index"] if isinstance(old, dict) else None)
            dense = None
            if band["dinv"] is not None:
                flat = band["dinv"].compute(a, b)
                dense = old["dense"] if isinstance(old, dict) else self.ex.empty(tuple(flat.shape))
                self.ex.assign(dense, flat)
            inv = dict(index=index, dense=dense)
        else:
            inv = self._inverse_terms(a, b, old=old)
        return self._store_lu(inv, a, b, reuse)

    def solve(self, lu, rhs, x):
        inv = self._lus[lu]
        if isinstance(inv, dict):
            band = self._band
            self.ex.fill_zero(x)
            band["dev"].solve(inv["index"], rhs, x)
            if inv["dense"] is not None:
                shape = (self.R, 2 * self.nm, self.nl, self.Nr)
                n2 = (self.R * self.Nr) ** 2
                for k, g in enumerate(band["plan"].dense_groups):
                    if self.cx:
                        self.ex.dense_group_solve(inv["dense"][2 * k * n2:2 * (k + 1) * n2], rhs.reshape(shape),
                                                  x.reshape(shape), g, complex_=True)
                        continue
                    self.ex.dense_group_solve(inv["dense"][k * n2:(k + 1) * n2], rhs.reshape(shape), x.reshape(shape), g)
        else:
            inv.apply(rhs, x)
        self._probe_solve(lu, rhs, x)


# ==================================================================================================
# products with radial non-constant coefficients (NCCs) on the LHS
# ==================================================================================================

def gamma_regularity(rank_a, rank_b, ell_a, ell_b, ell_c, contract=False):
    """Gamma[alpha, beta, gamma]: regularity components of a product, out_gamma = sum Gamma a_alpha b_beta
    (Product.Gamma, core/arithmetic.py:560-580: the coordinate-component product tensor carried through the spin
    intertwiner U and the regularity intertwiners Q(ell) of the three operands).  contract: DotProduct of the last
    index of a with the first of b (GammaCoord :649-664), else the tensor product (MultiplyFields)."""
    ia_list = reg_indices(rank_a)
    ib_list = reg_indices(rank_b)
    rank_c = rank_a + rank_b - (2 if contract else 0)
    ic_list = reg_indices(rank_c)
    G = np.zeros((len(ia_list), len(ib_list), len(ic_list)), dtype=complex)
    for ia, a in enumerate(ia_list):
        for ib, b in enumerate(ib_list):
            if contract:
                if a[-1] != b[0]:
                    continue
                c = tuple(a[:-1]) + tuple(b[1:])
            else:
                c = tuple(a) + tuple(b)
            G[ia, ib, ic_list.index(c)] = 1.0
    # coordinate -> spin components
    UA = np.conj(SphericalCoordinates.U_forward(rank_a))
    UB = np.conj(SphericalCoordinates.U_forward(rank_b))
    UC = SphericalCoordinates.U_forward(rank_c)
    G = np.einsum("ai,bj,ck,ijk->abc", UA, UB, UC, G)
    # spin -> regularity components
    QA = sph.intertwiner(ell_a, rank_a).T if rank_a else np.eye(1)
    QB = sph.intertwiner(ell_b, rank_b).T if rank_b else np.eye(1)
    QC = sph.intertwiner(ell_c, rank_c).T if rank_c else np.eye(1)
    return np.einsum("ai,bj,ck,ijk->abc", QA, QB, QC, G)
