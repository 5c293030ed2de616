"""
Symbol term list of a triply periodic problem (three RealFourier axes) for the matrix-free modal solve.

With a Fourier pencil axis every matrix along the pencil is a function of the 2 x 2 generator J = [[0, -1], [1, 0]] of
d/dz on a (cos, msin) pair: Z = blockdiag_m (a_m I + b_m J), and a_m + i b_m = c (i kz_m)^ez is its symbol on the
combination cos_z + i msin_z.  `ModalPlan` holds, for the rc tensor-component rows of the variables, the entries

    A[i, j] += (a or b) * coef * kx^ex ky^ey kz^ez [mx == 0]^dx [my == 0]^dy [mz == 0]^dz

that ddh_pencil_solve_modal (csrc/ddh_modal.hip) assembles and eliminates per Fourier mode; `dense` is the same assembly on
the host (tests, tools).  The reference builds these matrices numerically per subproblem (core/subsystems.py:497-596).
"""

import numpy as np

RC_MAX = 8
EXP_MAX = 4


class ModalPlan:
    def __init__(self, rc, nx, ny, nz, kx, ky, kz, rhs_row, x_row, axes, ti, tj, coef, ex, ey, ez, flags,
                 nrows_rhs, nrows_x, mx_offset=0):
        self.rc, self.nx, self.ny, self.nz = int(rc), int(nx), int(ny), int(nz)
        self.kx, self.ky, self.kz = (np.asarray(k, dtype=np.float64) for k in (kx, ky, kz))
        self.rhs_row = np.asarray(rhs_row, dtype=np.int32)
        self.x_row = np.asarray(x_row, dtype=np.int32)
        self.axes = np.asarray(axes, dtype=np.uint8)
        self.ti, self.tj = np.asarray(ti, dtype=np.int32), np.asarray(tj, dtype=np.int32)
        self.coef = np.asarray(coef, dtype=np.complex128)
        self.ex, self.ey, self.ez, self.flags = (np.asarray(v, dtype=np.uint8) for v in (ex, ey, ez, flags))
        self.nrows_rhs, self.nrows_x, self.mx_offset = int(nrows_rhs), int(nrows_x), int(mx_offset)

    def valid(self, mx, my, mz):
        """bool [rc]: which component rows have a mode in the cell (mx: the global index)"""
        ax = self.axes.astype(int)
        return ((mx == 0) | ((ax & 1) != 0)) & ((my == 0) | ((ax & 2) != 0)) & ((mz == 0) | ((ax & 4) != 0))

    def dense(self, a, b, mx, my, mz, sx=1, sz=1, dtype=np.complex128):
        """(a M + b L)(sx kx, ky, sz kz) of the local cell (mx, my, mz), identity rows / columns for the components
        without a mode there; `dtype` = numpy.clongdouble assembles in extended precision."""
        real = np.longdouble if dtype == np.clongdouble else np.float64
        kx, ky, kz = real(sx) * real(self.kx[mx]), real(self.ky[my]), real(sz) * real(self.kz[mz])
        gmx = mx + self.mx_offset
        A = np.zeros((self.rc, self.rc), dtype=dtype)
        for t in range(self.ti.size):
            f = int(self.flags[t])
            if (f & 1 and gmx != 0) or (f & 2 and my != 0) or (f & 4 and mz != 0):
                continue
            w = (real(b) if f & 8 else real(a)) * kx ** int(self.ex[t]) * ky ** int(self.ey[t]) * kz ** int(self.ez[t])
            A[self.ti[t], self.tj[t]] += dtype(self.coef[t]) * w
        v = self.valid(gmx, my, mz)
        A[~v, :] = 0
        A[:, ~v] = 0
        A[~v, ~v] = 1
        return A


def z_symbol(Z, kz, tol=1e-12):
    """(c, ez, dz) with Z == c (d/dz)^ez along a RealFourier pencil axis (dz = 1: an embedding of / a projection on the
    mean mode, an entry that only exists at mz = 0), None for a zero matrix; raises when Z has no such form."""
    Z = np.asarray(Z.todense() if hasattr(Z, "todense") else Z)
    if not np.any(Z):
        return None
    nzo, nzi = Z.shape
    if nzo == 1 or nzi == 1:
        c = Z[0, 0]
        rest = Z.copy()
        rest[0, 0] = 0
        if np.any(rest):
            raise NotImplementedError("a matrix along the Fourier pencil axis that is no function of d/dz")
        return complex(c), 0, 1
    n = nzo // 2
    if nzo != nzi or nzo != 2 * kz.size:
        raise NotImplementedError("a matrix along the Fourier pencil axis that is no function of d/dz")
    m = np.arange(1, n)
    s = Z[2 * m, 2 * m] + 1j * Z[2 * m + 1, 2 * m]
    blocks = np.zeros_like(Z)
    blocks[2 * m, 2 * m] = blocks[2 * m + 1, 2 * m + 1] = Z[2 * m, 2 * m]
    blocks[2 * m + 1, 2 * m] = Z[2 * m + 1, 2 * m]
    blocks[2 * m, 2 * m + 1] = -Z[2 * m + 1, 2 * m]
    blocks[0, 0] = Z[0, 0]
    blocks[1, 1] = Z[1, 1]                      # (the msin slot of kz = 0 holds no mode: whatever stands there)
    scale = np.abs(Z).max()
    if np.abs(Z - blocks).max() > tol * scale:
        raise NotImplementedError("a matrix along the Fourier pencil axis that is no function of d/dz")
    s0 = Z[0, 0]
    if n == 1:
        return complex(s0), 0, 0
    for ez in range(EXP_MAX + 1):
        c = s / (1j * kz[m]) ** ez
        if np.abs(c - c[0]).max() <= tol * max(np.abs(c).max(), 1e-300) and \
                abs(s0 - (c[0] if ez == 0 else 0.0)) <= tol * max(abs(c[0]), 1e-300):
            return complex(c[0] * (1j) ** ez), ez, 0
    raise NotImplementedError("a matrix along the Fourier pencil axis that is no monomial in d/dz of degree <= %d" % EXP_MAX)


def plan_from_solver(solver, cutoff=1e-12):
    """ModalPlan of a solver whose pencil axis is a RealFourier axis, or (None, reason)."""
    dist = solver.dist
    pf = sorted(getattr(dist, "_pencil_fourier", ()))
    if not pf:
        return None, "no Fourier pencil axis"
    if solver.nf != 2 or solver.P_id is not None or solver.eq_T is not None:
        return None, "not a triply periodic problem"
    zax = pf[0]

    def comps(infos, domain_of):
        out = []
        for i in infos:
            hasz = domain_of(i).by_axis[zax] is not None
            for c in range(i["ncomp"]):
                out.append((i["row0"] + c * i["nz"], (i["bits"] & 3) | (4 if hasz else 0)))
        return out

    eqs = comps(solver.eq_info, lambda i: i["eq"]["domain"])
    vrs = comps(solver.var_info, lambda i: i["field"].domain)
    rc = len(eqs)
    if rc != len(vrs):
        return None, "equation and variable components do not balance"
    if rc > RC_MAX:
        return None, "%d component rows, the modal kernel takes %d" % (rc, RC_MAX)
    # the k-th system row and column must have modes in the same cells: pair every equation component with a variable
    # component of the same axes
    colpos, used = {}, set()
    order = []
    for k, (_, ax) in enumerate(eqs):
        hit = [j for j, (_, axv) in enumerate(vrs) if axv == ax and j not in used]
        if not hit:
            return None, "equation and variable components exist for different modes"
        used.add(hit[0])
        colpos[hit[0]] = k
        order.append(hit[0])
    basis = next(v["field"].domain.by_axis[zax] for v in solver.var_info if v["field"].domain.by_axis[zax] is not None)
    kz = basis.mode_wavenumbers
    eq_base, n = {}, 0
    for i in solver.eq_info:
        eq_base[id(i)] = n
        n += i["ncomp"]
    var_base, n = {}, 0
    for i in solver.var_info:
        var_base[id(i["field"])] = n
        n += i["ncomp"]
    ti, tj, coef, exs, eys, ezs, fl = [], [], [], [], [], [], []
    for which in ("M", "L"):
        for einfo in solver.eq_info:
            le = einfo["eq"][which]
            efx, efy = solver._flags(einfo["eq"]["domain"])
            for leaf, terms in le.leaves.items():
                vfx, vfy = solver._flags(leaf.domain)
                for t in terms:
                    try:
                        sym = z_symbol(t.Z, kz)
                    except NotImplementedError as e:
                        return None, str(e)
                    if sym is None:
                        continue
                    c, ez, dz = sym
                    c = c * t.coef
                    if abs(c) <= cutoff:
                        continue
                    if t.ex > EXP_MAX or t.ey > EXP_MAX:
                        return None, "wavenumber exponent above %d" % EXP_MAX
                    ti.append(eq_base[id(einfo)] + t.co)
                    tj.append(colpos[var_base[id(leaf)] + t.ci])
                    coef.append(c)
                    exs.append(t.ex)
                    eys.append(t.ey)
                    ezs.append(ez)
                    fl.append((1 if (t.dx or efx or vfx) else 0) | (2 if (t.dy or efy or vfy) else 0) | (4 if dz else 0)
                              | (8 if which == "L" else 0))
    nf, nx, ny, kx, ky = solver.evaluator_core.geom()
    return ModalPlan(rc, nx, ny, basis.coeff_size, kx, ky, kz, [r for r, _ in eqs], [vrs[j][0] for j in order],
                     [ax for _, ax in eqs], ti, tj, coef, exs, eys, ezs, fl, solver.R, solver.R, dist._mx_offset), None
