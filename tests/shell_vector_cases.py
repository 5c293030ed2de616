"""Cases of the shell cross product and curl (tests/test_shell_vector_ops.py, tests/test_gpu_shell_vector_ops.py,
tools/make_golden_shell_vector_ops.py -> tests/golden/shell_vector_ops.npz), and the kernel-level cases that pin the
banded kernel of ddh_ell_terms_apply (csrc/ddh_sphere.hip, both instances) at the edges of its launch shape.

Launch shape of the kernel: one workgroup = 8 consecutive (m, part) slots of one ell; 64 / 128 / 256 threads along the
output radial index for nr <= 64 / <= 255 / >= 256; 4 output components at a time.  Hence the edges: 2 nm = 8 | 10,
nr = 64 | 65 and 255 | 256, ncomp_out = 4 | 5 (the curl itself has 3), and ncomp_in * nr * 64 bytes of LDS on either side
of 64 KiB, above which the creation opts in to a larger allocation: nr = 341 | 342 for three input components.  One case
has the shape of the per-ell GEMM path (full matrices, sizes that tile it): its rotated terms keep it on the banded kernel."""
import numpy as np

RADII = (0.7, 1.9)
DEALIAS = 3 / 2

# (a) curl(u), curl(curl(u)), div(curl(u)) of a full-spectrum vector field, ShellBasis shapes (Nphi, Ntheta, Nr)
CURL_SHAPES = [
    (8, 4, 6),        # 2 nm = 8: exactly one slot group; ell <= 3, fewer radii than a wavefront
    (32, 16, 12),
    (24, 12, 17),     # odd Nr
    (20, 10, 9),      # 2 nm = 20: the last slot group is half empty; ell range no multiple of any tile
    (8, 4, 64),       # last size on 64 threads per component
    (8, 4, 65),       # first size on 128 threads
]
# (b) cross(a, b): two full-spectrum vectors, a radial, a = ez
CROSS_SHAPES = [(32, 16, 12), (8, 4, 6)]

CURL_TASKS = ("curl", "curlcurl", "divcurl")
CROSS_TASKS = ("cross_uv", "cross_rad", "cross_ez", "sum_products")


def tag(shape):
    return "%dx%dx%d" % tuple(shape)


def build(d3, shape, dist_kw=None):
    coords = d3.SphericalCoordinates("phi", "theta", "r")
    dist = d3.Distributor(coords, dtype=np.float64, **(dist_kw or {}))
    shell = d3.ShellBasis(coords, shape=shape, radii=RADII, dealias=DEALIAS, dtype=np.float64)
    u = dist.VectorField(coords, name="u", bases=shell)
    v = dist.VectorField(coords, name="v", bases=shell)
    return coords, dist, shell, u, v


def radial_vector(d3, coords, dist, shell):
    """a(r) = (1 + r^2 / 2) e_r: a smooth vector field that depends on r alone has no angular components"""
    a = dist.VectorField(coords, bases=shell.radial_basis)
    r = dist.local_grids(shell)[2]
    a["g"][2] = 1 + 0.5 * r ** 2
    return a


def rotation_axis(d3, coords, dist, shell):
    ez = dist.VectorField(coords, bases=shell.meridional_basis)
    phi, theta, r = dist.local_grids(shell)
    ez["g"][1] = -np.sin(theta)
    ez["g"][2] = np.cos(theta)
    return ez


def curl_tasks(d3, u):
    return dict(curl=d3.curl(u), curlcurl=d3.curl(d3.curl(u)), divcurl=d3.div(d3.curl(u)))


def cross_tasks(d3, coords, dist, shell, u, v):
    # sum_products: two operands formed on the grid, in different bases (k = 0 and k = 1).  The reference adds them on the
    # grid and transforms the sum once, in the k = 1 basis (AddFields / Convert.operate); transforming each product on its
    # own and converting with the E matrices differs from that at truncation level
    return dict(cross_uv=d3.cross(u, v), cross_rad=d3.cross(radial_vector(d3, coords, dist, shell), u),
                cross_ez=d3.cross(rotation_axis(d3, coords, dist, shell), u),
                sum_products=d3.cross(u, v) + d3.cross(v, d3.curl(u)))


# ---- kernel-level cases: (label, nm, nl, nr, ncomp_out, ncomp_in, bandwidth, holes)
# holes: slots whose slot_map is -1 besides ell < m (and the (m, ell, part) = (0, 0, 1) slot, always a hole here)
KERNEL_CASES = [
    ("slots8", 4, 5, 7, 3, 3, 2, ()),
    ("slots10", 5, 6, 7, 3, 3, 2, ((3, 4),)),
    ("nr64", 2, 3, 64, 3, 3, 3, ()),
    ("nr65", 2, 3, 65, 3, 3, 3, ((2, 2),)),
    ("nr255", 1, 2, 255, 3, 3, 2, ()),
    ("nr256", 1, 2, 256, 3, 3, 2, ()),
    ("nr341", 1, 2, 341, 3, 3, 2, ()),
    ("nr342", 1, 2, 342, 3, 3, 2, ()),
    ("co4", 3, 4, 9, 4, 3, 9, ()),
    ("co5_mixed_ids", 3, 4, 9, 5, 2, 2, ((4, 3),)),
    ("gemm_shaped", 4, 9, 64, 2, 3, 64, ()),
]


def kernel_case(label):
    """-> nm, nl, nr, nco, terms [(co, ci, mats [nmat][nr][nr])], rot, slot_map, x (NaN in every slot without a mode)"""
    (_, nm, nl, nr, nco, nci, bw, holes), = [c for c in KERNEL_CASES if c[0] == label]
    rng = np.random.default_rng(sum(map(ord, label)))
    nmat = nl + (2 if "mixed" in label else 0)
    i1, ell = np.indices((2 * nm, nl))
    slot_map = np.where(i1 // 2 <= ell, ell, -1).astype(np.int32)
    if "mixed" in label:                      # slots of one group with different matrices, a pair with two ids included
        slot_map[2, 2] = nl
        slot_map[3, 3] = nl + 1
    slot_map[1, 0] = -1
    for (a, b) in holes:
        slot_map[a, b] = -1
    band = np.abs(np.subtract.outer(np.arange(nr), np.arange(nr))) <= bw
    terms, rot = [], []
    for co in range(nco):
        for ci in range(nci):
            for r in (0, 1):
                if rng.random() < 0.6:
                    m = rng.standard_normal((nmat, nr, nr)) * band
                    m[:, nr // 2, :] = 0.0                         # an empty row
                    terms.append((co, ci, m))
                    rot.append(r)
    x = rng.standard_normal((nci, 2 * nm, nl, nr))
    x[:, slot_map < 0, :] = np.nan
    return nm, nl, nr, nco, terms, rot, slot_map, x


def kernel_reference(nm, nl, nr, nco, terms, rot, slot_map, x):
    """longdouble product of the same term list -> (y, sum |a| |x|, products summed per output element)"""
    LD = np.longdouble
    live = slot_map >= 0
    xs = np.where(np.isnan(x), 0.0, x).astype(LD)
    y = np.zeros((nco, 2 * nm, nl, nr), LD)
    mag = np.zeros_like(y)
    cnt = np.zeros(y.shape, np.int64)
    for (co, ci, mats), r in zip(terms, rot):
        A = mats[np.where(live, slot_map, 0)].astype(LD)              # [2 nm][nl][nr][nr]: the OUTPUT slot's matrix
        src = xs[ci]
        if r:
            src = np.empty_like(xs[ci])
            src[0::2] = -xs[ci][1::2]
            src[1::2] = xs[ci][0::2]
        y[co] += np.einsum("alij,alj->ali", A, src)
        mag[co] += np.einsum("alij,alj->ali", np.abs(A), np.abs(src))
        cnt[co] += np.count_nonzero(A, axis=3)
    y *= live[None, :, :, None]
    return y, mag, cnt


def with_rot(executor_cls):
    """The NumPy oracle executor with rotated terms: the real executor's contraction applied to the part-swapped input
    (an independent statement of the convention: i (c + i s) = -s + i c)."""
    class _Cx(executor_cls):
        def make_ell_terms(self, nm, nl, nr, ncomp_out, terms, slot_map=None, rot=None):
            base = super().make_ell_terms
            if rot is None or not any(rot):
                return base(nm, nl, nr, ncomp_out, terms, slot_map)
            real = base(nm, nl, nr, ncomp_out, [t for t, r in zip(terms, rot) if not r], slot_map)
            imag = base(nm, nl, nr, ncomp_out, [t for t, r in zip(terms, rot) if r], slot_map)
            sm = None if slot_map is None else np.asarray(slot_map)

            class _Terms:
                def apply(self_, x, y):
                    x = np.asarray(x)
                    if sm is not None:
                        x = np.where((sm >= 0)[None, :, :, None], x, 0.0)
                    ix = np.empty_like(x)
                    ix[:, 0::2] = -x[:, 1::2]
                    ix[:, 1::2] = x[:, 0::2]
                    y2 = np.empty_like(y)
                    real.apply(x, y)
                    imag.apply(ix, y2)
                    y += y2
            return _Terms()
    return _Cx()


# (c) rotating convection: the shell convection problem of tests/problems.py::shell_convection (the reference's
# examples/ivp_shell_convection) with the Coriolis force - cross(ez, u) / Ekman on the right-hand side
IVP_SHAPE, IVP_STEPS, IVP_DT, EKMAN = (32, 16, 16), 3, 0.02, 1e-2


def rotating_convection(d3, shape=IVP_SHAPE, dist_kw=None, ekman=EKMAN, rotate=True):
    Ri, Ro = 14, 15
    Rayleigh, Prandtl = 3500, 1
    coords = d3.SphericalCoordinates('phi', 'theta', 'r')
    dist = d3.Distributor(coords, dtype=np.float64, **(dist_kw or {}))
    shell = d3.ShellBasis(coords, shape=shape, radii=(Ri, Ro), dealias=DEALIAS, dtype=np.float64)
    sphere = shell.outer_surface
    p = dist.Field(name='p', bases=shell)
    b = dist.Field(name='b', bases=shell)
    u = dist.VectorField(coords, name='u', bases=shell)
    tau_p = dist.Field(name='tau_p')
    tau_b1 = dist.Field(name='tau_b1', bases=sphere)
    tau_b2 = dist.Field(name='tau_b2', bases=sphere)
    tau_u1 = dist.VectorField(coords, name='tau_u1', bases=sphere)
    tau_u2 = dist.VectorField(coords, name='tau_u2', bases=sphere)
    kappa = (Rayleigh * Prandtl) ** (-1 / 2)
    nu = (Rayleigh / Prandtl) ** (-1 / 2)
    Ekman = ekman
    phi, theta, r = dist.local_grids(shell)
    er = dist.VectorField(coords, bases=shell.radial_basis)
    er['g'][2] = 1
    rvec = dist.VectorField(coords, bases=shell.radial_basis)
    rvec['g'][2] = r
    ez = dist.VectorField(coords, bases=shell.meridional_basis)
    ez['g'][1] = -np.sin(theta)
    ez['g'][2] = np.cos(theta)
    lift_basis = shell.derivative_basis(1)
    lift = lambda A: d3.Lift(A, lift_basis, -1)
    grad_u = d3.grad(u) + rvec * lift(tau_u1)
    grad_b = d3.grad(b) + rvec * lift(tau_b1)
    cross = d3.cross
    problem = d3.IVP([p, b, u, tau_p, tau_b1, tau_b2, tau_u1, tau_u2], namespace=locals())
    problem.add_equation("trace(grad_u) + tau_p = 0")
    problem.add_equation("dt(b) - kappa*div(grad_b) + lift(tau_b2) = - u@grad(b)")
    if rotate:
        problem.add_equation("dt(u) - nu*div(grad_u) + grad(p) - b*er + lift(tau_u2) = - u@grad(u) - cross(ez, u)/Ekman")
    else:
        problem.add_equation("dt(u) - nu*div(grad_u) + grad(p) - b*er + lift(tau_u2) = - u@grad(u)")
    problem.add_equation("b(r=Ri) = 1")
    problem.add_equation("u(r=Ri) = 0")
    problem.add_equation("b(r=Ro) = 0")
    problem.add_equation("u(r=Ro) = 0")
    problem.add_equation("integ(p) = 0")
    solver = problem.build_solver(d3.SBDF2)
    b.fill_random('g', seed=42, distribution='normal', scale=1e-3)
    b['g'] *= (r - Ri) * (Ro - r)
    b['g'] += (Ri - Ri * Ro / r) / (Ri - Ro)
    return solver, dict(p=p, b=b, u=u, tau_p=tau_p, tau_b1=tau_b1, tau_b2=tau_b2, tau_u1=tau_u1, tau_u2=tau_u2)


def run_rotating_convection(d3, dist_kw=None, shape=IVP_SHAPE, steps=IVP_STEPS):
    """-> end state of every variable ('c'), the task curl(u) ('c') and the flow property sqrt(curl(u)@curl(u)) (its coefficients:
    the grid values as the forward transform sees them) after the last step"""
    solver, f = rotating_convection(d3, shape, dist_kw)
    for _ in range(steps):
        solver.step(IVP_DT)
    res = {}
    for k, fld in f.items():
        if hasattr(fld, "change_scales"):
            fld.change_scales(1)
        res[k] = np.array(fld['c'] if k != "tau_p" else fld['g'])
    w = d3.curl(f["u"]).evaluate()
    w.change_scales(1)
    res["curl_u"] = np.array(w['c'])
    en = np.sqrt(d3.curl(f["u"]) @ d3.curl(f["u"])).evaluate()
    en.change_scales(1)
    res["enstrophy_sqrt"] = np.array(en['c'])
    return solver, res
