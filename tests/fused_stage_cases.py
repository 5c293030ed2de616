"""Cases, inputs and references of the fused grid stage (ddh_rfft_bilinear_fused) away from the 3/2 rule, shared by
tests/test_fused_stage_host.py (CPU) and tests/test_gpu_fused_stage.py.

Two references.  The double-precision oracle (NumpyExecutor.rfft_bilinear_fused: pocketfft transforms) is applied to every
line of a case.  A longdouble restatement by matrices, independent of any FFT call, is applied to a subset of lines: the
synthesis matrix [N][M] of the (cos, -sin) coefficient layout with the derivative at load folded in, the pointwise term
table on the plan's own N-point grid, and the analysis matrix [M][N] with the truncation rule of oracle/np_transforms.py
(kmax, the empty -sin slot of k = 0, zero slots above kmax).  Products of an under-dealiased line (N <= 3 kmax) alias on
that grid in both references; a kernel that works on a wider internal grid loses the aliasing and misses both.

Each case names the selection it pins: (internal grid, kernel family, C, NT, lines per wave), family 0 = wave-per-line
second generation, 1 = first generation, 2 = workgroup-per-line-pair, as ddh_rfft_fused_plan_info reports them.

Also the end-to-end problem of the under-dealiased stage: a Rayleigh-Benard box whose y basis has 128 modes on 128 points
(dealias 1), stepped by the reference (tools/make_golden_fused_dealias1.py -> tests/golden/fused_dealias1.npz), by the
oracle executor and on the device."""
import collections

import numpy as np

LD = np.longdouble
PI = LD(4) * np.arctan(LD(1))
TOL = 1e-12                   # the standing bound of the transforms (tests/test_gpu_transforms.py), rel-L2
ORACLE_TOL = 1e-13            # the oracle against the longdouble reference, per line: a tenth of the kernel's bound
GUARD = 64                    # doubles behind every output array that must come back untouched
WAVES = 4                     # lines (wavefronts) per workgroup of the wave kernels, one line per wave and pass
SUBSET_RANDOM = 32
GW2, GW, WG = 0, 1, 2
WAVE_SIZES = (256, 384, 512, 768, 1024)


def kmax(N, M):
    return min((N - 1) // 2, (M - 1) // 2)


def internal_grid(N, M):
    """The selection rule: the own grid where it has a wave kernel or is under-dealiased, else the smallest wave size that
    is at least N and free of aliasing for the line's modes."""
    K = kmax(N, M)
    if N in WAVE_SIZES or N <= 3 * K:
        return N
    for Np in WAVE_SIZES:
        if Np >= N and Np > 3 * K:
            return Np
    return N


def lines_per_wave(nlines):
    return min(8, max(1, nlines // (WAVES * 2048)))


# ---- term tables ------------------------------------------------------------------------------------------------------
# name -> (na, nb, nc, terms, a_dscale, b_dscale); terms (ic, ia, ib, coefficient).  "grad": the u.grad(b) + u.grad(u)
# shape of the existing kernel test (three register operands, 3 + 9 line operands, 1 + 3 results, every third line operand
# and one register operand differentiated at load); "one": a single product whose line operand is differentiated.
def _grad_table():
    rng = np.random.default_rng(20)
    na, terms, ob, bb = 3, [], 0, 0
    for nb, nc in ((3, 1), (9, 3)):
        for c in range(nc):
            for j in range(na):
                terms.append((ob + c, j, bb + (c * na + j) % nb, float(rng.standard_normal())))
        ob += nc
        bb += nb
    return na, bb, ob, terms, [0.0, 0.6, 0.0], [(1.7 if i % 3 == 1 else 0.0) for i in range(bb)]


TABLES = {"grad": _grad_table(), "one": (1, 1, 1, [(0, 0, 0, -0.75)], [0.0], [1.7])}

Case = collections.namedtuple("Case", "N M nlines table internal family C NT lpw what")


def _case(N, M, nlines, table, internal, family, C=0, NT=0, what=""):
    lpw = lines_per_wave(nlines) if family != WG else 0
    return Case(N, M, nlines, table, internal, family, C, NT, lpw, what)


CASES = []
# under-dealiased and no wave kernel of the own size: the own grid, workgroup kernel (a wider grid removes the aliasing)
for _N, _M in ((128, 128), (192, 160), (96, 96), (128, 100), (320, 256), (640, 512)):
    for _t in ("grad", "one"):
        CASES.append(_case(_N, _M, 5, _t, _N, WG, what="under-dealiased, own grid"))
# alias-free own grid without a wave kernel: widened, first generation, narrow
for _N, _M, _Np, _C, _NT in ((192, 128, 256, 2, 2), (128, 84, 256, 2, 2), (320, 212, 384, 3, 2), (640, 426, 768, 6, 4),
                             (896, 596, 1024, 8, 6)):
    for _n, _t in ((5, "grad"), (6, "grad"), (5, "one")):
        CASES.append(_case(_N, _M, _n, _t, _Np, GW, _C, _NT, "widened, narrow"))
# full-spectrum instantiations <C, C>
for _N, _M, _n, _C in ((512, 512, 7, 4), (512, 400, 7, 4), (1024, 1024, 3, 8), (1024, 800, 3, 8)):
    for _t in ("grad", "one"):
        CASES.append(_case(_N, _M, _n, _t, _N, GW, _C, _C, "full spectrum <%d, %d>" % (_C, _C)))
for _t in ("grad", "one"):
    CASES.append(_case(256, 256, 9, _t, 256, GW, 2, 2, "C = 2 at full spectrum"))
# either side of K + 1 == 64 NT32 (the second generation takes the equality: (384, 256), (768, 512))
for _N, _M, _C, _NT in ((384, 258, 3, 3), (384, 254, 3, 2), (768, 514, 6, 6), (768, 510, 6, 4)):
    for _t in ("grad", "one"):
        CASES.append(_case(_N, _M, 5, _t, _N, GW, _C, _NT, "beside K + 1 == 64 NT32"))
for _N, _M, _C, _NT in ((1024, 684, 8, 6), (256, 172, 2, 2)):
    for _t in ("grad", "one"):
        CASES.append(_case(_N, _M, 3, _t, _N, GW, _C, _NT, "narrow, last alias-free M"))
# lines per wave 1 -> 2 -> 8, ragged last workgroup
for _n in (8191, 16383, 16384, 16387, 65541):
    CASES.append(_case(256, 170, _n, "one", 256, GW, 2, 2, "lines per wave"))
CASES.append(_case(384, 256, 16387, "one", 384, GW2, 3, 2, "lines per wave, second generation"))
# odd line counts.  (60, 40) and (24, 16) are alias-free: the stage widens them to 256 points (first generation), where the
# odd counts leave waves of the last workgroup without a line; (60, 60) and (24, 24) are under-dealiased and stay on the
# workgroup kernel, where the last line of an odd count has no partner
for _N, _M, _Np, _fam, _C in ((60, 40, 256, GW, 2), (24, 16, 256, GW, 2), (60, 60, 60, WG, 0), (24, 24, 24, WG, 0)):
    for _n, _t in ((1, "grad"), (2, "grad"), (131, "grad"), (1, "one"), (2, "one"), (131, "one")):
        CASES.append(_case(_N, _M, _n, _t, _Np, _fam, _C, _C, "odd line counts"))


def case_id(c):
    return "%dx%d-%d-%s" % (c.N, c.M, c.nlines, c.table)


# ---- inputs -----------------------------------------------------------------------------------------------------------
def inputs(c):
    """a [na][nlines][M], b [nb][nlines][M]: seeded normal deviates, the -sin slot of k = 0 empty."""
    na, nb = TABLES[c.table][:2]
    rng = np.random.default_rng(c.N * 1000003 + c.M * 1009 + c.nlines * 7 + na)
    a = rng.standard_normal((na, c.nlines, c.M))
    b = rng.standard_normal((nb, c.nlines, c.M))
    a[..., 1] = 0.0
    b[..., 1] = 0.0
    return a, b


# Which workgroup takes which line.  The wave kernels are grid-stride: wave w of workgroup g takes the lines
# 4 g + w + 4 grid p of the passes p = 0, 1, .. below nlines (both generations: `line = blockIdx.x * WAVES + wave;
# line += gridDim.x * WAVES`), with grid = ceil(nlines / (4 lpw)) workgroups -- so a wave's lines are 4 grid apart, not
# adjacent.  The workgroup kernel takes the line pair (2 q, 2 q + 1) of its (swizzled) index q; the last workgroup's is
# always the last pair.
def wave_grid(c):
    return -(-c.nlines // (WAVES * c.lpw))


def wave_place(c, line):
    """(workgroup, wave, pass) of a line of a wave-kernel case"""
    stride = WAVES * wave_grid(c)
    return (line % stride) // WAVES, line % WAVES, line // stride


def passes(c):
    return -(-c.nlines // (WAVES * wave_grid(c)))


def last_workgroup_lines(c):
    if c.family == WG:
        return list(range(2 * ((c.nlines + 1) // 2 - 1), c.nlines))
    grid = wave_grid(c)
    return [l for p in range(passes(c)) for l in range(WAVES * (grid * p + grid - 1), WAVES * grid * (p + 1)) if l < c.nlines]


def short_wave_lines(c):
    """Wave kernels: the last line of every wave that takes fewer lines than the others (the last pass ends before it):
    where a ragged line count cuts the lines-per-wave loop short."""
    if c.family == WG:
        return []
    stride, np_ = WAVES * wave_grid(c), passes(c)
    return [l - stride for l in range(c.nlines, stride * np_) if l - stride >= 0]


def subset(c):
    """The lines the longdouble reference is applied to: the first and the last four, every line of the last workgroup
    (all its passes), the last line of every wave the ragged count cuts short, and 32 seeded random ones."""
    rng = np.random.default_rng(c.nlines + 31 * c.N)
    pick = {0} | set(range(max(0, c.nlines - 4), c.nlines)) | set(last_workgroup_lines(c)) | set(short_wave_lines(c))
    pick |= set(int(i) for i in rng.integers(0, c.nlines, SUBSET_RANDOM))
    return np.array(sorted(pick))


def alone_lines(c):
    """Wave kernels with several lines per wave: seven consecutive lines of the first, the second and the last pass, i.e.
    lines their waves take before and after other lines; run alone they must give the same bits."""
    stride = WAVES * wave_grid(c)
    out = []
    for p in sorted({0, 1, passes(c) - 1}):
        out += [l for l in range(stride * p, stride * p + 7) if l < c.nlines]
    return out


def nan_plants(c):
    """Lines for the planted NaN of a wave-kernel case with several passes: (the issue's line nlines - 2, the last line its
    wave takes: anything it leaves behind could only reach an EARLIER line, through a prefetch; [lines of other waves that
    take further lines afterwards -- first pass, and a middle pass where there are more than two -- whose leftovers in a
    reused staging or exchange buffer would reach a LATER line])."""
    stride, np_ = WAVES * wave_grid(c), passes(c)
    last = c.nlines - 2
    others = [5] + ([stride * (np_ // 2) + 6] if np_ > 2 else [])
    for l in others:
        assert wave_place(c, l)[:2] != wave_place(c, last)[:2] and l + stride < c.nlines
    return last, others


# ---- the longdouble reference -----------------------------------------------------------------------------------------
_MATRICES = {}


def _angles(N, K):
    """cos and sin of 2 pi k n / N for k <= K, arguments reduced in integers"""
    kn = (np.arange(K + 1)[:, None] * np.arange(N)[None, :]) % N
    ang = (LD(2) * PI / LD(N)) * kn.astype(LD)
    return np.cos(ang), np.sin(ang)


def matrices(N, M):
    """(synthesis [N][M], its derivative form per unit dscale [N][M], analysis [M][N]) in longdouble."""
    if (N, M) not in _MATRICES:
        K = kmax(N, M)
        cs, sn = _angles(N, K)
        S, D, A = np.zeros((N, M), LD), np.zeros((N, M), LD), np.zeros((M, N), LD)
        S[:, 0] = 1
        A[0] = LD(1) / LD(N)
        for k in range(1, K + 1):
            S[:, 2 * k], S[:, 2 * k + 1] = cs[k], -sn[k]
            # d/dy at load: (cos, -sin) amplitudes (c, s) of mode k -> (-k dscale s, k dscale c)
            D[:, 2 * k], D[:, 2 * k + 1] = k * S[:, 2 * k + 1], -k * S[:, 2 * k]
            A[2 * k], A[2 * k + 1] = (LD(2) / LD(N)) * cs[k], -(LD(2) / LD(N)) * sn[k]
        _MATRICES.clear()                         # (one size at a time: the largest is 3 x 16 MB)
        _MATRICES[(N, M)] = (S, D, A)
    return _MATRICES[(N, M)]


def longdouble_reference(c, a, b, lines):
    """out [nc][len(lines)][M] of the lines `lines`, by matrices on the N-point grid."""
    na, nb, nc, terms, ads, bds = TABLES[c.table]
    S, D, A = matrices(c.N, c.M)

    def grid(x, ds):
        syn = S if not ds else LD(ds) * D
        return x[lines].astype(LD) @ syn.T
    ga = [grid(a[i], ads[i]) for i in range(na)]
    gb = {}
    acc = [np.zeros((len(lines), c.N), LD) for _ in range(nc)]
    for ic, ia, ib, cf in terms:
        if ib not in gb:
            gb[ib] = grid(b[ib], bds[ib])
        acc[ic] += LD(cf) * ga[ia] * gb[ib]
    return np.stack([g @ A.T for g in acc])


def oracle(c, a, b):
    """out [nc][nlines][M] of every line, NumpyExecutor."""
    from oracle.np_executor import NumpyExecutor
    na, nb, nc, terms, ads, bds = TABLES[c.table]
    out = np.full((nc, c.nlines, c.M), np.nan)
    NumpyExecutor().rfft_bilinear_fused(("rfft", c.N, c.M), None, [a[i] for i in range(na)], [b[i] for i in range(nb)],
                                        [out[i] for i in range(nc)], c.nlines, terms, ads, bds)
    return out


def per_line_error(got, ref):
    """largest rel-L2 over (result, line) of got [nc][n][M] against the longdouble ref [nc][n][M]"""
    d = np.sqrt(((got.astype(LD) - ref) ** 2).sum(axis=-1))
    n = np.sqrt((ref ** 2).sum(axis=-1))
    return float((d / np.maximum(n, LD(1e-300))).max())


def rel(a, b):
    return float(np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-300))


_REFERENCES = {}


def references(c):
    """(a, b, oracle of all lines, subset, longdouble reference of the subset); computed once per case and kept for the
    small cases (read-only: nobody writes into them)."""
    key = case_id(c)
    if key in _REFERENCES:
        return _REFERENCES[key]
    a, b = inputs(c)
    lines = subset(c)
    res = (a, b, oracle(c, a, b), lines, longdouble_reference(c, a, b, lines))
    for x in res:
        x.setflags(write=False)
    if c.nlines <= 1024:
        _REFERENCES[key] = res
    return res


def plan_info(N, M, nlines):
    """ddh_rfft_fused_plan_info -> dict; host only"""
    import ctypes as C

    from dedalus_amd import libhip
    info = (C.c_int * 9)(*([-1] * 9))
    libhip.call("ddh_rfft_fused_plan_info", N, M, nlines, info)
    return dict(zip(("internal", "family", "C", "NT", "twreg", "dma", "lpw", "grid", "block"), list(info)))


def assert_selection(c):
    """the library reports what the case's row claims: a fallback to another kernel fails here"""
    got = plan_info(c.N, c.M, c.nlines)
    want = dict(internal=c.internal, family=c.family, C=c.C, NT=c.NT, lpw=c.lpw)
    assert {k: got[k] for k in want} == want, (case_id(c), got)
    if c.family == WG:
        assert got["grid"] == (c.nlines + 1) // 2
    else:
        assert got["grid"] == -(-c.nlines // (WAVES * c.lpw)) and got["block"] == 64 * WAVES
    return got


# ---- end to end: the under-dealiased stage inside a run ---------------------------------------------------------------
E2E_SHAPE = (8, 128, 8)
E2E_DT = 1e-3
E2E_STEPS = 3
E2E_SPEC = ("rfft", 128, 128)
E2E_GOLDEN = "fused_dealias1.npz"


def rayleigh_benard_dealias1(d3, timestepper="RK222", dist_kw=None):
    """The 3-D Rayleigh-Benard problem of tests/problems.py with every basis at dealias = 1: the y axis (the axis of the
    fused stage) has 128 modes on 128 points.  The initial buoyancy and velocity are seeded noise of O(0.1) at every
    wavenumber, so that the aliased part of u.grad(b) and u.grad(u) is of the order of the products themselves."""
    Nx, Ny, Nz = E2E_SHAPE
    Lx, Ly, Lz = 4, 4, 1
    Rayleigh, Prandtl, dealias = 2e6, 1, 1
    coords = d3.CartesianCoordinates('x', 'y', 'z')
    dist = d3.Distributor(coords, dtype=np.float64, **(dist_kw or {}))
    xbasis = d3.RealFourier(coords['x'], size=Nx, bounds=(0, Lx), dealias=dealias)
    ybasis = d3.RealFourier(coords['y'], size=Ny, bounds=(0, Ly), dealias=dealias)
    zbasis = d3.ChebyshevT(coords['z'], size=Nz, bounds=(0, Lz), dealias=dealias)
    B, Bh = (xbasis, ybasis, zbasis), (xbasis, ybasis)
    p = dist.Field(name='p', bases=B)
    b = dist.Field(name='b', bases=B)
    u = dist.VectorField(coords, name='u', bases=B)
    tau_p = dist.Field(name='tau_p')
    tau_b1 = dist.Field(name='tau_b1', bases=Bh)
    tau_b2 = dist.Field(name='tau_b2', bases=Bh)
    tau_u1 = dist.VectorField(coords, name='tau_u1', bases=Bh)
    tau_u2 = dist.VectorField(coords, name='tau_u2', bases=Bh)
    kappa = (Rayleigh * Prandtl) ** (-1 / 2)
    nu = (Rayleigh / Prandtl) ** (-1 / 2)
    x, y, z = dist.local_grids(*B)
    ex, ey, ez = coords.unit_vector_fields(dist)
    lift_basis = zbasis.derivative_basis(1)
    lift = lambda A: d3.Lift(A, lift_basis, -1)
    grad_u = d3.grad(u) + ez * lift(tau_u1)
    grad_b = d3.grad(b) + ez * lift(tau_b1)
    problem = d3.IVP([p, b, u, tau_p, tau_b1, tau_b2, tau_u1, tau_u2], namespace=locals())
    problem.add_equation("trace(grad_u) + tau_p = 0")
    problem.add_equation("dt(b) - kappa*div(grad_b) + lift(tau_b2) = - u@grad(b)")
    problem.add_equation("dt(u) - nu*div(grad_u) + grad(p) - b*ez + lift(tau_u2) = - u@grad(u)")
    problem.add_equation("b(z=0) = Lz")
    problem.add_equation("u(z=0) = 0")
    problem.add_equation("b(z=Lz) = 0")
    problem.add_equation("u(z=Lz) = 0")
    problem.add_equation("integ(p) = 0")
    solver = problem.build_solver(getattr(d3, timestepper))
    rng = np.random.default_rng(128)
    shape = np.broadcast(x, y, z).shape
    b['g'] = 0.1 * rng.standard_normal(shape) * z * (Lz - z) + (Lz - z)
    u['g'] = 0.1 * rng.standard_normal((3,) + shape) * z * (Lz - z)
    return solver, dict(p=p, b=b, u=u, tau_b1=tau_b1, tau_b2=tau_b2, tau_u1=tau_u1, tau_u2=tau_u2)


def run_dealias1(d3, dist_kw=None):
    solver, fields = rayleigh_benard_dealias1(d3, dist_kw=dist_kw)
    start = {k: np.array(f['c']) for k, f in fields.items()}
    for _ in range(E2E_STEPS):
        solver.step(E2E_DT)
    return solver, start, {k: np.array(f['c']) for k, f in fields.items()}
