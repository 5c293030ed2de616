"""Case table and longdouble reference for the size-generic transform kernel (fft_axis_kernel, csrc/ddh_fft.hip) at its
radix and launch-shape edges.  No GPU work here: tests/test_transform_edge_cases_host.py pins the table and the
double-precision oracle to this reference on the CPU, tests/test_gpu_transform_edges.py runs the kernel against both.

Reference: the matrix definition of every transform as plain longdouble sums of cos / sin.  The
angle of every matrix entry is reduced with exact integers -- (j k) mod N for the Fourier kinds, (2 j + 1) k mod 4 N
for Chebyshev -- and looked up in a longdouble table of one period, so that no entry carries an argument-reduction
error.  The conversion matrix is the float64 matrix the plan is given, applied (forward) or solved by upper-banded back
substitution (backward) in longdouble.  Nothing here calls an FFT or oracle/np_transforms.py.

Launch shapes: plan_mirror restates transform_plan's arithmetic for the workgroup kernel (csrc/ddh_fftwave.hip);
solve_mirror that of the conversion solve's path selection (CHEB_BWD in csrc/ddh_fft.hip, make_plan).  Every row of the
table carries the (B, T, lds) it was put there to hit; the host test checks the mirror against it and the GPU test checks
ddh_fft_plan_info against the mirror, so a row cannot silently lose its target."""
import functools
import math
from collections import namedtuple

import numpy as np

LD = np.longdouble
PI = 4 * np.arctan(LD(1))

TOL = 1e-12              # forward and plain backward (tests/test_gpu_transforms.py)
TOL_SOLVE = 1e-11        # backward through a conversion solve
ORACLE_MARGIN = 0.1      # oracle/np_transforms.py stays within this fraction of the bound against the longdouble reference
GUARD = 64               # sentinel doubles on each side of a destination
SENTINEL = -7.25e3
DSCALE = 2 * np.pi / 4.0
STRETCH = 1.7            # z-derivative of the dual Chebyshev entry point: differentiation_matrix * (2 / STRETCH)
BIG = 512                # above it: three shapes, two lines against the longdouble reference

RFFT_OPS = ("forward", "backward", "backward_deriv", "backward_dual")
CFFT_OPS = ("forward", "backward")
CHEB_OPS = ("forward", "backward")

# kind: rfft / cfft / cheb; alpha: ultraspherical parameter of the coefficient basis (cheb); decay: exponent of the
# 1 / (1 + k)^decay envelope of a backward input that goes through a conversion solve; expect: what plan_mirror must give
# for EVERY shape of the row (keys B, T, lds; "lds_gt" / "lds_le": a bound on lds); why: the property the row pins
Case = namedtuple("Case", "kind N M alpha ops decay expect why")

_SMALL = dict(T=256, lds_le=64 * 1024)


def _rows():
    rows = []

    def rf(N, M, why, expect=None):
        rows.append(Case("rfft", N, M, 0, RFFT_OPS, 0, expect or _SMALL, why))

    def cf(N, M, why, expect=None):
        rows.append(Case("cfft", N, M, 0, CFFT_OPS, 0, expect or _SMALL, why))

    def ch(N, M, alpha, why, expect=None, ops=CHEB_OPS, decay=2):
        rows.append(Case("cheb", N, M, alpha, ops, decay, expect or _SMALL, why))

    for N, M, why in [(1, 2, "length 1: no pass at all"), (2, 2, "length 2, K = 0"), (3, 2, "length 3, odd, K = 0"),
                      (4, 4, "one radix-4 pass"), (6, 4, "one radix-6 pass"), (9, 6, "3 x 3, odd")]:
        rf(N, M, "tiny: " + why)
    for N, M, why in [(25, 16, "5 x 5"), (36, 24, "4 3 3 -> 6 6 rewrite"), (45, 30, "odd grid, 30 modes at 3/2: 3 3 5"),
                      (49, 32, "7 x 7"), (75, 50, "3 5 5, odd"), (105, 70, "3 5 7, odd"), (125, 84, "5 5 5"),
                      (144, 96, "16 3 3: must NOT take the 6 6 rewrite"), (343, 228, "7 7 7"),
                      (1000, 666, "8 5 5 5, more than 512 points")]:
        rf(N, M, "radix: " + why)
    rf(48, 64, "M > N, even N: K from the grid")
    rf(45, 64, "M > N, odd N: K = (N - 1) / 2")
    rf(1728, 1152, "T = 512 with B = 2", dict(B=2, T=512, lds=60176))
    rf(1920, 1280, "T = 512, LDS opt-in above 64 KiB", dict(B=2, T=512, lds=66800))
    rf(2048, 1364, "B = 1 with T = 256", dict(B=1, T=256, lds=36384))
    rf(3456, 2304, "B = 1 with T = 512", dict(B=1, T=512, lds=61024))
    rf(8192, 5460, "the 1024-thread instantiation, 141 KiB", dict(B=1, T=1024, lds=143904))
    rf(9216, 6144, "largest LDS request that fits 160 KiB", dict(B=1, T=1024, lds=161824))

    cf(1, 1, "length 1")
    cf(2, 2, "even M = N = 2: the 2 m == M slot is all there is beside k = 0")
    cf(15, 10, "odd N, even M: Nyquist slot m = 5 zeroed")
    cf(45, 30, "odd N, three passes")
    cf(63, 42, "3 3 7, odd N")
    cf(64, 64, "M = N even: Nyquist slot and K = N / 2 - 1")
    cf(96, 64, "16 6")
    cf(48, 64, "M > N")
    cf(768, 512, "multi-pass, several lines per workgroup")
    cf(1920, 1280, "LDS opt-in above 64 KiB", dict(B=2, T=512, lds=66800))
    cf(8192, 5461, "odd M at the 1024-thread instantiation", dict(B=1, T=1024, lds=143904))

    for alpha in range(4):
        for N, M, why in [(2, 2, "length 2"), (3, 2, "length 3"), (45, 30, "odd N"), (49, 49, "odd M = N"),
                          (210, 140, "ragged chain, E = 2"), (48, 64, "M > N: solve truncated to N")]:
            ch(N, M, alpha, "alpha %d: %s" % (alpha, why))
    for alpha in range(3):
        ch(1536, 1024, alpha, "alpha %d: E = 8, the last scan size" % alpha, dict(B=2, T=256, lds=53552))
        ch(1728, 1152, alpha, "alpha %d: E = 9, serial fallback; T = 512" % alpha, dict(B=2, T=512, lds=60176))
    for alpha in range(2):
        ch(8192, 5460, alpha, "alpha %d: the 1024-thread instantiation" % alpha, dict(B=1, T=1024, lds=143904))
    ch(210, 140, 1, "dual backward: plain + derivative through the alpha = 1 solve", ops=("backward_dual",), decay=3)
    ch(1728, 1152, 1, "dual backward at T = 512, E = 9", dict(B=2, T=512, lds=60176), ops=("backward_dual",), decay=3)
    return rows


CASES = _rows()


def case_id(c):
    tag = "%s-%dx%d" % (c.kind, c.N, c.M)
    if c.kind == "cheb":
        tag += "-a%d" % c.alpha
    if c.ops == ("backward_dual",):
        tag += "-dual"
    return tag


CASE_IDS = [case_id(c) for c in CASES]

# Refused at plan creation (kind, N, M, alpha, text of the library's message)
PLAN_REFUSALS = [("rfft", 11, 8, 0, "must factor into 2,3,5,7"), ("cfft", 22, 14, 0, "must factor into 2,3,5,7"),
                 ("cheb", 208, 138, 0, "must factor into 2,3,5,7"), ("rfft", 16, 15, 0, "n_coeff must be even"),
                 ("cheb", 48, 32, 4, "at most 4 conversion bands")]
# Refused by the call: the plan exists, no kernel takes the axis
CALL_REFUSALS = [("rfft", 10240, 6826, "axis too long")]
# Either runs and matches, or is refused with the library's own message.  With the whole dynamic-LDS request held against
# 160 KiB (lines AND twiddle table: 165184 B and 168544 B here) both are refused.
LDS_EDGE = [("rfft", 9408, 6272), ("rfft", 9600, 6400)]


def shapes_for(N):
    """(shape, axis = 1).  Small: contiguous lines 1 / 3 / 35 (B clamped to the pair count; two blocks with a half-empty
    last pair), strided odd inner 19 (ragged second block, half-empty last pair), strided even inner 36 (partial block)."""
    if N <= BIG:
        return [(1, N), (3, N), (35, N), (2, N, 19), (1, N, 36)]
    return [(3, N), (2, N, 3), (1, N, 4)]


def outer_inner(shape):
    return int(shape[0]), int(np.prod(shape[2:], dtype=np.int64))


# ---------------------------------------------------------------------------------------------------------------------
# mirrors of the planner
# ---------------------------------------------------------------------------------------------------------------------
LDS_LIMIT = 160 * 1024


def tw_bytes(N):
    return (32 + (N >> 5) + 1) * 16


def plan_mirror(kind, N, outer, inner):
    """transform_plan for the workgroup kernel: dict(B, T, grid, lds), or the error text"""
    strided = inner > 1
    if kind == "cfft":
        npairs = inner if strided else outer
    else:
        npairs = (inner + 1) // 2 if strided else (outer + 1) // 2
    per_line = (N + (N >> 4) + 1) * 16
    B = 8 if strided else 4
    if not strided:
        while B < 16 and N * 2 * B <= 12 * 256:
            B *= 2
    while B > 1 and per_line * B > 64 * 1024:
        B //= 2
    B = min(B, npairs)
    if per_line * B + tw_bytes(N) > LDS_LIMIT:
        return "axis too long"
    T = 256
    while N * B > 12 * T and T < 1024:
        T *= 2
    if N * B > 12 * T:
        return "axis too long"
    bpo = (npairs + B - 1) // B
    return dict(B=B, T=T, grid=bpo * outer if strided else bpo, lds=per_line * B + tw_bytes(N), npairs=npairs)


def factorize_mirror(n):
    """factorize() of csrc/ddh_fft.hip: the pass schedule, or None for a prime factor above 7"""
    radix = []
    for r in (16, 8, 4, 2, 3, 5, 7):
        while n % r == 0 and n > 1:
            radix.append(r)
            n //= r
    if n != 1:
        return None
    while 2 in radix and 3 in radix:
        radix.remove(2)
        radix.remove(3)
        radix.append(6)
    while 4 in radix and radix.count(3) >= 2:
        radix.remove(4)
        radix.remove(3)
        radix.remove(3)
        radix += [6, 6]
    return radix


def solve_mirror(N, M, offsets):
    """The conversion solve of CHEB_BWD: dict(g, order, E, path); path: scan / serial (table) / general (p.bands loop)"""
    g = 0
    for o in offsets:
        g = math.gcd(g, int(o))
    g = g or 1
    ring_ok = all(o // g <= 2 for o in offsets[1:])
    order = 0 if not ring_ok else (2 if any(o // g == 2 for o in offsets[1:]) else 1)
    Mk = min(M, N)
    L = (Mk + g - 1) // g
    E = (L + 63) >> 6
    path = "scan" if ring_ok and order == 1 and E <= 8 else ("serial" if ring_ok else "general")
    return dict(g=g, order=order, E=E, L=L, path=path)


@functools.lru_cache(maxsize=None)
def conversion(M, alpha):
    """(float64 sparse matrix as the plan gets it, offsets int32, bands [nbands][M]); alpha = 0: (None, None, None)"""
    if alpha == 0:
        return None, None, None
    from dedalus_amd.tools import jacobi
    conv = jacobi.conversion_matrix(M, -0.5, -0.5, alpha - 0.5, alpha - 0.5)
    offs = np.array([o for o in range(M) if np.any(conv.diagonal(o) != 0)], dtype=np.int32)
    bands = np.zeros((len(offs), M))
    for d, o in enumerate(offs):
        bands[d, :M - o] = conv.diagonal(o)
    return conv, offs, bands


@functools.lru_cache(maxsize=None)
def dual_dvec(M):
    from dedalus_amd.tools import jacobi
    D = jacobi.differentiation_matrix(M, -0.5, -0.5) * (2.0 / STRETCH)
    dvec = np.zeros(M)
    dvec[:M - 1] = D.diagonal(1)
    return dvec


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
_OPCODE = {"forward": 0, "backward": 1, "backward_deriv": 2, "backward_dual": 3}


def coeff_shape(c, shape):
    return (shape[0], c.M) + tuple(shape[2:])


def make_input(c, op, shape):
    """Seeded standard normal.  Forward: grid data of `shape`; backward: coefficients of coeff_shape.  Real Fourier: the
    msin slot of k = 0 is no mode -- the oracle and the kernel both ignore it on input -- and is zeroed, except in the LAST
    line, where a non-zero value pins that it is ignored."""
    rng = np.random.default_rng([c.N, c.M, c.alpha, _OPCODE[op]] + list(shape))
    if op == "forward":
        if c.kind == "cfft":
            return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
        return rng.standard_normal(shape)
    cs = coeff_shape(c, shape)
    if c.kind == "cfft":
        return rng.standard_normal(cs) + 1j * rng.standard_normal(cs)
    a = rng.standard_normal(cs)
    if c.kind == "rfft":
        keep = a.reshape(cs[0], c.M, -1)[-1, 1, -1]
        a[:, 1] = 0.0
        a.reshape(cs[0], c.M, -1)[-1, 1, -1] = keep
    elif c.alpha > 0 or op == "backward_dual":
        env = (1.0 + np.arange(c.M)) ** float(c.decay)
        a /= env.reshape((1, -1) + (1,) * (len(cs) - 2))
    return a


def lines_of(a, n_axis):
    """[outer][n][inner...] -> [n][outer * inner]: one column per line"""
    a = a.reshape(a.shape[0], n_axis, -1)
    return np.ascontiguousarray(np.moveaxis(a, 1, 0)).reshape(n_axis, -1)


def compared_lines(N, nlines):
    """line indices held against the longdouble reference"""
    return np.arange(nlines) if N <= BIG else np.array(sorted({0, nlines - 1}))


def line_errors(got, ref):
    """rel-L2 of every column of got [n][lines] against ref (longdouble)"""
    d = got.astype(ref.dtype) - ref
    num = np.sqrt((np.abs(d) ** 2).sum(axis=0))
    den = np.sqrt((np.abs(ref) ** 2).sum(axis=0))
    den = np.where(den > 0, den, LD(1))          # an all-zero reference line (K = 0 derivative): absolute error
    return (num / den).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------------
# the longdouble matrix definitions
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=8)
def _period_table(P):
    a = (2 * PI / LD(P)) * np.arange(P, dtype=LD)
    return np.cos(a), np.sin(a)


def _chunked(nrows, ncols):
    """row chunks of a matrix of bounded size, so that 8192 points stay in memory"""
    step = max(1, min(nrows, (1 << 21) // max(ncols, 1)))
    for i0 in range(0, nrows, step):
        yield i0, min(nrows, i0 + step)


def _apply(nrows, ncols, block, xs):
    """block(i0, i1) -> tuple of longdouble [i1 - i0][ncols] matrices; returns per matrix and per x the product"""
    outs = None
    for i0, i1 in _chunked(nrows, ncols):
        mats = block(i0, i1)
        if outs is None:
            outs = [[np.zeros((nrows, x.shape[1]), dtype=LD) for x in xs] for _ in mats]
        for a, m in enumerate(mats):
            for b, x in enumerate(xs):
                outs[a][b][i0:i1] = m @ x
    return outs


def kmax(N, M):
    return min((N - 1) // 2, (M - 1) // 2)


def rfft_forward_ref(g, M):
    """g [N][lines] -> c [M][lines], (cos, msin) interleaved"""
    N = g.shape[0]
    K = kmax(N, M)
    cos, sin = _period_table(N)
    j = np.arange(N, dtype=np.int64)

    def block(i0, i1):
        m = np.arange(i0, i1, dtype=np.int64)
        k = m // 2
        idx = (k[:, None] * j[None, :]) % N
        mat = np.where((m % 2 == 1)[:, None], -sin[idx], cos[idx])
        scale = np.where(k == 0, LD(1), LD(2)) / LD(N)
        scale = np.where((k > K) | (m == 1), LD(0), scale)
        return (mat * scale[:, None],)

    return _apply(M, N, block, [g.astype(LD)])[0][0]


def rfft_deriv_coeffs(c, dscale):
    """d/dx on (cos, msin) coefficients [M][lines]: (cos, msin) -> (-kappa msin, kappa cos), kappa = dscale k; longdouble"""
    c = c.astype(LD)
    kap = (LD(dscale) * np.arange(c.shape[0] // 2, dtype=LD))[:, None]
    d = np.empty_like(c)
    d[0::2] = -kap * c[1::2]
    d[1::2] = kap * c[0::2]
    return d


def rfft_backward_ref(c, N):
    """c [M][lines] -> g [N][lines]"""
    M = c.shape[0]
    K = kmax(N, M)
    cos, sin = _period_table(N)
    m = np.arange(M, dtype=np.int64)
    k = m // 2
    live = np.where((k > K) | (m == 1), LD(0), LD(1))

    def block(i0, i1):
        j = np.arange(i0, i1, dtype=np.int64)
        idx = (j[:, None] * k[None, :]) % N
        return (np.where((m % 2 == 1)[None, :], -sin[idx], cos[idx]) * live[None, :],)

    return _apply(N, M, block, [c.astype(LD)])[0][0]


def cfft_wavenumbers(N, M):
    """slot m -> wavenumber k, and which slots carry a mode: |k| <= K and not the 2 m == M slot"""
    m = np.arange(M, dtype=np.int64)
    k = np.where(m <= (M - 1) // 2, m, m - M)
    live = (np.abs(k) <= kmax(N, M)) & (2 * m != M)
    return k, live


def cfft_forward_ref(g, M):
    N = g.shape[0]
    cos, sin = _period_table(N)
    k, live = cfft_wavenumbers(N, M)
    j = np.arange(N, dtype=np.int64)
    gr, gi = g.real.astype(LD), g.imag.astype(LD)

    def block(i0, i1):
        idx = (k[i0:i1, None] * j[None, :]) % N
        s = np.where(live[i0:i1], LD(1), LD(0))[:, None] / LD(N)
        return cos[idx] * s, sin[idx] * s

    (cr, ci), (sr, si) = _apply(M, N, block, [gr, gi])
    return (cr + si) + 1j * (ci - sr).astype(np.clongdouble)        # sum g (cos - i sin)


def cfft_backward_ref(c, N):
    M = c.shape[0]
    cos, sin = _period_table(N)
    k, live = cfft_wavenumbers(N, M)
    s = np.where(live, LD(1), LD(0))[None, :]
    cr, ci = c.real.astype(LD), c.imag.astype(LD)

    def block(i0, i1):
        j = np.arange(i0, i1, dtype=np.int64)
        idx = (j[:, None] * k[None, :]) % N
        return cos[idx] * s, sin[idx] * s

    (xr, xi), (yr, yi) = _apply(N, M, block, [cr, ci])
    return (xr - yi) + 1j * (xi + yr).astype(np.clongdouble)        # sum c (cos + i sin)


def _cheb_cos(N, kk, jj):
    """cos(pi k (2 j + 1) / (2 N)) for index vectors kk (rows) x jj (columns), or jj rows x kk columns if transposed"""
    cos, _ = _period_table(4 * N)
    return cos[(kk * (2 * jj + 1)) % (4 * N)]


def cheb_analysis_ref(g, M):
    """g [N][lines] on the ascending Gauss grid -> orthonormal Chebyshev-T coefficients [M][lines]"""
    N = g.shape[0]
    Mk = min(M, N)
    j = np.arange(N, dtype=np.int64)
    sq = np.sqrt(PI)

    def block(i0, i1):
        k = np.arange(i0, i1, dtype=np.int64)
        fs = np.where(k % 2 == 0, LD(1), LD(-1)) * np.sqrt(PI / 2) / LD(N)
        fs = np.where(k == 0, sq / (2 * LD(N)), fs)
        return (2 * fs[:, None] * _cheb_cos(N, k[:, None], j[None, :]),)

    c = np.zeros((M, g.shape[1]), dtype=LD)
    c[:Mk] = _apply(Mk, N, block, [g.astype(LD)])[0][0]
    return c


def cheb_convert_ref(c, alpha):
    """the conversion matrix (as the plan gets it) applied in longdouble"""
    M = c.shape[0]
    _, offs, bands = conversion(M, alpha)
    if offs is None:
        return c
    out = np.zeros_like(c)
    for d, o in enumerate(offs):
        out[:M - o] += bands[d, :M - o].astype(LD)[:, None] * c[o:]
    return out


def cheb_forward_ref(g, M, alpha):
    return cheb_convert_ref(cheb_analysis_ref(g, M), alpha)


def cheb_solve_ref(c, N, alpha):
    """upper-banded back substitution of the conversion matrix on the leading min(M, N) coefficients (the rest dropped
    BEFORE the solve), longdouble"""
    M = c.shape[0]
    Mk = min(M, N)
    _, offs, bands = conversion(M, alpha)
    x = np.zeros((M, c.shape[1]), dtype=LD)
    bl = bands.astype(LD)
    c = c.astype(LD)
    for k in range(Mk - 1, -1, -1):
        acc = c[k].copy()
        for d in range(1, len(offs)):
            kk = k + int(offs[d])
            if kk < Mk:
                acc -= bl[d, k] * x[kk]
        x[k] = acc / bl[0, k]
    return x


def cheb_synthesis_ref(x, N):
    """coefficients x [M][lines] of the grid's own basis -> values on the ascending Gauss grid [N][lines]"""
    Mk = min(x.shape[0], N)
    k = np.arange(Mk, dtype=np.int64)
    bs = np.where(k % 2 == 0, LD(1), LD(-1)) * np.sqrt(2 / PI)
    bs = np.where(k == 0, 1 / np.sqrt(PI), bs)

    def block(i0, i1):
        j = np.arange(i0, i1, dtype=np.int64)
        return (_cheb_cos(N, k[None, :], j[:, None]) * bs[None, :],)

    return _apply(N, Mk, block, [x[:Mk].astype(LD)])[0][0]


def cheb_backward_ref(c, N, alpha):
    return cheb_synthesis_ref(cheb_solve_ref(c, N, alpha) if alpha > 0 else c, N)


def derivative_coeffs(c):
    """(D c)[k] = dvec[k] c[k + 1], float64 exactly as one product per entry: [M][...]"""
    M = c.shape[0]
    dc = np.zeros_like(c)
    dc[:M - 1] = dual_dvec(M)[:M - 1].reshape((-1,) + (1,) * (c.ndim - 1)) * c[1:]
    return dc


def reference_many(c, items):
    """longdouble outputs of entry points on the columns of their inputs: items = [(op, x_lines)], returns per item a list
    (two arrays for backward_dual).  Whatever differs between the entry points is applied to the columns before or after
    the synthesis / analysis matrix, so the matrix of a direction is built once for all items."""
    fwd, bwd = [], []                 # column blocks through the analysis (forward) / synthesis (backward) matrix
    for op, x in items:
        if op == "forward":
            fwd.append(x)
        elif c.kind == "rfft":
            bwd += {"backward": [x], "backward_deriv": [rfft_deriv_coeffs(x, DSCALE)],
                    "backward_dual": [x, rfft_deriv_coeffs(x, DSCALE)]}[op]
        elif c.kind == "cfft":
            bwd.append(x)
        elif op == "backward":
            bwd.append(cheb_solve_ref(x, c.N, c.alpha) if c.alpha > 0 else x)
        else:
            bwd += [x, cheb_solve_ref(derivative_coeffs(x), c.N, c.alpha)]
    outs = {}
    for name, blocks in (("f", fwd), ("b", bwd)):
        if not blocks:
            continue
        cd = np.clongdouble if c.kind == "cfft" else LD
        X = np.concatenate([b.astype(cd) for b in blocks], axis=1)
        if name == "f":
            Y = {"rfft": lambda: rfft_forward_ref(X, c.M), "cfft": lambda: cfft_forward_ref(X, c.M),
                 "cheb": lambda: cheb_forward_ref(X, c.M, c.alpha)}[c.kind]()
        else:
            Y = {"rfft": lambda: rfft_backward_ref(X, c.N), "cfft": lambda: cfft_backward_ref(X, c.N),
                 "cheb": lambda: cheb_synthesis_ref(X, c.N)}[c.kind]()
        cuts = np.cumsum([b.shape[1] for b in blocks])[:-1]
        outs[name] = np.split(Y, cuts, axis=1)
    res = []
    for op, _ in items:
        if op == "forward":
            res.append([outs["f"].pop(0)])
        else:
            res.append([outs["b"].pop(0) for _ in range(2 if op == "backward_dual" else 1)])
    return res


def reference(c, op, x_lines):
    return reference_many(c, [(op, x_lines)])[0]


def oracle(c, op, x):
    """oracle/np_transforms.py on the whole array (axis 1): the same list"""
    from oracle import np_transforms as npt
    conv = conversion(c.M, c.alpha)[0]
    if c.kind == "rfft":
        if op == "forward":
            return [npt.rfft_forward(x, 1, c.M)]
        plain = npt.rfft_backward(x, 1, c.N)
        if op == "backward":
            return [plain]
        kap = (DSCALE * np.arange(c.M // 2)).reshape((1, -1) + (1,) * (x.ndim - 2))
        dc = np.empty_like(x)
        dc[:, 0::2] = -kap * x[:, 1::2]
        dc[:, 1::2] = kap * x[:, 0::2]
        deriv = npt.rfft_backward(dc, 1, c.N)
        return [deriv] if op == "backward_deriv" else [plain, deriv]
    if c.kind == "cfft":
        return [npt.cfft_forward(x, 1, c.M) if op == "forward" else npt.cfft_backward(x, 1, c.N)]
    if op == "forward":
        return [npt.cheb_forward(x, 1, c.M, conv)]
    if op == "backward":
        return [npt.cheb_backward(x, 1, c.N, conv)]
    dc = np.moveaxis(derivative_coeffs(np.moveaxis(x, 1, 0)), 0, 1)
    return [npt.cheb_backward(x, 1, c.N, None), npt.cheb_backward(np.ascontiguousarray(dc), 1, c.N, conv)]


def tolerances(c, op):
    """per output of `reference`: the bound the GPU result is held to"""
    if c.kind == "cheb" and op == "backward_dual":
        return [TOL, TOL_SOLVE]
    if c.kind == "cheb" and op == "backward" and c.alpha > 0:
        return [TOL_SOLVE]
    return [TOL, TOL] if op == "backward_dual" else [TOL]


def out_axis(c, op):
    return c.M if op == "forward" else c.N
