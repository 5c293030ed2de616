"""Synthetic plans, case table and high-precision references for the band LU kernels of dedalus_amd/csrc/ddh_ellband.hip
(ddh_ellband_create / factor / solve / gather_complex_inverse / bordered_inverse), importable without a device.
tests/test_ellband_cases_host.py proves the inputs (conditioning, pivot coverage, window selection) and the references;
tests/test_gpu_ellband_kernels.py runs the kernels on them.

The operation of one group g (layout: core/ellband.py::EllBandPlan): gather the permuted right-hand side r = rhs[row_index],
apply T to its first nbc_of[g] rows, solve (a M + b L) y = r, z = y + sum_s P[:, s] y[1 + s:], scatter z by col_index.
`reference` does that in np.longdouble with a dense partial-pivoting elimination; `baseline` does it in float64 through
LAPACK's dgbtrf / dgbtrs (the body of EllBandPlan.reference_solve, which the host test holds it equal to).

M and L are independent standard-normal bands without diagonal dominance, so LAPACK interchanges rows in most columns;
one planted entry of magnitude 10 on sub-diagonal kl makes the largest pivot offset exactly kl.  Rows past n[g] of
MB / LB / P are NaN: the kernels must not read them."""
import copy
import functools

import numpy as np

LD = np.longdouble
NAN = float("nan")

# ---- restated from dedalus_amd/csrc/ddh_ellband.hip -------------------------------------------------------------------
VARIANTS = ((12, 24), (20, 40), (28, 56), (36, 64), (36, 96))      # eb_variants: (nw, wt), first fit
EB_NBC, EB_MP = 8, 16                                              # boundary rows / recombination super diagonals at most
FORWARD_SLOTS, BACKWARD_SLOTS = 64, 16                             # slots per wave of the two sweeps
GATHER_SINGLE_PASS = 4096 * 256                                    # entries one pass of ellband_gather_cinv_kernel covers
BORDERED_ROW_STRIDE = 64                                           # gridDim.y - 1 of bordered_inverse_kernel
GUARD = 16                                                         # NaN doubles behind the gather's last block

AB_PAIRS = ((1.0, 0.37), (0.0, 1.0))
COND_CAP = 1e6          # cond_2(a M + b L) of every live group, both pairs (the host test asserts it)
COND_DRAW = 5e5         # a group is redrawn (same generator, so still deterministic) until it is within this
COND_TRIES = 60


def variant_for(kl, ku):
    """the rule of the header comment of ddh_ellband_create: kl + 1 <= nw and kl + ku <= wt, first fit"""
    for nw, wt in VARIANTS:
        if kl + 1 <= nw and kl + ku <= wt:
            return nw, wt
    return None


# name: (kl, ku, expected nw, expected wt, mp, nbc, nslots, ncomp, nmax, sizes of the live groups with slot_limit 0 and 1,
# layouts).  The expected windows are literals.
# nmax is 300 except for kl = 12, ku = 3: a standard-normal band that lopsided has cond_2 ~ 1e17 at n = 300 in every draw,
# beyond the cap this file keeps, while at n = 2 wt + 5 = 85 some draws are within it (the redraw loop finds one): that
# is its largest group; the 300-row systems of the (20, 40) windows are those of the next two rows.
CASES = {
    "kl3_ku4":     (3, 4, 12, 24, 0, 0, 1, 1, 300, 11, None, ("default",)),
    "kl11_ku13":   (11, 13, 12, 24, 16, 8, 15, 3, 300, 1, None, ("default",)),
    "kl12_ku3":    (12, 3, 20, 40, 1, 1, 17, 1, 85, 1, 19, ("default", "rows_by_slots")),
    "kl11_ku14":   (11, 14, 20, 40, 16, 0, 64, 3, 300, 19, 1, ("default",)),
    "kl19_ku21":   (19, 21, 20, 40, 0, 8, 65, 1, 300, 41, 20, ("default",)),
    "kl20_ku32":   (20, 32, 28, 56, 16, 8, 130, 3, 300, 1, None, ("default",)),
    "kl27_ku29":   (27, 29, 28, 56, 1, 1, 1, 1, 300, 27, None, ("default",)),
    "kl28_ku20":   (28, 20, 36, 64, 0, 1, 15, 3, 300, 36, 1, ("default",)),
    "kl35_ku29":   (35, 29, 36, 64, 1, 8, 17, 1, 300, 1, 35, ("default", "rows_by_slots")),
    "kl35_ku30":   (35, 30, 36, 96, 0, 0, 64, 3, 300, 1, 35, ("default",)),
    "kl35_ku61":   (35, 61, 36, 96, 16, 8, 65, 1, 300, 197, 1, ("default",)),
}
CASE_LAYOUTS = [(name, lay) for name, row in CASES.items() for lay in row[11]]
WIDEST = ("kl11_ku13", "kl19_ku21", "kl27_ku29", "kl35_ku29", "kl35_ku61")       # widest case of each variant
ALIVE_CASE = "kl20_ku32"                                                            # several factorizations at once


def group_sizes(nw, wt, nbc, nmax):
    """system sizes at the edges of the whole-block loops, one empty group between live ones, duplicates skipped"""
    out = []
    for n in (1, nbc + 1, nw - 1, nw, wt, 0, wt + 1, 2 * wt + 5, nmax):
        if n not in out and n <= nmax:
            out.append(n)
    return out


def slot_limits(nslots, sizes, zero_n, one_n):
    """slot_limit[g] from {0, 1, 20, nslots - 1, nslots}, clipped to nslots.  0 goes to the empty group and to the live
    group of size zero_n, 1 to the group of size one_n (None: to none): different sizes in the cases of a window variant,
    and none but the one-row system in a variant's only case with several slots, so that every size edge is solved in
    more than one slot on its variant (the host test asserts it).  The others take nslots, nslots - 1 and 20 in turn,
    the largest system first: the longest sweeps run every slot."""
    values = []
    for v in (nslots, nslots - 1, 20):
        v = min(v, nslots)
        if v > 0 and v not in values:
            values.append(v)
    lim = np.zeros(len(sizes), dtype=np.int32)
    rest = [g for g, n in enumerate(sizes) if n > 0 and n not in (zero_n, one_n)]
    assert len(rest) == sum(n > 0 for n in sizes) - 1 - (one_n is not None)
    for k, g in enumerate(sorted(rest, key=lambda g: -sizes[g])):
        lim[g] = values[k % len(values)]
    if one_n is not None:
        lim[sizes.index(one_n)] = 1
    return lim


def _orthogonal(k, rng):
    q, r = np.linalg.qr(rng.standard_normal((k, k)))
    return q * np.sign(np.diag(r))


class SyntheticPlan:
    """The attributes executor.EllBand reads, filled with seeded random systems (kind: "random" as described in the
    module docstring; "dominant": off-diagonals scaled by 1 / (kl + ku + 1) and 4 sign added to the diagonal, so that
    column dominance rules out every interchange; "one_swap": the same plus one entry of magnitude 10 on sub-diagonal kl
    of column n - 1 - kl, the only column whose interchange cannot unseat a later diagonal)."""

    def __init__(self, kl, ku, mp, nbc, sizes, ncomp, seed, kinds=None, zero_column_groups=()):
        rng = np.random.default_rng(seed)
        self.kl, self.ku, self.mp, self.nbc, self.ncomp = kl, ku, mp, nbc, ncomp
        self.nl, self.nmax = len(sizes), max(max(sizes), 1)
        self.nr = -(-self.nmax // ncomp)
        self.n = np.array(sizes, dtype=np.int32)
        self.nbc_of = np.minimum(nbc, self.n).astype(np.int32)
        nl, nmax, W = self.nl, self.nmax, kl + ku + 1
        self.T = np.zeros((nl, max(nbc, 1), max(nbc, 1)))
        self.P = np.full((nl, nmax, max(mp, 1)), NAN)
        self.MB = np.full((nl, nmax, W), NAN)
        self.LB = np.full((nl, nmax, W), NAN)
        self.row_index = np.full((nl, nmax), -1, dtype=np.int64)
        self.col_index = np.full((nl, nmax), -1, dtype=np.int64)
        self.planted = {}
        i = np.arange(nmax)[:, None]
        col = i - kl + np.arange(W)[None, :]
        for g, n in enumerate(sizes):
            kind = kinds[g] if kinds else "random"
            k = int(self.nbc_of[g])
            self.T[g, :k, :k] = _orthogonal(k, rng) if k else 0.0
            inside = (col[:n] >= 0) & (col[:n] < n)
            for attempt in range(COND_TRIES):
                M = np.where(inside, rng.standard_normal((n, W)), 0.0)
                L = np.where(inside, rng.standard_normal((n, W)), 0.0)
                if kind != "random" and n:
                    M, L = M / W, L / W
                    sgn = np.where(rng.standard_normal(n) < 0, -1.0, 1.0)
                    M[:, kl] = (np.abs(M[:, kl]) + 4.0) * sgn
                    L[:, kl] = (np.abs(L[:, kl]) + 4.0) * sgn
                if n > kl and kl > 0 and kind != "dominant":
                    j = n - 1 - kl if kind == "one_swap" else int(rng.integers(0, n - kl))
                    sgn = 1.0 if rng.standard_normal() > 0 else -1.0
                    M[j + kl, 0] = L[j + kl, 0] = 10.0 * sgn              # entry (j + kl, j)
                    self.planted[g] = j
                self.MB[g, :n], self.LB[g, :n] = M, L
                if n == 0 or kind != "random" or max(np.linalg.cond(self.dense(g, a, b, np.float64)) for a, b in AB_PAIRS) <= COND_DRAW:
                    break
            else:
                raise AssertionError("no draw of group %d (n = %d) within the condition cap" % (g, n))
            if g in zero_column_groups:
                j = n // 2
                rows = np.arange(max(j - ku, 0), min(j + kl, n - 1) + 1)
                M[rows, j - rows + kl] = L[rows, j - rows + kl] = 0.0
                self.MB[g, :n], self.LB[g, :n] = M, L
            ps = rng.standard_normal((n, max(mp, 1))) * 0.3
            ps[np.arange(n)[:, None] + 1 + np.arange(max(mp, 1))[None, :] >= n] = 0.0
            self.P[g, :n] = ps if mp else 0.0
            self.row_index[g, :n] = rng.permutation(ncomp * self.nr)[:n]
            self.col_index[g, :n] = rng.permutation(ncomp * self.nr)[:n]

    def without_P(self):
        """the same systems with a vanishing recombination band (same mp, so the same kernels run): their solution is
        the y of this plan's solves"""
        twin = copy.copy(self)
        twin.P = np.where(np.isnan(self.P), NAN, 0.0)
        return twin

    def dense(self, g, a, b, dtype=LD):
        """a M + b L of group g as a dense n x n matrix"""
        n, kl = int(self.n[g]), self.kl
        A = np.zeros((n, n), dtype=dtype)
        B = dtype(a) * self.MB[g, :n].astype(dtype) + dtype(b) * self.LB[g, :n].astype(dtype)
        for d in range(self.kl + self.ku + 1):
            i = np.arange(n)
            j = i - kl + d
            ok = (j >= 0) & (j < n)
            A[i[ok], j[ok]] = B[i[ok], d]
        return A


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (plan, nslots, slot_limit) of a row of CASES"""
    kl, ku, nw, wt, mp, nbc, nslots, ncomp, nmax, zero_n, one_n, _ = CASES[name]
    seed = 1000 + list(CASES).index(name)
    sizes = group_sizes(nw, wt, nbc, nmax)
    plan = SyntheticPlan(kl, ku, mp, nbc, sizes, ncomp, seed)
    return plan, nslots, slot_limits(nslots, sizes, zero_n, one_n)


@functools.lru_cache(maxsize=None)
def single_group_case(name):
    """the explicit-offset layout has one group: the 2 wt + 5 system of the row (nmax where that is smaller), every slot live"""
    kl, ku, nw, wt, mp, nbc, nslots, ncomp, nmax, zero_n, one_n, _ = CASES[name]
    plan = SyntheticPlan(kl, ku, mp, nbc, [min(2 * wt + 5, nmax)], 1, 2000 + list(CASES).index(name))
    return plan, nslots, np.array([nslots], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def pivot_case(name):
    """group 0: no interchange at all, group 1: one interchange, at offset kl; the widths of a row of CASES"""
    kl, ku, nw, wt, mp, nbc, nslots, ncomp, nmax, zero_n, one_n, _ = CASES[name]
    n = min(2 * wt + 5, nmax)
    plan = SyntheticPlan(kl, ku, mp, nbc, [n, n], ncomp, 3000 + list(CASES).index(name), kinds=("dominant", "one_swap"))
    return plan, 17, np.array([17, 17], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def zero_pivot_case():
    """five groups of the (28, 56) widths, groups 1 and 3 with a column that vanishes in M and in L"""
    plan = SyntheticPlan(20, 32, 16, 8, [61, 117, 40, 117, 200], 3, 4000, zero_column_groups=(1, 3))
    return plan, 20, np.array([20, 20, 20, 20, 20], dtype=np.int32), (1, 3)


def get_case(name, layout="default"):
    return single_group_case(name) if layout == "rows_by_slots" else case(name)


# ---- layouts ----------------------------------------------------------------------------------------------------------
def offsets(plan, nslots, layout):
    """-> (rowoff [nl][nmax], coloff, slot_stride, doubles of a system vector): element offsets of the permuted rows and
    columns inside slot 0.  default: [comp][slot][group][n] (what executor.EllBand derives itself); rows_by_slots: the
    [row][slot] vectors of executor.BorderedBandInverse, offsets = (i nslots, i nslots, 1)"""
    nl, nr = plan.nl, plan.nr
    if layout == "rows_by_slots":
        assert nl == 1 and plan.ncomp == 1
        return plan.row_index * nslots * (plan.row_index >= 0), plan.col_index * nslots * (plan.col_index >= 0), 1, nr * nslots
    g = np.arange(nl)[:, None]

    def off(idx):
        return np.where(idx >= 0, (idx // nr) * (nslots * nl * nr) + g * nr + idx % nr, 0)
    return off(plan.row_index), off(plan.col_index), nl * nr, plan.ncomp * nslots * nl * nr


@functools.lru_cache(maxsize=None)
def rhs_columns(name, layout="default"):
    """per group the (n, slot_limit) standard-normal right-hand sides in the permuted order (before T)"""
    plan, nslots, lim = get_case(name, layout)
    return random_columns(plan, lim, 77)


def random_columns(plan, lim, seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((int(plan.n[g]), int(lim[g]))) for g in range(plan.nl)]


def make_rhs(plan, nslots, lim, layout, cols):
    """the system vector: cols at the elements rowoff names for (g, i < n[g], s < slot_limit[g]), NaN everywhere else"""
    rowoff, _, stride, size = offsets(plan, nslots, layout)
    v = np.full(size, NAN)
    for g in range(plan.nl):
        n = int(plan.n[g])
        at = rowoff[g, :n, None] + np.arange(int(lim[g]))[None, :] * stride
        assert np.isnan(v[at]).all()                                 # no two (g, i, s) share an element
        v[at] = cols[g]
    return v


# ---- references -------------------------------------------------------------------------------------------------------
def ld_solve(A, r):
    """dense Gaussian elimination with partial pivoting in longdouble (rows without an entry in the column are skipped:
    they would subtract zeros)"""
    A, r = np.array(A, dtype=LD), np.array(r, dtype=LD)
    n = A.shape[0]
    for j in range(n):
        p = j + int(np.argmax(np.abs(A[j:, j])))
        if p != j:
            A[[j, p]], r[[j, p]] = A[[p, j]], r[[p, j]]
        rows = j + 1 + np.flatnonzero(A[j + 1:, j])
        l = A[rows, j] / A[j, j]
        A[rows, j:] -= l[:, None] * A[j, None, j:]
        r[rows] -= l[:, None] * r[j, None]
    for j in range(n - 1, -1, -1):
        r[j] = (r[j] - A[j, j + 1:] @ r[j + 1:]) / A[j, j]
    return r


def permuted_rhs(plan, g, cols, dtype=LD):
    """T applied to the first nbc_of[g] rows of the gathered right-hand side"""
    r = np.array(cols, dtype=dtype)
    k = int(plan.nbc_of[g])
    r[:k] = plan.T[g, :k, :k].astype(dtype) @ r[:k]
    return r


def apply_P(plan, g, y):
    n = int(plan.n[g])
    z = y.copy()
    for s in range(min(plan.mp, n - 1)):
        z[:n - 1 - s] += plan.P[g, :n - 1 - s, s, None].astype(y.dtype) * y[1 + s:]
    return z


def undo_P(plan, g, z):
    """y from z = P y in longdouble (P unit upper triangular: back substitution from the last row)"""
    n = int(plan.n[g])
    y = np.array(z, dtype=LD)
    Pg = plan.P[g, :n].astype(LD)
    for i in range(n - 2, -1, -1):
        m = min(plan.mp, n - 1 - i)
        if m:
            y[i] -= Pg[i, :m] @ y[i + 1:i + 1 + m]
    return y


def reference(plan, g, a, b, cols):
    """-> (y, z) in longdouble for the permuted right-hand sides cols (n, nrhs): the defined operation up to the scatter"""
    y = ld_solve(plan.dense(g, a, b), permuted_rhs(plan, g, cols))
    return y, apply_P(plan, g, y)


def band_lu(plan, g, a, b):
    """LAPACK dgbtrf of a M + b L -> (lu, piv, info)"""
    from scipy.linalg import lapack
    n, kl, ku = int(plan.n[g]), plan.kl, plan.ku
    A = a * plan.MB[g, :n] + b * plan.LB[g, :n]
    ab = np.zeros((2 * kl + ku + 1, n))
    i = np.arange(n)
    for d in range(kl + ku + 1):
        j = i - kl + d
        ok = (j >= 0) & (j < n)
        ab[kl + ku + i[ok] - j[ok], j[ok]] = A[i[ok], d]
    return lapack.dgbtrf(ab, kl, ku)


def baseline(plan, g, a, b, cols):
    """the same operation in float64 through dgbtrf / dgbtrs -> (y, z)"""
    from scipy.linalg import lapack
    lu, piv, info = band_lu(plan, g, a, b)
    assert info == 0
    y, info = lapack.dgbtrs(lu, plan.kl, plan.ku, permuted_rhs(plan, g, cols, np.float64), piv)
    assert info == 0
    return y, apply_P(plan, g, y)


def backward_error(plan, g, a, b, cols, y):
    """normwise eta = max over the columns of |A y - r|_inf / (|A|_inf |y|_inf + |r|_inf), in longdouble, on the permuted
    system before P"""
    A = plan.dense(g, a, b)
    r = permuted_rhs(plan, g, cols)
    y = np.asarray(y, dtype=LD)
    res = np.abs(A @ y - r).max(axis=0)
    den = np.abs(A).sum(axis=1).max() * np.abs(y).max(axis=0) + np.abs(r).max(axis=0)
    return float((res / den).max())


@functools.lru_cache(maxsize=None)
def solved(name, layout, a, b):
    """per live group with live slots: dict(y, z longdouble reference; yb, zb float64 baseline; eta_b; err_b) -- computed
    once and shared"""
    plan, nslots, lim = get_case(name, layout)
    return solve_all(plan, lim, rhs_columns(name, layout), a, b)


def solve_all(plan, lim, cols, a, b, skip=()):
    out = {}
    for g in range(plan.nl):
        if plan.n[g] == 0 or lim[g] == 0 or g in skip:
            continue
        y, z = reference(plan, g, a, b, cols[g])
        yb, zb = baseline(plan, g, a, b, cols[g])
        out[g] = dict(y=y, z=z, yb=yb, zb=zb, eta_b=backward_error(plan, g, a, b, cols[g], yb),
                      err_b=float(np.abs(zb - z).max() / np.abs(z).max()))
    return out


def pivot_offsets(piv):
    """dgbtrf's 0-based pivot rows -> offsets from the diagonal"""
    return np.asarray(piv) - np.arange(len(piv))


# ---- ddh_ellband_gather_complex_inverse -------------------------------------------------------------------------------
GATHER_SHAPES = ((1, 5, 5, 5), (3, 7, 4, 25), (2, 16, 20, 40), (4, 260, 2, 1040))       # (R, nl, nm, nslots)


def gather_offsets(R, nl, nm):
    """-> (off[m] in complex numbers, total count)"""
    sizes = np.array([(R * max(nl - m, 0)) ** 2 for m in range(nm)], dtype=np.int64)
    return np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64), int(sizes.sum())


def gather_complex_inverse(x, R, nl, nm, nslots, out):
    """The kernel's index map: x [2 R][nslots][nm][nl]; unknown j = c (nl - m) + (ell - m); row j of block m comes from
    slot (nl - 1 - ell) R + c, its column (cp, ellp) from components 2 cp / 2 cp + 1 at [m][ellp].  Fills the complex
    array out at off[m] and leaves everything else as it is."""
    x4 = np.asarray(x).reshape(2 * R, nslots, nm, nl)
    off, _ = gather_offsets(R, nl, nm)
    for m in range(min(nm, nl)):
        ne = nl - m
        blk = np.empty((R, ne, R, ne), dtype=np.complex128)
        for c in range(R):
            sl = (nl - 1 - (m + np.arange(ne))) * R + c
            for cp in range(R):
                blk[c, :, cp, :] = x4[2 * cp, sl, m, m:] + 1j * x4[2 * cp + 1, sl, m, m:]
        out[off[m]:off[m] + (R * ne) ** 2] = blk.reshape(-1)
    return out


# ---- ddh_ellband_bordered_inverse -------------------------------------------------------------------------------------
BORDERED_SIZES = (1, 2, 63, 64, 65, 255, 256, 300)


def bordered_inputs(n, j0):
    rng = np.random.default_rng(9000 + 7 * n + j0)
    X = rng.standard_normal((n, n))
    wM, wL = rng.standard_normal(n), rng.standard_normal(n)
    dM, dL, a, b = (float(v) for v in rng.standard_normal(4))
    return X, wM, wL, dM, dL, a, b


def bordered_row(X, wM, wL, dM, dL, a, b):
    """-> (row j0 of the inverse: -(w^T X) / d, 1 / d; its rounding scale sum_i |w_i| |X_is| / |d|), longdouble"""
    w = LD(a) * wM.astype(LD) + LD(b) * wL.astype(LD)
    d = LD(a) * LD(dM) + LD(b) * LD(dL)
    XL = X.astype(LD)
    return np.concatenate([-(w @ XL) / d, [1 / d]]), np.concatenate([np.abs(w) @ np.abs(XL) / abs(d), [abs(1 / d)]])


def bordered_system(n=130, kl=5, ku=6, seed=11):
    """M, L (n + 1)^2: a band block with the vanishing column j0, the gauge variable's column inside the band of column
    j0, a dense gauge row -> (M, L, j0)"""
    rng = np.random.default_rng(seed)
    j0 = n // 3
    i, j = np.indices((n + 1, n + 1))
    band = (i - j <= kl) & (j - i <= ku) & (i < n) & (j < n)
    out = []
    for _ in range(2):
        A = np.where(band, rng.standard_normal((n + 1, n + 1)), 0.0)
        A[:n, n] = np.where(band[:n, j0], rng.standard_normal(n), 0.0)
        A[:n, j0] = 0.0
        A[n, :] = rng.standard_normal(n + 1)
        out.append(A)
    return out[0], out[1], j0
