"""Synthetic COMPLEX plans, case table and high-precision references for the complex instances of the band LU kernels of
dedalus_amd/csrc/ddh_ellband.hip (ddh_ellband_create_complex, then factor / solve as for a real handle), importable
without a device.  Built on tests/ellband_cases.py: the same band widths, group sizes, layouts and real T / P; the
matrices get an independent standard-normal imaginary part on every entry of the band, and the slots of the real system
vectors are (re, im) pairs of complex right-hand sides.  tests/test_ellband_complex_cases_host.py proves the inputs and
the references; tests/test_gpu_ellband_complex_kernels.py runs the kernels on them.

`reference` is a dense partial-pivoting elimination in np.clongdouble, `baseline` LAPACK's zgbtrf / zgbtrs in complex128.
The complex handle compiles the windows (12, 24) (20, 40) (28, 56) (36, 64); a band that needs (36, 96) is refused."""
import functools

import numpy as np

import ellband_cases as ec

CLD = np.clongdouble
CX_VARIANTS = ec.VARIANTS[:4]
FORWARD_PAIRS, BACKWARD_PAIRS = 64, 16                   # pairs per wave of the two complex sweeps

# name (a row of ellband_cases.CASES: widths, mp, nbc, ncomp, sizes) -> pairs of slots.  Per compiled variant its widest
# case (ellband_cases.WIDEST) and a narrower one; pair counts on either side of 16 and 64.
CX_CASES = {
    "kl3_ku4": 1,
    "kl11_ku13": 15,
    "kl12_ku3": 17,
    "kl19_ku21": 65,
    "kl20_ku32": 64,
    "kl27_ku29": 16,
    "kl28_ku20": 63,
    "kl35_ku29": 17,
}
CX_WIDEST = ec.WIDEST[:4]
CX_CASE_LAYOUTS = [(name, lay) for name in CX_CASES for lay in ec.CASES[name][11]]
CX_REFUSED = ("kl35_ku30", "kl35_ku61")                  # the (36, 96) rows of the real table
ALIVE_CASE = ec.ALIVE_CASE


def _cdtype(dtype):
    return CLD if dtype in (ec.LD, CLD) else np.complex128


class ComplexPlan(ec.SyntheticPlan):
    """ellband_cases.SyntheticPlan with cx = True and complex128 MB / LB: the real plan of the same seed plus i times an
    independent standard-normal band on the entries the real band holds (scaled like the real part for the dominant
    kinds, so that the |re| + |im| column dominance stands; NaN rows stay NaN).  The imaginary part is redrawn until
    cond_2(a M + b L) <= COND_DRAW for both AB_PAIRS, as the real part was."""
    cx = True

    def __init__(self, kl, ku, mp, nbc, sizes, ncomp, seed, kinds=None, zero_column_groups=()):
        super().__init__(kl, ku, mp, nbc, sizes, ncomp, seed, kinds=kinds, zero_column_groups=zero_column_groups)
        rng = np.random.default_rng(seed + 500000)
        W = kl + ku + 1
        MB, LB = self.MB.astype(np.complex128), self.LB.astype(np.complex128)
        re_M, re_L = self.MB, self.LB
        for g, n in enumerate(sizes):
            kind = kinds[g] if kinds else "random"
            scale = 1.0 if kind == "random" else 1.0 / W
            for attempt in range(ec.COND_TRIES):
                iM = np.where(re_M[g, :n] != 0, rng.standard_normal((n, W)), 0.0) * scale
                iL = np.where(re_L[g, :n] != 0, rng.standard_normal((n, W)), 0.0) * scale
                if kind != "random":
                    iM[:, kl] = iL[:, kl] = 0.0
                MB[g, :n] = re_M[g, :n] + 1j * iM
                LB[g, :n] = re_L[g, :n] + 1j * iL
                self.MB, self.LB = MB, LB
                if n == 0 or kind != "random" or g in zero_column_groups:
                    break
                if max(np.linalg.cond(self.dense(g, a, b, np.float64)) for a, b in ec.AB_PAIRS) <= ec.COND_DRAW:
                    break
            else:
                raise AssertionError("no complex draw of group %d (n = %d) within the condition cap" % (g, n))
        self.MB, self.LB = MB, LB

    def dense(self, g, a, b, dtype=ec.LD):
        if self.MB.dtype.kind != "c":                      # (the base constructor conditions its real draw)
            return super().dense(g, a, b, dtype)
        dt = _cdtype(dtype)
        n, kl = int(self.n[g]), self.kl
        A = np.zeros((n, n), dtype=dt)
        B = dt(a) * self.MB[g, :n].astype(dt) + dt(b) * self.LB[g, :n].astype(dt)
        i = np.arange(n)
        for d in range(self.kl + self.ku + 1):
            j = i - kl + d
            ok = (j >= 0) & (j < n)
            A[i[ok], j[ok]] = B[i[ok], d]
        return A


def pair_limits(pairs, sizes, zero_n, one_n):
    """slot_limit[g] = 2 x ellband_cases.slot_limits in pairs: 0, 2, 40, 2 (pairs - 1), 2 pairs"""
    return (2 * ec.slot_limits(pairs, sizes, zero_n, one_n)).astype(np.int32)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (plan, nslots, slot_limit)"""
    kl, ku, nw, wt, mp, nbc, _, ncomp, nmax, zero_n, one_n, _ = ec.CASES[name]
    sizes = ec.group_sizes(nw, wt, nbc, nmax)
    plan = ComplexPlan(kl, ku, mp, nbc, sizes, ncomp, 1000 + list(ec.CASES).index(name))
    return plan, 2 * CX_CASES[name], pair_limits(CX_CASES[name], sizes, zero_n, one_n)


@functools.lru_cache(maxsize=None)
def single_group_case(name):
    kl, ku, nw, wt, mp, nbc, _, ncomp, nmax, zero_n, one_n, _ = ec.CASES[name]
    plan = ComplexPlan(kl, ku, mp, nbc, [min(2 * wt + 5, nmax)], 1, 2000 + list(ec.CASES).index(name))
    return plan, 2 * CX_CASES[name], np.array([2 * CX_CASES[name]], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def pivot_case(name):
    """group 0: no interchange at all, group 1: one interchange, at offset kl"""
    kl, ku, nw, wt, mp, nbc, _, ncomp, nmax, zero_n, one_n, _ = ec.CASES[name]
    n = min(2 * wt + 5, nmax)
    plan = ComplexPlan(kl, ku, mp, nbc, [n, n], ncomp, 3000 + list(ec.CASES).index(name), kinds=("dominant", "one_swap"))
    return plan, 34, np.array([34, 34], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def zero_pivot_case():
    plan = ComplexPlan(20, 32, 16, 8, [61, 117, 40, 117, 200], 3, 4000, zero_column_groups=(1, 3))
    return plan, 20, np.array([20, 20, 20, 20, 20], dtype=np.int32), (1, 3)


def get_case(name, layout="default"):
    return single_group_case(name) if layout == "rows_by_slots" else case(name)


# ---- right-hand sides -------------------------------------------------------------------------------------------------
def random_columns(plan, lim, seed):
    """per group the complex (n, slot_limit / 2) right-hand sides in the permuted order (before T)"""
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((int(plan.n[g]), int(lim[g]) // 2)) + 1j * rng.standard_normal((int(plan.n[g]), int(lim[g]) // 2))
            for g in range(plan.nl)]


@functools.lru_cache(maxsize=None)
def rhs_columns(name, layout="default"):
    plan, nslots, lim = get_case(name, layout)
    return random_columns(plan, lim, 77)


def to_slots(c):
    """complex (n, k) -> real (n, 2 k): slot 2 j = re, 2 j + 1 = im"""
    out = np.empty((c.shape[0], 2 * c.shape[1]), dtype=np.float64)
    out[:, 0::2], out[:, 1::2] = c.real, c.imag
    return out


def from_slots(x):
    return x[:, 0::2] + 1j * x[:, 1::2]


def make_rhs(plan, nslots, lim, layout, cols):
    return ec.make_rhs(plan, nslots, lim, layout, [to_slots(c) for c in cols])


# ---- references -------------------------------------------------------------------------------------------------------
def permuted_rhs(plan, g, cols, dtype=CLD):
    r = np.array(cols, dtype=dtype)
    k = int(plan.nbc_of[g])
    r[:k] = plan.T[g, :k, :k].astype(dtype) @ r[:k]
    return r


def ld_solve(A, r):
    """ellband_cases.ld_solve in clongdouble (pivot: largest modulus)"""
    A, r = np.array(A, dtype=CLD), np.array(r, dtype=CLD)
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


def reference(plan, g, a, b, cols):
    y = ld_solve(plan.dense(g, a, b), permuted_rhs(plan, g, cols))
    return y, ec.apply_P(plan, g, y)


def band_lu(plan, g, a, b):
    """LAPACK zgbtrf of a M + b L -> (lu, piv, info)"""
    from scipy.linalg import lapack
    n, kl, ku = int(plan.n[g]), plan.kl, plan.ku
    A = a * plan.MB[g, :n] + b * plan.LB[g, :n]
    ab = np.zeros((2 * kl + ku + 1, n), dtype=np.complex128)
    i = np.arange(n)
    for d in range(kl + ku + 1):
        j = i - kl + d
        ok = (j >= 0) & (j < n)
        ab[kl + ku + i[ok] - j[ok], j[ok]] = A[i[ok], d]
    return lapack.zgbtrf(ab, kl, ku)


def baseline(plan, g, a, b, cols):
    from scipy.linalg import lapack
    lu, piv, info = band_lu(plan, g, a, b)
    assert info == 0
    y, info = lapack.zgbtrs(lu, plan.kl, plan.ku, permuted_rhs(plan, g, cols, np.complex128), piv)
    assert info == 0
    return y, ec.apply_P(plan, g, y)


def backward_error(plan, g, a, b, cols, y):
    """normwise eta = max over the columns of |A y - r|_inf / (|A|_inf |y|_inf + |r|_inf) in clongdouble (moduli)"""
    A = plan.dense(g, a, b)
    r = permuted_rhs(plan, g, cols)
    y = np.asarray(y, dtype=CLD)
    res = np.abs(A @ y - r).max(axis=0)
    den = np.abs(A).sum(axis=1).max() * np.abs(y).max(axis=0) + np.abs(r).max(axis=0)
    return float((res / den).max())


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


@functools.lru_cache(maxsize=None)
def solved(name, layout, a, b):
    plan, nslots, lim = get_case(name, layout)
    return solve_all(plan, lim, rhs_columns(name, layout), a, b)
