"""Systems, masks and longdouble references for the kernels of dedalus_amd/csrc/ddh_dense.hip (batched Gauss-Jordan
inversion of a M + b L on valid-mode blocks) and for the per-ell GEMM chain of csrc/ddh_sphere.hip that consumes its
result.  Imports without a device: tests/test_dense_inverse_cases_host.py proves the inputs and the references on the
CPU, tests/test_gpu_dense_inverse_kernels.py runs the kernels on them.

One case is one DenseInverse handle, so its largest system -- and with it the kernel instance -- is fixed by the table:
    real,    nmax <= 768:   dense_inverse_kernel<false, 12>  (25 nmax doubles of LDS within the 150 KiB budget)
    real,    nmax <= 1024:  dense_inverse_kernel<false, 8>
    complex, nmax <= 1024:  dense_inverse_kernel<true, 4>
    n > 1024:               big_assemble / big_panel / big_update / big_unpivot, one system at a time, BS = 16
Every case holds an empty system (n = 0) between live ones, one small system without any valid row, and every mask
pattern.  The system lives on the valid block [rv] x [cv]; every other entry of M and L is NaN.

Two families of systems:
    n <= 320, "random":      M and L standard normal (complex: independent imaginary parts), no diagonal shift, redrawn
                             from the same generator until cond_2(a M + b L) <= 5e4 for both (a, b) pairs; the reference
                             is a partial-pivoting elimination in longdouble.
    n > 320, "structured":   M = D1 Pi + U1 V1^T, L = D2 Pi + U2 V2^T with one random permutation Pi, rank 4 and dyadic
                             entries (exact in float64, as is a M + b L for the dyadic pairs below, fused or not); the
                             reference is the Woodbury formula in longdouble, O(n^2 k)."""
import functools

import numpy as np

LD, CLD = np.longdouble, np.clongdouble
U = 2.0 ** -53

# ---- restated from csrc/ddh_dense.hip -----------------------------------------------------------------------------
DI_T = DI_NMAX = 1024
LDS_BUDGET = 150 * 1024
LDS_STATIC = 4296              # s_piv [1024] int, s_best [16] double, s_arg [16] int, s_p, s_bad
LDS_CU = 160 * 1024
BS_REAL_WIDE, BS_REAL, BS_COMPLEX = 12, 8, 4
RB = 8
BIG_BS = 16
BIG_RW = 64
GUARD = 16                     # NaN doubles behind the output

AB_PAIRS = ((1.0, 0.375), (0.0, 1.0))
SINGULAR_PAIRS = ((1.0, 0.0), (0.0, 1.0))       # a M + b L = M (singular in one system), then = L (regular in all)
COND_CAP = 1e5                 # cond_2(a M + b L) of every valid block, both pairs (the host test asserts it)
COND_DRAW = 5e4                # a random system is redrawn (same generator: still deterministic) until it is within this
COND_TRIES = 200
RANDOM_MAX = 320               # largest n of the random family
RANK = 4


def expected_bs(nmax, cx):
    """pending rank-1 updates of the single-workgroup kernel that ddh_dense_inverse_compute picks (nmax <= DI_NMAX)"""
    if cx:
        return BS_COMPLEX
    return BS_REAL_WIDE if (2 * BS_REAL_WIDE + 1) * nmax * 8 <= LDS_BUDGET else BS_REAL


def lds_bytes(nmax, cx):
    return (2 * expected_bs(nmax, cx) + 1) * nmax * (16 if cx else 8) + LDS_STATIC


# ---- the table: case -> (complex, ((n, mask pattern), ...)) ----------------------------------------------------------
# patterns: A all valid; S about 15 % of the rows invalid and as many columns at other places; F only row 0 and column
# n - 1 invalid; L only row n - 1 and column 0 invalid; N nothing valid (the result is all zeros, no singular flag)
CASES = {
    "real bs12 small": (False, ((1, "A"), (7, "S"), (8, "F"), (9, "L"), (12, "A"), (13, "S"), (16, "F"), (0, "A"), (17, "L"),
                                (24, "A"), (5, "N"), (31, "S"), (63, "F"), (64, "L"), (65, "A"))),
    "real bs12 768": (False, ((12, "A"), (24, "F"), (0, "A"), (768, "S"), (6, "N"), (16, "L"))),
    "real bs8 769": (False, ((8, "S"), (9, "F"), (15, "L"), (0, "A"), (769, "A"), (16, "S"), (4, "N"), (23, "F"))),
    "real bs8 1024": (False, ((24, "A"), (25, "S"), (0, "A"), (1024, "F"), (8, "L"), (9, "A"), (3, "N"))),
    "complex small": (True, ((1, "A"), (3, "S"), (4, "F"), (5, "L"), (8, "A"), (63, "S"), (64, "F"), (0, "A"), (65, "L"),
                             (2, "N"), (71, "A"), (127, "S"), (128, "F"), (129, "L"))),
    "complex 765": (True, ((3, "A"), (5, "S"), (0, "A"), (765, "L"), (4, "F"), (8, "N"))),
    "complex 1024": (True, ((8, "L"), (4, "N"), (0, "A"), (1024, "A"), (5, "F"), (3, "S"))),
    "real multi 1025": (False, ((17, "A"), (40, "F"), (1025, "S"), (0, "A"), (9, "N"), (31, "L"))),
    "real multi 1088": (False, ((12, "S"), (33, "L"), (1088, "A"), (0, "A"), (7, "N"), (16, "F"))),
    "complex multi 1040": (True, ((5, "A"), (20, "S"), (1040, "F"), (0, "A"), (6, "N"), (18, "L"))),
}
# every n the kernels' block edges ask for, per instance
REQUIRED_N = {
    "real bs12": (1, 7, 8, 9, 12, 13, 16, 17, 24, 31, 63, 64, 65, 768),
    "real bs8": (8, 9, 15, 16, 23, 24, 25, 769, 1024),
    "complex": (1, 3, 4, 5, 8, 63, 64, 65, 71, 127, 128, 129, 765, 1024),
    "real multi": (1025, 1088),
    "complex multi": (1040,),
}
SINGULAR_SETS = {            # set -> (complex, sizes and patterns, index of the singular system, how it is singular)
    "real single": (False, ((12, "A"), (33, "S"), (20, "S"), (9, "F")), 2, "zero column"),
    "complex single": (True, ((9, "F"), (70, "A"), (5, "S"), (16, "A")), 1, "equal rows"),
    "real multi 1025": (False, ((10, "A"), (1025, "A"), (24, "S"), (7, "L")), 1, "zero column"),
}


def instance(name):
    """which kernels a case runs: (label, BS the pivot coverage refers to)"""
    cx, systems = CASES[name] if name in CASES else SINGULAR_SETS[name][:2]
    nmax = max(n for n, _ in systems)
    if nmax > DI_NMAX:
        return ("complex multi" if cx else "real multi"), BIG_BS
    bs = expected_bs(nmax, cx)
    return ("complex" if cx else "real bs%d" % bs), bs


# ---- masks ------------------------------------------------------------------------------------------------------------
def masks(n, pattern, rng):
    rv, cv = np.ones(n, bool), np.ones(n, bool)
    if pattern == "S":
        k = max(1, int(round(0.15 * n)))
        rv[rng.permutation(n)[:k]] = False
        cv[rng.permutation(n)[:k]] = False
    elif pattern == "F":
        rv[0] = cv[n - 1] = False
    elif pattern == "L":
        rv[n - 1] = cv[0] = False
    elif pattern == "N":
        rv[:] = cv[:] = False
    elif pattern != "A":
        raise ValueError(pattern)
    return rv, cv


def scatter(block, rv, cv):
    """the valid block inside an n x n array of NaN"""
    n = rv.size
    nan = complex(np.nan, np.nan) if np.iscomplexobj(block) else np.nan
    full = np.full((n, n), nan, dtype=block.dtype)
    full[np.ix_(rv, cv)] = block
    return full


# ---- references -------------------------------------------------------------------------------------------------------
def ld_inverse(A, want_inverse=True):
    """inverse by Gaussian elimination with partial pivoting in longdouble / clongdouble on [A | I].
    -> (X, zero): zero is the first column whose pivot candidates are all exactly 0 (X is None then), else None;
    want_inverse=False eliminates A alone and returns (None, zero)"""
    dt = CLD if np.iscomplexobj(A) else LD
    n = A.shape[0]
    W = np.concatenate([np.array(A, dtype=dt), np.eye(n, dtype=dt)[:, :n if want_inverse else 0]], axis=1)
    for j in range(n):
        p = j + int(np.argmax(np.abs(W[j:, j])))
        if W[p, j] == 0:
            return None, j
        if p != j:
            W[[j, p]] = W[[p, j]]
        l = W[j + 1:, j] / W[j, j]
        W[j + 1:, j:] -= l[:, None] * W[j, None, j:]
    if not want_inverse:
        return None, None
    X = W[:, n:]
    for j in range(n - 1, -1, -1):
        X[j] = (X[j] - W[j, j + 1:n] @ X[j + 1:]) / W[j, j]
    return X, None


def ld_refine_dyadic(A, X):
    """One Newton step X + X (I - A X) whose residual is exact: for A with entries k / 2048, |A| <= 8 and n <= 256.
    X is split into a fixed-point part with 39 bits (A Xh then sums 63-bit integers on one grid: no rounding in
    longdouble's 64) and a remainder below 2^-39 max |X|, so the residual carries a relative error of 1e-31 and the step
    squares the error of X: what is left is the rounding of the result, 1e-19 relative -- the elimination alone is
    only good to cond * 1e-19."""
    n = A.shape[0]
    parts = lambda Z: (Z.real.astype(LD), Z.imag.astype(LD)) if np.iscomplexobj(Z) else (Z.astype(LD),)
    Ap, Xp = parts(A), parts(X)
    assert n <= 256 and all(np.array_equal(np.rint(P * 2048), P * 2048) and np.abs(P).max() <= 8 for P in Ap)
    g = LD(2.0) ** (int(np.ceil(np.log2(float(max(np.abs(P).max() for P in Xp))))) - 39)
    Xh = [np.rint(P / g) * g for P in Xp]
    Xl = [P - H for P, H in zip(Xp, Xh)]
    if len(Ap) == 1:
        R = (np.eye(n, dtype=LD) - Ap[0] @ Xh[0]) - Ap[0] @ Xl[0]
    else:
        (Ar, Ai), (Hr, Hi), (Lr, Li) = Ap, Xh, Xl
        Rr = ((np.eye(n, dtype=LD) - Ar @ Hr) + Ai @ Hi) - (Ar @ Lr - Ai @ Li)
        Ri = (-(Ar @ Hi) - Ai @ Hr) - (Ar @ Li + Ai @ Lr)
        R = Rr + 1j * Ri
    return X + X @ R


def combine(M, L, a, b):
    dt = CLD if np.iscomplexobj(M) else LD
    return LD(a) * M.astype(dt) + LD(b) * L.astype(dt)


def random_block(n, cx, rng, pairs=AB_PAIRS):
    for _ in range(COND_TRIES):
        M, L = rng.standard_normal((n, n)), rng.standard_normal((n, n))
        if cx:
            M = M + 1j * rng.standard_normal((n, n))
            L = L + 1j * rng.standard_normal((n, n))
        if n == 0 or all(np.linalg.cond(a * M + b * L) <= COND_DRAW for a, b in pairs):
            return M, L
    raise RuntimeError("no system of size %d within cond %g" % (n, COND_DRAW))


def _dyadic(rng, shape, cx, lo, hi, den, sign=False):
    def one():
        v = rng.integers(lo, hi + 1, shape).astype(np.float64) / den
        return v * rng.choice([-1.0, 1.0], shape) if sign else v
    return one() + 1j * one() if cx else one()


def structured_parts(n, cx, rng, pairs=AB_PAIRS):
    """(perm, d1, U1, V1, d2, U2, V2), float64 / complex128 with dyadic entries: D from +-{8..16}/8, U and V from {-8..8}/16"""
    perm = rng.permutation(n)
    for _ in range(COND_TRIES):
        d1, d2 = (_dyadic(rng, n, cx, 8, 16, 8.0, sign=True) for _ in range(2))
        if all(np.abs(a * d1 + b * d2).min() >= 0.25 for a, b in pairs):
            break
    else:
        raise RuntimeError("no diagonal away from zero")
    U1, V1, U2, V2 = (_dyadic(rng, (n, RANK), cx, -8, 8, 16.0) for _ in range(4))
    return perm, d1, U1, V1, d2, U2, V2


def structured_block(parts):
    """M and L of the parts in float64; the longdouble construction gives the same numbers (asserted: they are exact)"""
    perm, d1, U1, V1, d2, U2, V2 = parts
    n = perm.size
    out = []
    for d, Uk, Vk in ((d1, U1, V1), (d2, U2, V2)):
        A = Uk @ Vk.T
        A[np.arange(n), perm] += d
        dt = CLD if np.iscomplexobj(A) else LD
        Al = Uk.astype(dt) @ Vk.astype(dt).T
        Al[np.arange(n), perm] += d.astype(dt)
        assert np.array_equal(A.astype(dt), Al), "structured system is not exact in float64"
        out.append(A)
    return out[0], out[1]


def woodbury_inverse(parts, a, b):
    """(a M + b L)^-1 in longdouble: B = (a D1 + b D2) Pi, U = [a U1, b U2], V = [V1, V2],
    X = B^-1 - B^-1 U (I + V^T B^-1 U)^-1 V^T B^-1"""
    perm, d1, U1, V1, d2, U2, V2 = parts
    dt = CLD if np.iscomplexobj(d1) else LD
    n = perm.size
    a, b = LD(a), LD(b)
    dab = a * d1.astype(dt) + b * d2.astype(dt)
    Uc = np.concatenate([a * U1.astype(dt), b * U2.astype(dt)], axis=1)
    Vc = np.concatenate([V1.astype(dt), V2.astype(dt)], axis=1)
    BiU = np.zeros((n, 2 * RANK), dtype=dt)                 # B^-1 = Pi^T D^-1: row perm[i] of B^-1 U is U[i] / d[i]
    BiU[perm] = Uc / dab[:, None]
    VtBi = (Vc[perm] / dab[:, None]).T                      # column i of V^T B^-1 is V[perm[i]] / d[i]
    core, zero = ld_inverse(np.eye(2 * RANK, dtype=dt) + Vc.T @ BiU)
    assert zero is None
    X = -(BiU @ core) @ VtBi
    X[perm, np.arange(n)] += 1 / dab
    return X


# ---- systems ----------------------------------------------------------------------------------------------------------
class System:
    """one system of a batch: M, L (n x n, NaN outside the valid block), masks, and the valid blocks Mv, Lv"""

    def __init__(self, n, cx, pattern, rng, pairs=AB_PAIRS, family=None, singular=None):
        self.n, self.cx, self.pattern = n, cx, pattern
        self.rv, self.cv = masks(n, pattern, rng)
        self.nv = int(self.rv.sum())
        assert self.nv == int(self.cv.sum())
        self.family = family or ("random" if n <= RANDOM_MAX else "structured")
        self.parts = None
        if self.family == "random":
            self.Mv, self.Lv = random_block(self.nv, cx, rng, pairs)
        else:
            self.parts = structured_parts(self.nv, cx, rng, pairs)
            self.Mv, self.Lv = structured_block(self.parts)
        self.singular = singular
        if singular == "zero column":
            self.Mv[:, min(self.nv // 3, 40)] = 0
        elif singular == "equal rows":
            # two equal dyadic rows whose first entry 4 is the column's largest: the first elimination step picks one of
            # them, its multiplier for the other is 4 * (1 / 4) = 1 exactly and the difference of the rows is exactly 0
            i1, i2 = self.nv // 4, (3 * self.nv) // 4
            self.Mv[:, 0] *= 2.0 / np.abs(self.Mv[:, 0]).max()
            self.Mv[i1] = np.round(self.Mv[i1] * 16) / 16
            self.Mv[i1, 0] = 4.0
            self.Mv[i2] = self.Mv[i1]
        self.M, self.L = scatter(self.Mv, self.rv, self.cv), scatter(self.Lv, self.rv, self.cv)
        self._ref = {}

    def A64(self, a, b):
        return a * self.Mv + b * self.Lv

    def reference(self, a, b):
        """longdouble inverse of the valid block (nv x nv); None for a singular combination"""
        key = (float(a), float(b))
        if self.singular and a != 0:
            return None
        if key not in self._ref:
            if self.parts is not None:
                self._ref[key] = woodbury_inverse(self.parts, a, b)
            else:
                self._ref[key] = ld_inverse(combine(self.Mv, self.Lv, a, b))[0]
        return self._ref[key]

    def embedded(self, X):
        """the valid block's inverse inside n x n zeros: rows = valid columns, columns = valid rows"""
        out = np.zeros((self.n, self.n), dtype=X.dtype)
        out[np.ix_(self.cv, self.rv)] = X
        return out


def _seed(name):
    return [ord(c) for c in name]


@functools.lru_cache(maxsize=None)
def case(name):
    cx, systems = CASES[name]
    rng = np.random.default_rng(_seed(name))
    return tuple(System(n, cx, pat, rng) for n, pat in systems)


@functools.lru_cache(maxsize=None)
def singular_set(name):
    cx, systems, bad, how = SINGULAR_SETS[name]
    rng = np.random.default_rng(_seed("singular " + name))
    return tuple(System(n, cx, pat, rng, pairs=SINGULAR_PAIRS, singular=how if i == bad else None)
                 for i, (n, pat) in enumerate(systems))


@functools.lru_cache(maxsize=None)
def structured_check_system(n, cx):
    """a structured system small enough for the elimination: Woodbury and elimination must agree"""
    return System(n, cx, "A", np.random.default_rng([n, int(cx)]), family="structured")


def lapack_error(sysm, a, b):
    """(err_lapack, max |X_ref|): numpy.linalg.inv of the float64 a M + b L beside the longdouble reference"""
    X = sysm.reference(a, b)
    scale = float(np.abs(X).max())
    return float(np.abs(np.linalg.inv(sysm.A64(a, b)) - X).max()) / scale, scale


def residual(sysm, a, b, rows=40):
    """max |A X_ref - I| in longdouble, over all rows of a small system and `rows` spread rows of a large one"""
    X = sysm.reference(a, b)
    A = combine(sysm.Mv, sysm.Lv, a, b)
    pick = np.arange(sysm.nv) if sysm.nv <= RANDOM_MAX else np.unique(np.linspace(0, sysm.nv - 1, rows).astype(int))
    R = A[pick] @ X
    R[np.arange(pick.size), pick] -= 1
    return float(np.abs(R).max())


def cond_inf(sysm, a, b):
    A = combine(sysm.Mv, sysm.Lv, a, b)
    return float(np.abs(A).sum(axis=1).max() * np.abs(sysm.reference(a, b)).sum(axis=1).max())


def getrf_pivots(A):
    """LAPACK's row interchanges: piv[k] = the row exchanged with row k at step k"""
    import scipy.linalg
    return scipy.linalg.lu_factor(A, check_finite=False)[1]


# ---- the per-ell GEMM chain (csrc/ddh_sphere.hip: ell_blocks_kernel, ell_prune_kernel, ell_gemm_kernel) ----------------
EG_M, EG_N, EG_K = 64, 128, 64
GEMM_SHAPES = ((66, 67, 64, 2), (64, 65, 64, 1), (8, 9, 128, 3))            # (nm, nl, nr, ncomp)


def live_slots(nm, nl):
    """[2 nm][nl] bool: slot i1 of ell is live iff i1 / 2 <= ell"""
    i1, ell = np.indices((2 * nm, nl))
    return i1 // 2 <= ell


@functools.lru_cache(maxsize=None)
def gemm_inputs(nm, nl, nr, ncomp):
    """flat [nl][ncomp nr][ncomp nr] in three fillings, x [ncomp][2 nm][nl][nr] (NaN in the dead slots), y0 for the
    accumulating form.  Filling 0: block (0, 1) is zero for every ell and block (1, 0) for every ell but the last.
    Filling 1 (the refill): (0, 1) is non-zero and the formerly full (0, 0) is empty.  Filling 2: as 0 with every block of
    the last output component empty.  With one component there is one block, and it stays full."""
    rng = np.random.default_rng([nm, nl, nr, ncomp])
    N = ncomp * nr
    blk = lambda c: slice(c * nr, (c + 1) * nr)
    f0 = rng.standard_normal((nl, N, N))
    f1 = rng.standard_normal((nl, N, N))
    if ncomp > 1:
        f0[:, blk(0), blk(1)] = 0.0
        f0[:-1, blk(1), blk(0)] = 0.0
        f1[:, blk(0), blk(0)] = 0.0
    f2 = f0.copy()
    if ncomp > 1:
        f2[:, blk(ncomp - 1), :] = 0.0
    x = rng.standard_normal((ncomp, 2 * nm, nl, nr))
    x[:, ~live_slots(nm, nl)] = np.nan
    y0 = rng.standard_normal((ncomp, 2 * nm, nl, nr))
    for a in (f0, f1, f2, x, y0):
        a.setflags(write=False)
    return (f0, f1, f2), x, y0


def gemm_reference(flat, x, nm, nl, nr, ncomp):
    """y [ncomp][2 nm][nl][nr] in longdouble on the live slots, 0 on the dead ones"""
    live = live_slots(nm, nl)
    y = np.zeros(x.shape, dtype=LD)
    for l in range(nl):
        s = np.flatnonzero(live[:, l])
        xv = x[:, s, l, :].astype(LD).transpose(0, 2, 1).reshape(ncomp * nr, s.size)
        yv = flat[l].astype(LD) @ xv
        y[:, s, l, :] = yv.reshape(ncomp, nr, s.size).transpose(0, 2, 1)
    return y


@functools.lru_cache(maxsize=None)
def gemm_references(nm, nl, nr, ncomp):
    flats, x, _ = gemm_inputs(nm, nl, nr, ncomp)
    return tuple(gemm_reference(f, x, nm, nl, nr, ncomp) for f in flats)


# the whole chain: DenseInverse -> make_ell_terms_from_dense -> apply
CHAIN_SHAPE = (5, 9, 64, 2)                                  # (nm, nl, nr, ncomp): 128 x 128 per ell
CHAIN_GROUPS = {0: "A", 3: "S", 4: "F", 8: "L"}             # ell -> mask pattern; every other ell has no valid row


@functools.lru_cache(maxsize=None)
def chain_systems():
    nm, nl, nr, ncomp = CHAIN_SHAPE
    rng = np.random.default_rng(_seed("chain"))
    return tuple(System(ncomp * nr, False, CHAIN_GROUPS.get(l, "N"), rng) for l in range(nl))


# the sphere's route: complex per-m inverses copied into a CgemvBatch
SPHERE_SHAPE = (5, 7, 3)                                     # (nm, nl, ncomp): n_m = 3 (7 - m) = 21, 18, 15, 12, 9
SPHERE_PATTERNS = ("A", "S", "F", "L", "S")


@functools.lru_cache(maxsize=None)
def sphere_systems():
    nm, nl, ncomp = SPHERE_SHAPE
    rng = np.random.default_rng(_seed("sphere"))
    return tuple(System(ncomp * (nl - m), True, SPHERE_PATTERNS[m], rng) for m in range(nm))
