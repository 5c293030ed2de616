"""Synthetic plans, case tables and high-precision references for the kernels of dedalus_amd/csrc/ddh_swsh.hip (the grouped
colatitude transform behind ddh_grouped_mmt_forward / backward / set_pairs and ddh_regularity_recombine), importable
without a device.  tests/test_swsh_cases_host.py proves the inputs, the references and the coverage of the tables;
tests/test_gpu_swsh_kernels.py runs the kernels on them.

The kernel is a grouped matrix product, so the cases need no harmonics.  Per matrix key an independent standard-normal
forward matrix F [n_ell][n_grid] and backward matrix B [n_grid][n_ell] (B is NOT F^T and neither is symmetric under
t -> N-1-t: the real SWSH matrices hide a reversed contraction index, a swapped matrix offset and a wrong mirrored sign).
The defined operation of a group (key, g_start, c_start, count, ell_start, ell_step, n_ell), j < count:
    forward    c[o, c_start+j, ell_start + ell_step i, x] = sum_t F[i, t] g[o, g_start+j, t, x]
    backward   g[o, g_start+j, t, x] = sum_i B[t, i] c[o, c_start+j, ell_start + ell_step i, x]
    key without a matrix: forward writes nothing, backward writes +0.0
    pair mode 1: the same products on the partner's slices
    pair mode 2: the partner uses F2[i, t] = (-1)^(ell_start+i+parity) F[i, N-1-t], B2[t, i] = (-1)^(ell_start+i+parity) B[N-1-t, i]
F2 / B2 are built explicitly here and every pair is expanded into one more plain product, so the reference shares no index
logic with the kernel.  References are np.longdouble; beside every value comes its scale S = sum |a_k| |x_k|.

Inputs are NaN wherever the operation names no element (slices of no group, coefficient rows outside a group's ell
range, everything of a group without a matrix)."""
import functools
import math
import zlib

import numpy as np

LD = np.longdouble
NAN = float("nan")
# the references need more than float64: x87 extended (eps 2^-63) or better; otherwise exact products summed by math.fsum
LD_OK = bool(np.finfo(np.longdouble).eps <= 2.0 ** -63)

# ---- restated from dedalus_amd/csrc/ddh_swsh.hip ----------------------------------------------------------------------
GV_COLS, GV_ROWS, GV_WAVES, LANES = 8, 4, 4, 64            # GEMV: at most 8 columns, 4 rows per wave, 4 waves, 64 lanes
GV_WIDTHS = (2, 4, 8)                                       # compiled column widths
GT_I, GT_X, GT_J = 32, 64, 16                               # LDS GEMM tile: rows x columns, contraction step
GM_M, GM_N, GM_K, GM_STRIP, GM_KSTEP = 64, 64, 32, 16, 4   # MFMA GEMM tile, contraction chunk, rows per wave, k per MFMA
MFMA_MIN_N3 = 16
REG_T = (64, 128, 256)                                      # regularity_kernel: threads per block


def path_of(ncols, n3):
    """launch_grouped: chosen from ncols = n0 max_count n3 and n3 only"""
    if ncols <= GV_COLS:
        return "gemv"
    return "mfma" if n3 >= MFMA_MIN_N3 else "lds"


def gemv_width(ncols):
    return 2 if ncols <= 2 else 4 if ncols <= 4 else 8


def regularity_threads(n3):
    return 256 if n3 >= 256 else 128 if n3 > 64 else 64


# ---- case tables ------------------------------------------------------------------------------------------------------
NELL = (1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 67)      # one group each, in every case
N2C = 71                                                                        # coefficient rows
FOLDED_NELL, FOLDED_START = 17, 25                                              # ell_step = -1: rows 25 down to 9
NO_MATRIX_KEY = 999

# name: (n_grid, n0, max_count, n3, pairing).  pairing: none / mode1 / mode2 (every group that can be paired is, the
# mode-2 groups with alternating parity) / mixed (unpaired, mode 1 and mode 2 in turn).  The folded group is never paired
# (set_pairs refuses it), the group without a matrix is paired in every paired plan.
CASES = {
    # GEMV: ncols <= 8
    "gemv_n5_c1":        (5, 1, 1, 1, "none"),
    "gemv_n63_c2_m1":    (63, 1, 2, 1, "mode1"),
    "gemv_n64_c3_m2":    (64, 1, 3, 1, "mode2"),
    "gemv_n65_c4_mix":   (65, 2, 2, 1, "mixed"),
    "gemv_n130_c5":      (130, 1, 1, 5, "none"),
    "gemv_n130_c8_m2":   (130, 2, 2, 2, "mode2"),
    "gemv_n65_c3":       (65, 1, 3, 1, "none"),
    "gemv_n5_c6_mix":    (5, 1, 3, 2, "mixed"),
    "gemv_n64_c2":       (64, 2, 1, 1, "none"),
    "gemv_n63_c5_m1":    (63, 5, 1, 1, "mode1"),
    # LDS GEMM: ncols > 8, n3 < 16
    "lds_n15_c9":        (15, 3, 3, 1, "none"),
    "lds_n16_c63":       (16, 7, 3, 3, "none"),
    "lds_n17_c64":       (17, 32, 2, 1, "none"),
    "lds_n65_c65":       (65, 5, 1, 13, "none"),
    "lds_n16_c130":      (16, 5, 2, 13, "none"),
    "lds_n17_c45":       (17, 1, 3, 15, "none"),
    # MFMA GEMM: n3 >= 16
    "mfma_n3_x16":       (3, 1, 3, 16, "none"),
    "mfma_n31_x17":      (31, 2, 2, 17, "none"),
    "mfma_n32_x63":      (32, 1, 1, 63, "none"),
    "mfma_n33_x64":      (33, 2, 1, 64, "none"),
    "mfma_n65_x65":      (65, 1, 2, 65, "none"),
    "mfma_n130_x130":    (130, 1, 2, 130, "none"),
}
# out overlapping in: one forward and one backward run per path (and one through the paired GEMV)
ALIAS_CASES = ("gemv_n65_c3", "gemv_n65_c4_mix", "lds_n16_c63", "mfma_n33_x64")

# what the tables must contain, per path (the host test derives the right-hand sides from CASES)
REQUIRED = {
    "gemv": dict(n_grid={5, 63, 64, 65, 130}, ncols={1, 2, 3, 4, 5, 8}, pairing={"none", "mode1", "mode2", "mixed"}),
    "lds": dict(n_grid={15, 16, 17, 65}, ncols={9, 63, 64, 65, 130}, n3={1, 3, 13, 15}),
    "mfma": dict(n_grid={3, 31, 32, 33, 65, 130}, n3={16, 17, 63, 64, 65, 130}, n0={1, 2}),
}


def case_path(name):
    n_grid, n0, mc, n3, pairing = CASES[name]
    return path_of(n0 * mc * n3, n3)


class SyntheticPlan:
    """What HipExecutor.make_grouped_mmt / GroupedMmt.set_pairs take (groups, keys, fwd, bwd, pair arrays) and the array
    extents n1g, n1c, n2c."""

    def __init__(self, name):
        self.name = name
        self.n_grid, self.n0, self.max_count, self.n3, self.pairing = CASES[name]
        self.ncols = self.n0 * self.max_count * self.n3
        self.path = path_of(self.ncols, self.n3)
        rng = np.random.default_rng(zlib.crc32(name.encode()))
        N, mc = self.n_grid, self.max_count
        self.keys = [100 + i for i in range(len(NELL))]
        self.fwd = [rng.standard_normal((ne, N)) for ne in NELL]
        self.bwd = [rng.standard_normal((N, ne)) for ne in NELL]
        rows = [dict(key=100 + i, count=1 + i % mc, ell_start=(5 * i) % (N2C - ne + 1), ell_step=1, n_ell=ne)
                for i, ne in enumerate(NELL)]
        rows.append(dict(key=100 + NELL.index(FOLDED_NELL), count=mc, ell_start=FOLDED_START, ell_step=-1, n_ell=FOLDED_NELL))
        rows.append(dict(key=NO_MATRIX_KEY, count=min(2, mc), ell_start=0, ell_step=1, n_ell=0))
        flips = 0
        for i, r in enumerate(rows):
            if r["ell_step"] < 0 or self.pairing == "none":
                r["mode"] = 0
            elif self.pairing == "mixed":
                r["mode"] = 2 if r["key"] == NO_MATRIX_KEY else i % 3
            else:
                r["mode"] = 1 if self.pairing == "mode1" else 2
            r["parity"] = 0
            if r["mode"] == 2:
                r["parity"], flips = flips & 1, flips + 1
        rows = [rows[k] for k in rng.permutation(len(rows))]            # groups not in the order of their matrices
        # slices: every block (a group's `count` slices, and as many for its partner) at a shuffled place, a slice of
        # no group in front, behind every third block and at the end; grid and coefficient sides shuffled apart
        blocks = [(k, which) for k, r in enumerate(rows) for which in (("p", "q") if r["mode"] else ("p",))]
        for side in ("g", "c"):
            pos = 1
            for n, b in enumerate(rng.permutation(len(blocks))):
                k, which = blocks[b]
                rows[k][side + which] = pos
                pos += rows[k]["count"] + (n % 3 == 2)
            setattr(self, "n1" + side, pos + 1)
        self.n2c = N2C
        self.rows = rows
        self.groups = np.array([(r["key"], r["gp"], r["cp"], r["count"], r["ell_start"], r["ell_step"], r["n_ell"])
                                for r in rows], dtype=np.int64)
        self.paired = self.pairing != "none"
        self.pair_g = [r.get("gq", -1) for r in rows]
        self.pair_c = [r.get("cq", -1) for r in rows]
        self.pair_mode = [r["mode"] for r in rows]
        self.parity = [r["parity"] for r in rows]
        self.gshape = (self.n0, self.n1g, self.n_grid, self.n3)
        self.cshape = (self.n0, self.n1c, self.n2c, self.n3)

    def matrices(self, key):
        """(F, B) of a key, (None, None) for a key that owns no matrix"""
        if key not in self.keys:
            return None, None
        return self.fwd[self.keys.index(key)], self.bwd[self.keys.index(key)]

    def products(self):
        """every plain product of the plan: (F, B, g_start, c_start, count, coefficient rows), pairs expanded, the
        mirrored partner with its own explicitly built matrices; F = B = None without a matrix"""
        out = []
        for r in self.rows:
            F, B = self.matrices(r["key"])
            ells = r["ell_start"] + r["ell_step"] * np.arange(r["n_ell"])
            out.append((F, B, r["gp"], r["cp"], r["count"], ells))
            if r["mode"] == 0:
                continue
            if F is not None and r["mode"] == 2:
                F, B = mirrored(F, B, r["ell_start"], r["parity"])
            out.append((F, B, r["gq"], r["cq"], r["count"], ells))
        return out


def mirrored(F, B, ell_start, parity):
    """the matrices pair mode 2 applies to the partner"""
    sign = np.where((ell_start + np.arange(F.shape[0]) + parity) % 2 == 1, -1.0, 1.0)
    return sign[:, None] * F[:, ::-1], sign[None, :] * B[::-1, :]


@functools.lru_cache(maxsize=None)
def plan(name):
    return SyntheticPlan(name)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """-> (g, c): standard normal where a product reads, NaN everywhere else.  Do not modify."""
    p = plan(name)
    rng = np.random.default_rng(zlib.crc32(name.encode()) + 1)
    g, c = np.full(p.gshape, NAN), np.full(p.cshape, NAN)
    for F, B, g0, c0, cnt, ells in p.products():
        if F is None:
            continue
        assert np.isnan(g[:, g0:g0 + cnt]).all() and np.isnan(c[:, c0:c0 + cnt][:, :, ells]).all()     # nothing shared
        g[:, g0:g0 + cnt] = rng.standard_normal((p.n0, cnt, p.n_grid, p.n3))
        c[:, c0:c0 + cnt, ells] = rng.standard_normal((p.n0, cnt, len(ells), p.n3))
    g.setflags(write=False)
    c.setflags(write=False)
    return g, c


# ---- references -------------------------------------------------------------------------------------------------------
def _two_product(a, b):
    """a b = p + e exactly (Veltkamp / Dekker), elementwise float64"""
    p = a * b
    def split(v):
        t = 134217729.0 * v
        hi = t - (t - v)
        return hi, v - hi
    ah, al = split(a)
    bh, bl = split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def product_and_scale(A, X):
    """A [r][k] times X [..., k, x] along k -> (A X, |A| |X|), longdouble; without an extended longdouble: float64 values
    of the exactly rounded sums (math.fsum over error-free products)"""
    if LD_OK:
        return np.matmul(A.astype(LD), X.astype(LD)), np.matmul(np.abs(A).astype(LD), np.abs(X).astype(LD))
    A, X = np.asarray(A, dtype=np.float64), np.asarray(X, dtype=np.float64)
    Xm = np.moveaxis(X, -2, -1)                                         # [..., x, k]
    ref = np.empty(Xm.shape[:-1] + (A.shape[0],))
    for idx in np.ndindex(*Xm.shape[:-1]):
        for r in range(A.shape[0]):
            p, e = _two_product(A[r], Xm[idx])
            ref[idx + (r,)] = math.fsum(np.concatenate([p, e]))
    return np.moveaxis(ref, -1, -2).astype(LD), np.matmul(np.abs(A), np.abs(X)).astype(LD)


@functools.lru_cache(maxsize=None)
def forward_reference(name):
    """-> dict(ref, S longdouble [cshape], K int [cshape], named bool [cshape]).  Unnamed elements hold 0."""
    p = plan(name)
    g, _ = inputs(name)
    out = dict(ref=np.zeros(p.cshape, LD), S=np.zeros(p.cshape, LD), K=np.zeros(p.cshape, np.int64),
               named=np.zeros(p.cshape, bool))
    for F, B, g0, c0, cnt, ells in p.products():
        if F is None:
            continue
        r, s = product_and_scale(F, g[:, g0:g0 + cnt])
        assert not out["named"][:, c0:c0 + cnt][:, :, ells].any()
        out["ref"][:, c0:c0 + cnt, ells], out["S"][:, c0:c0 + cnt, ells] = r, s
        out["K"][:, c0:c0 + cnt, ells], out["named"][:, c0:c0 + cnt, ells] = p.n_grid, True
    return out


@functools.lru_cache(maxsize=None)
def backward_reference(name):
    """-> dict(ref, S, K, named [gshape], zero bool [gshape]: the slices backward fills with +0.0)"""
    p = plan(name)
    _, c = inputs(name)
    out = dict(ref=np.zeros(p.gshape, LD), S=np.zeros(p.gshape, LD), K=np.zeros(p.gshape, np.int64),
               named=np.zeros(p.gshape, bool), zero=np.zeros(p.gshape, bool))
    for F, B, g0, c0, cnt, ells in p.products():
        assert not (out["named"] | out["zero"])[:, g0:g0 + cnt].any()
        if B is None:
            out["zero"][:, g0:g0 + cnt] = True
            continue
        r, s = product_and_scale(B, c[:, c0:c0 + cnt][:, :, ells])
        out["ref"][:, g0:g0 + cnt], out["S"][:, g0:g0 + cnt] = r, s
        out["K"][:, g0:g0 + cnt], out["named"][:, g0:g0 + cnt] = len(ells), True
    return out


# ---- regularity recombination -----------------------------------------------------------------------------------------
REG_NCOMP = (1, 3, 9)
REG_N12 = (3, 5)
REG_N3 = (1, 63, 64, 65, 128, 129, 255, 256, 257, 600)
REG_NMATS = 5                                     # the last matrix is NaN and no slot names it


@functools.lru_cache(maxsize=None)
def regularity_inputs(ncomp, n3):
    """-> (data [ncomp][n1][n2][n3], slot_map [n1][n2] with -1 entries, mats [nmats][ncomp][ncomp], fac [n3]).  A scalar
    (ncomp = 1) has no recombination, Q = 1: its matrices are ones.  Do not modify."""
    rng = np.random.default_rng(7000 + 1000 * ncomp + n3)
    n1, n2 = REG_N12
    data = rng.standard_normal((ncomp, n1, n2, n3))
    slot_map = ((3 * np.arange(n1 * n2) + n3) % (REG_NMATS - 1)).reshape(n1, n2).astype(np.int32)
    slot_map[0, 1] = slot_map[1, 3] = slot_map[2, 0] = slot_map[2, 4] = -1
    mats = rng.standard_normal((REG_NMATS, ncomp, ncomp)) if ncomp > 1 else np.ones((REG_NMATS, 1, 1))
    mats[REG_NMATS - 1] = NAN
    fac = rng.standard_normal(n3) + np.where(np.arange(n3) % 2, 1.5, -1.5)
    for a in (data, slot_map, mats, fac):
        a.setflags(write=False)
    return data, slot_map, mats, fac


def regularity_reference(data, slot_map, mats, fac):
    """per live slot f[x] (Q[slot] @ v), per dead slot f[x] v (fac None: f = 1) -> (ref, S = |f| sum |q| |v|), longdouble"""
    ref, S = np.array(data, dtype=LD), np.abs(np.array(data, dtype=LD))
    for i1 in range(data.shape[1]):
        for i2 in range(data.shape[2]):
            k = int(slot_map[i1, i2]) if slot_map is not None else -1
            if k >= 0:
                ref[:, i1, i2], S[:, i1, i2] = product_and_scale(mats[k], data[:, i1, i2])
    if fac is not None:
        f = np.asarray(fac).astype(LD)
        ref, S = ref * f, S * np.abs(f)
    return ref, S
