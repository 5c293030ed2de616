"""Case tables and high-precision references for the streaming grid kernels of dedalus_amd/csrc/ddh_grid.hip (lincomb,
bilinear, the two CFL reductions, scatter, the pack / unpack pairs around the all-to-all), importable without a device.
tests/test_grid_cases_host.py checks the references against oracle/np_executor.py and the classification of every case;
tests/test_gpu_grid_kernels.py runs the kernels on the cases.

References take and return NumPy arrays.  Sums accumulate in np.longdouble and are returned in it; re-orderings and the
scatters are exact in float64 (one IEEE operation per entry at most) and are returned in float64.

Every case names the launch-shape class it is meant to reach as a tuple of tags.  `stream_tags`, `cfl_tags` and
`segment_tags` recompute the tags from the shape and the constants below, which restate what the kernel source fixes: a
later edit of a size that silently leaves a branch shows up as a mismatch in the host test."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53                      # unit round-off of float64

# ---- launch shapes restated from dedalus_amd/csrc/ddh_grid.hip --------------------------------------------------------
STREAM_THREADS = 256                # dim3(256) of every launch in the file (__launch_bounds__(256))
STREAM_MAX_BLOCKS = 2048            # stream_grid(): `if (blocks > 256 * 8) blocks = 256 * 8`
STREAM_PASS = STREAM_MAX_BLOCKS * STREAM_THREADS      # work items one grid-stride pass covers at the cap (524288)
LINCOMB_MAX_TERMS = 16              # MAX_TERMS
BILINEAR_MAX_TERMS = 32             # MAX_BIL
BILINEAR_MAX_OUT = 9                # ddh_grid_bilinear: `if (ncomp_out > 9) return fail(...)`; instantiations 1, 3, 9
SEG_WORDS_PER_CHUNK = 1024          # seg_grid(): cx = (seg_doubles / 2 + 1023) / 1024 chunks of 16-byte words
SEG_WORKGROUP_TARGET = 16384        # seg_grid(): `while (cx > 1 && cx * nseg > 16384) cx = (cx + 1) / 2`
SEG_CX_CAP = 1024                   # seg_grid(): `if (cx > 1024) cx = 1024`
SEG_GRID_Y_CAP = 65535              # seg_grid(): gridDim.y = min(nseg, 65535), the kernels loop `r += gridDim.y`
SEG_UNROLL = 4                      # copy_segment(): `for (; i + 3 * nth < n2; i += 4 * nth)`, nth = cx * 256
GUARD = 64                          # doubles of NaN past the end of every output buffer of the GPU tests
MAX_BUFFER_BYTES = 256 * 10 ** 6    # largest single buffer of a case (one documented exception: CX_HALVED_EXCEPTION)
HOST_LIMIT = 1 << 22                # cases up to this many doubles per buffer are cross-checked against NumpyExecutor


# ---- references -------------------------------------------------------------------------------------------------------
def lincomb(xs, alphas):
    """-> (sum_t alpha_t x_t, sum_t |alpha_t x_t|) in longdouble"""
    acc = np.zeros(np.shape(xs[0]), dtype=LD)
    mag = np.zeros(np.shape(xs[0]), dtype=LD)
    for x, a in zip(xs, alphas):
        p = LD(a) * np.asarray(x, dtype=LD)
        acc += p
        mag += np.abs(p)
    return acc, mag


def bilinear(ncomp_out, a, b, npts, terms):
    """out[ic] = sum_t coef_t a[ia_t] b[ib_t] -> (out, sum of |coef a b| per output, terms per output), longdouble"""
    a2 = np.asarray(a, dtype=LD).reshape(-1, npts)
    b2 = np.asarray(b, dtype=LD).reshape(-1, npts)
    out = np.zeros((ncomp_out, npts), dtype=LD)
    mag = np.zeros((ncomp_out, npts), dtype=LD)
    count = np.zeros(ncomp_out, dtype=int)
    for (ic, ia, ib, cf) in terms:
        p = LD(cf) * a2[ia] * b2[ib]
        out[ic] += p
        mag[ic] += np.abs(p)
        count[ic] += 1
    return out, mag, count


def cfl_field(u, ncomp, shape, inv_spacings, comp_axis):
    """sum_c |u_c| / dx_c on the grid, longdouble (NaN where a velocity is NaN)"""
    ug = np.abs(np.asarray(u, dtype=LD).reshape((ncomp,) + tuple(shape)))
    f = np.zeros(tuple(shape), dtype=LD)
    for c in range(ncomp):
        sh = [1] * len(shape)
        sh[comp_axis[c]] = -1
        f = f + ug[c] * np.asarray(inv_spacings[c], dtype=LD).reshape(sh)
    return f


def cfl_max(u, ncomp, shape, inv_spacings, comp_axis):
    """np.max of the field: NaN as soon as one point is NaN"""
    return cfl_field(u, ncomp, shape, inv_spacings, comp_axis).max()


def cfl_field_spherical(u, inv_h, inv_dr):
    u = np.asarray(u, dtype=LD)
    return np.sqrt(u[0] * u[0] + u[1] * u[1]) * np.asarray(inv_h, dtype=LD) + np.abs(u[2]) * np.asarray(inv_dr, dtype=LD)


def cfl_max_spherical(u, inv_h, inv_dr):
    return np.max(cfl_field_spherical(u, inv_h, inv_dr))


def scatter_add(y, idx, vals):
    """unique indices: one float64 addition per touched entry (exact reference, no extended precision needed)"""
    assert len(np.unique(idx)) == len(idx)
    out = np.array(y, dtype=np.float64).reshape(-1)
    out[np.asarray(idx)] += np.asarray(vals, dtype=np.float64)
    return out


def scatter_set(y, idx, vals):
    assert len(np.unique(idx)) == len(idx)
    out = np.array(y, dtype=np.float64).reshape(-1)
    out[np.asarray(idx)] = np.asarray(vals, dtype=np.float64)
    return out


def a2a_pack(src, outer, na, nb, inner, P):
    """[outer][na][nb][inner] -> [P][outer][na / P][nb][inner]"""
    s = np.asarray(src).reshape(outer, P, na // P, nb * inner)
    return np.ascontiguousarray(s.transpose(1, 0, 2, 3)).reshape(-1)


def a2a_unpack(src, outer, na, nb, inner, P):
    """[P][outer][na][nb / P][inner] -> [outer][na][nb][inner]"""
    s = np.asarray(src).reshape(P, outer, na, nb // P, inner)
    return np.ascontiguousarray(s.transpose(1, 2, 0, 3, 4)).reshape(-1)


def block_bounds(n, P, block=0):
    """rank p owns [lo[p], lo[p + 1]) of an axis of length n dealt out in blocks of `block` (0: ceil(n / P))"""
    B = block if block else -(-n // P)
    return [min(p * B, n) for p in range(P + 1)]


def a2av_pack(src, outer, na, row, P, block=0):
    """[outer][na][row] -> the blocks src[:, lo_p:hi_p, :] of the ranks back to back"""
    s = np.asarray(src).reshape(outer, na, row)
    lo = block_bounds(na, P, block)
    return np.concatenate([s[:, lo[p]:lo[p + 1], :].reshape(-1) for p in range(P)])


def a2av_unpack(src, outer_na, nb, inner, P, block=0):
    """blocks [outer_na][nb_p][inner] back to back -> [outer_na][nb][inner]"""
    s = np.asarray(src).reshape(-1)
    lo = block_bounds(nb, P, block)
    out = np.empty((outer_na, nb, inner), dtype=s.dtype)
    off = 0
    for p in range(P):
        cnt = outer_na * (lo[p + 1] - lo[p]) * inner
        out[:, lo[p]:lo[p + 1], :] = s[off:off + cnt].reshape(outer_na, lo[p + 1] - lo[p], inner)
        off += cnt
    return out.reshape(-1)


# ---- launch-shape classes ---------------------------------------------------------------------------------------------
def stream_tags(n, vector=True):
    """lincomb / bilinear: the grid-stride loop runs over n / 2 16-byte words, thread 0 takes the odd last element"""
    items = n // 2 if vector else n
    tags = ["odd" if n & 1 else "even"]
    if items == 0:
        tags.append("tail_only")
    elif items <= STREAM_PASS:
        tags.append("one_pass")
    else:
        tags.append("multi_pass")
    return tuple(sorted(tags))


def cfl_tags(shape, comp_axis):
    n = int(np.prod(shape))
    tags = ["axes%d" % len(shape), "multi_pass" if n > STREAM_PASS else "one_pass",
            "identity" if list(comp_axis) == list(range(len(comp_axis))) else "permuted"]
    if 1 in shape:
        tags.append("length1_axis")
    if any(s & (s - 1) for s in shape):
        tags.append("not_pow2")
    return tuple(sorted(tags))


def seg_grid(nseg, seg_doubles):
    """seg_grid() of the kernel source -> (gridDim.x, gridDim.y, halved, capped)"""
    cx = max((seg_doubles // 2 + SEG_WORDS_PER_CHUNK - 1) // SEG_WORDS_PER_CHUNK, 1)
    halved = False
    while cx > 1 and cx * nseg > SEG_WORKGROUP_TARGET:
        cx = (cx + 1) // 2
        halved = True
    capped = cx > SEG_CX_CAP
    return min(cx, SEG_CX_CAP), min(nseg, SEG_GRID_Y_CAP), halved, capped


def segment_tags(nseg, grid_seg_doubles, segments):
    """segments: the distinct (doubles, vector?) copies of the launch; grid_seg_doubles sizes the grid"""
    cx, gy, halved, capped = seg_grid(nseg, grid_seg_doubles)
    nth = cx * STREAM_THREADS
    tags = {"cx1" if cx == 1 else "cx_gt1"}
    if halved:
        tags.add("cx_halved")
    if capped:
        tags.add("cx_capped")
    if nseg > gy:
        tags.add("y_capped")
    for cnt, vec in segments:
        if cnt == 0:
            tags.add("empty_segment")
            continue
        if cnt > 2048:
            tags.add("seg_gt_2048")
        if not vec:
            tags.add("scalar")
            if cnt > nth:
                tags.add("scalar_multi_pass")
            continue
        tags.add("vec")
        n2 = cnt // 2
        if n2 > (SEG_UNROLL - 1) * nth:
            tags.add("unroll")                                   # some thread runs the 4x-unrolled loop
            if n2 % (SEG_UNROLL * nth) == 0:
                tags.add("unroll_exact")                         # ... and nobody the plain loop after it
            else:
                tags.add("unroll_rest")                          # ... and the plain loop moves the rest
                if n2 > SEG_UNROLL * nth:
                    tags.add("unroll_rest_same_thread")          # ... in a thread that ran unrolled rounds before
    return tuple(sorted(tags))


def pack_geometry(kind, dims):
    """-> (nseg, doubles that size the grid, distinct (doubles, vector?) segments, doubles in, doubles out)"""
    if kind == "a2a_pack":
        outer, na, nb, inner, P = dims
        seg = (na // P) * nb * inner
        return outer * P, seg, {(seg, seg % 2 == 0)}, outer * na * nb * inner, outer * na * nb * inner
    if kind == "a2a_unpack":
        outer, na, nb, inner, P = dims
        seg = (nb // P) * inner
        return P * outer * na, seg, {(seg, seg % 2 == 0 and (nb * inner) % 2 == 0)}, outer * na * nb * inner, outer * na * nb * inner
    if kind == "a2av_pack":
        outer, na, row, P, block = dims
        lo = block_bounds(na, P, block)
        B = block if block else -(-na // P)
        segs = set()
        for p in range(P):
            cnt = (lo[p + 1] - lo[p]) * row
            for o in sorted(set((0, 1 % outer))):                # addresses repeat with period 2 in o
                so, dof = (o * na + lo[p]) * row, outer * row * lo[p] + o * cnt
                segs.add((cnt, (cnt | so | dof) % 2 == 0))
        return outer * P, B * row, segs, outer * na * row, outer * na * row
    if kind == "a2av_unpack":
        outer_na, nb, inner, P, block = dims
        lo = block_bounds(nb, P, block)
        B = block if block else -(-nb // P)
        segs = set()
        for p in range(P):
            cnt = (lo[p + 1] - lo[p]) * inner
            for oi in sorted(set((0, 1 % outer_na))):
                so, dof = outer_na * inner * lo[p] + oi * cnt, (oi * nb + lo[p]) * inner
                segs.add((cnt, (cnt | so | dof) % 2 == 0))
        return P * outer_na, B * inner, segs, outer_na * nb * inner, outer_na * nb * inner
    raise ValueError(kind)


def pack_tags(kind, dims):
    nseg, gseg, segs, _, _ = pack_geometry(kind, dims)
    tags = set(segment_tags(nseg, gseg, segs))
    if kind.startswith("a2av"):
        n, P, block = (dims[1], dims[3], dims[4])
        lo = block_bounds(n, P, block)
        if any(lo[p + 1] == lo[p] for p in range(P)):
            tags.add("empty_rank")
        tags.discard("empty_segment")
    return tuple(sorted(tags))


def pack_reference(kind, src, dims):
    return {"a2a_pack": a2a_pack, "a2a_unpack": a2a_unpack, "a2av_pack": a2av_pack, "a2av_unpack": a2av_unpack}[kind](src, *dims)


def pack_input(kind, dims):
    """every entry distinct (its own index + 1/2): any misplaced, dropped or repeated element changes the result"""
    n_in = pack_geometry(kind, dims)[3]
    return np.arange(n_in, dtype=np.float64) + 0.5


# The classes the pack / unpack tests must reach -> predicate on the tags of a case.  Segments of 2000 and of 1800
# doubles both run ONE unrolled round in the low threads and the plain vector loop in the others (cx = 1, 256 threads,
# 1000 resp. 900 words): by the loop structure they are one class, kept as two cases.  Segments of 2048 doubles are the
# shape where the unrolled loop moves everything; a thread runs both loops only once cx is halved or capped.
PACK_CLASSES = {
    "unrolled_cx1": lambda t: "unroll" in t and "cx1" in t,
    "unrolled_exact": lambda t: "unroll_exact" in t and "cx1" in t,
    "unrolled_with_rest": lambda t: "unroll_rest" in t and "cx1" in t,
    "unrolled_and_rest_in_one_thread": lambda t: "unroll_rest_same_thread" in t,
    "cx_gt1_not_halved": lambda t: "cx_gt1" in t and "cx_halved" not in t and "cx_capped" not in t,
    "cx_halved": lambda t: "cx_halved" in t,
    "cx_capped": lambda t: "cx_capped" in t,
    "y_capped": lambda t: "y_capped" in t,
    "scalar_large": lambda t: "scalar_multi_pass" in t and "seg_gt_2048" in t,
    "a2av_mixed_with_empty_rank": lambda t: {"vec", "scalar", "empty_rank", "seg_gt_2048"} <= set(t),
}
# which kernels must reach which class ("a2av" where the class applies to uneven blocks as well)
PACK_CLASS_KINDS = {
    "unrolled_cx1": ("a2a_pack", "a2a_unpack", "a2av_pack", "a2av_unpack"),
    "unrolled_exact": ("a2a_pack", "a2a_unpack"),
    "unrolled_with_rest": ("a2a_pack", "a2a_unpack", "a2av_pack", "a2av_unpack"),
    "unrolled_and_rest_in_one_thread": ("a2a_pack", "a2a_unpack"),
    "cx_gt1_not_halved": ("a2a_pack", "a2a_unpack", "a2av_pack", "a2av_unpack"),
    "cx_halved": ("a2a_pack", "a2a_unpack", "a2av_pack", "a2av_unpack"),
    "cx_capped": ("a2a_pack", "a2a_unpack", "a2av_pack", "a2av_unpack"),
    "y_capped": ("a2a_pack", "a2a_unpack", "a2av_pack", "a2av_unpack"),
    "scalar_large": ("a2a_pack", "a2a_unpack", "a2av_pack", "a2av_unpack"),
    "a2av_mixed_with_empty_rank": ("a2av_pack", "a2av_unpack"),
}

_T_UNROLL_REST = ("cx1", "unroll", "unroll_rest", "vec")
_T_UNROLL_EXACT = ("cx1", "unroll", "unroll_exact", "vec")
_T_CX_GT1 = ("cx_gt1", "seg_gt_2048", "unroll", "unroll_rest", "vec")
_T_HALVED = ("cx_gt1", "cx_halved", "seg_gt_2048", "unroll", "unroll_exact", "vec")
_T_CAPPED = ("cx_capped", "cx_gt1", "seg_gt_2048", "unroll", "unroll_rest", "unroll_rest_same_thread", "vec")
_T_YCAP = ("cx1", "vec", "y_capped")
_T_SCALAR = ("cx_gt1", "scalar", "scalar_multi_pass", "seg_gt_2048")

# name -> (kernel, dims, declared tags).  dims: a2a_* (outer, na, nb, inner, P); a2av_pack (outer, na, row, P, block);
# a2av_unpack (outer_na, nb, inner, P, block), block 0 = ceil(n / P).
PACK_CASES = {
    # segments of 2000 / 1800 / 2048 doubles, cx = 1
    "pack_seg2000": ("a2a_pack", (3, 16, 50, 10, 4), _T_UNROLL_REST),
    "unpack_seg2000": ("a2a_unpack", (2, 3, 8, 1000, 4), _T_UNROLL_REST),
    "pack_seg1800": ("a2a_pack", (3, 8, 90, 10, 4), _T_UNROLL_REST),
    "unpack_seg1800": ("a2a_unpack", (2, 3, 8, 900, 4), _T_UNROLL_REST),
    "pack_seg2048": ("a2a_pack", (3, 8, 64, 16, 4), _T_UNROLL_EXACT),
    "unpack_seg2048": ("a2a_unpack", (2, 3, 8, 1024, 4), _T_UNROLL_EXACT),
    "packv_seg2000": ("a2av_pack", (3, 7, 1000, 4, 0), _T_UNROLL_REST),
    "unpackv_seg2000": ("a2av_unpack", (5, 7, 1000, 4, 0), _T_UNROLL_REST),
    "packv_seg1800": ("a2av_pack", (3, 7, 900, 4, 0), _T_UNROLL_REST),
    "unpackv_seg1800": ("a2av_unpack", (5, 7, 900, 4, 0), _T_UNROLL_REST),
    # cx = 5, no halving: 12 segments of 10 000 doubles
    "pack_cx5": ("a2a_pack", (3, 8, 50, 100, 4), _T_CX_GT1),
    "unpack_cx5": ("a2a_unpack", (1, 3, 8, 5000, 4), _T_CX_GT1),
    "packv_cx5": ("a2av_pack", (3, 7, 5000, 4, 0), _T_CX_GT1),
    "unpackv_cx5": ("a2av_unpack", (3, 7, 5000, 4, 0), _T_CX_GT1),
    # cx halved 512 -> 256: 64 segments of 2^20 doubles (see CX_HALVED_EXCEPTION)
    "pack_halved": ("a2a_pack", (8, 8, 1024, 1024, 8), _T_HALVED),
    "unpack_halved": ("a2a_unpack", (1, 8, 8, 1 << 20, 8), _T_HALVED),
    # ... with uneven blocks the grid is sized by the block, so 64 segments sized for 2^20 doubles of which the trailing
    # ranks own nothing stay small: explicit blocks of 2 rows of 2^19, an axis of 2 rows, 8 ranks
    "packv_halved": ("a2av_pack", (8, 2, 1 << 19, 8, 2), _T_HALVED + ("empty_rank",)),
    "unpackv_halved": ("a2av_unpack", (8, 2, 1 << 19, 8, 2), _T_HALVED + ("empty_rank",)),
    # cx capped 1600 -> 1024: 8 segments of 3 276 800 doubles, the per-rank shape of the 512^2 x 256 problem on 8 ranks
    "pack_capped": ("a2a_pack", (1, 8, 25, 131072, 8), _T_CAPPED),
    "unpack_capped": ("a2a_unpack", (1, 1, 200, 131072, 8), _T_CAPPED),
    "packv_capped": ("a2av_pack", (1, 8, 3276800, 8, 0), _T_CAPPED),
    "unpackv_capped": ("a2av_unpack", (1, 8, 3276800, 8, 0), _T_CAPPED),
    # 131 072 segments of 6 doubles on 8 ranks: gridDim.y = 65535 and the `r += gridDim.y` loop
    "pack_ycap": ("a2a_pack", (16384, 16, 3, 1, 8), _T_YCAP),
    "unpack_ycap": ("a2a_unpack", (128, 128, 16, 3, 8), _T_YCAP),
    "packv_ycap": ("a2av_pack", (16384, 16, 3, 8, 0), _T_YCAP),
    "unpackv_ycap": ("a2av_unpack", (16384, 16, 3, 8, 0), _T_YCAP),
    # odd segments of 4097 doubles: the scalar path, several passes of 512 threads
    "pack_scalar4097": ("a2a_pack", (3, 4, 17, 241, 4), _T_SCALAR),
    "unpack_scalar4097": ("a2a_unpack", (2, 3, 68, 241, 4), _T_SCALAR),
    "packv_scalar4097": ("a2av_pack", (3, 3, 4097, 4, 0), _T_SCALAR + ("empty_rank",)),
    "unpackv_scalar4097": ("a2av_unpack", (3, 3, 4097, 4, 0), _T_SCALAR + ("empty_rank",)),
    # odd row, 3 ranks, blocks of 4 of an axis of 7 (whole chunks of 2): segments of 4100 and 3075 doubles, vector or scalar
    # by the parity of their offsets, and a third rank that owns nothing (cx = 3: 2050 words stay below 3 * 768, no unrolling)
    "packv_mixed": ("a2av_pack", (4, 7, 1025, 3, 4),
                    ("cx_gt1", "empty_rank", "scalar", "scalar_multi_pass", "seg_gt_2048", "vec")),
    "unpackv_mixed": ("a2av_unpack", (4, 7, 1025, 3, 4),
                      ("cx_gt1", "empty_rank", "scalar", "scalar_multi_pass", "seg_gt_2048", "vec")),
}
PACK_CASES = {k: (v[0], v[1], tuple(sorted(v[2]))) for k, v in PACK_CASES.items()}
# seg_grid() halves cx only when ceil(seg / 2048) * nseg > 16384, i.e. when nseg * seg exceeds 2^25 doubles = 268 MB: an even
# pack / unpack cannot reach that loop with buffers of 256 MB.  These two cases use the 64 x 2^20 doubles (537 MB) that
# reach it; every other buffer of the tables stays below MAX_BUFFER_BYTES.
CX_HALVED_EXCEPTION = ("pack_halved", "unpack_halved")


# ---- lincomb ----------------------------------------------------------------------------------------------------------
LINCOMB_NTERMS = (1, 2, 5, 16)
LINCOMB_SIZES = (1, 2, 3, 255, 100003, 1048578, 3000001)
LINCOMB_TAGS = {1: ("odd", "tail_only"), 2: ("even", "one_pass"), 3: ("odd", "one_pass"), 255: ("odd", "one_pass"),
                100003: ("odd", "one_pass"), 1048578: ("even", "multi_pass"), 3000001: ("multi_pass", "odd")}
LINCOMB_CLASSES = (("odd", "tail_only"), ("even", "one_pass"), ("odd", "one_pass"), ("even", "multi_pass"),
                   ("multi_pass", "odd"))
LINCOMB_CASES = [(nt, n) for nt in LINCOMB_NTERMS for n in LINCOMB_SIZES]
LINCOMB_ALIAS_CASE = (5, 100003)            # y is also operand 0, the way the timesteppers accumulate into a stage


def lincomb_inputs(nterms, n):
    rng = np.random.default_rng(1000 * nterms + n % 997)
    xs = [rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4) for _ in range(nterms)]
    alphas = rng.standard_normal(nterms) * 10.0 ** rng.integers(-2, 3, nterms)
    return xs, alphas


# ---- bilinear ---------------------------------------------------------------------------------------------------------
def _shuffled(terms, seed):
    order = np.random.default_rng(seed).permutation(len(terms))
    out = [terms[i] for i in order]
    key = [(t[1], t[2]) for t in out]
    assert len(terms) < 3 or key != sorted(key), "the table must reach the kernel unsorted"
    return out


def _bilinear_tables():
    rng = np.random.default_rng(77)
    cf = lambda: float(np.round(rng.uniform(-2, 2), 3)) or 1.0
    t = {}
    # u . grad(b): a = u [3], b = grad b [3] -> 1 output
    t["u_grad_b"] = (1, 3, 3, [(0, j, j, -1.0) for j in range(3)])
    # 2-D u . grad(u): a = u [2], b = grad u [2][2] -> 2 outputs
    t["u_grad_u_2d"] = (2, 2, 4, [(i, j, 2 * j + i, -1.0) for i in range(2) for j in range(2)])
    # u . grad(u): a = u [3], b = grad u [3][3] (row j = d_j) -> 3 outputs, 9 terms
    t["u_grad_u"] = (3, 3, 9, [(i, j, 3 * j + i, -1.0) for i in range(3) for j in range(3)])
    # 4 outputs: three terms share the pair (1, 2) and feed outputs 0, 1, 3; two share (0, 0); output 2 gets nothing
    t["shared_pairs_gap"] = (4, 2, 3, [(0, 1, 2, 1.5), (1, 1, 2, -0.25), (3, 1, 2, 2.0), (0, 0, 0, 0.75), (3, 0, 0, -1.25),
                                         (1, 0, 1, 3.0)])
    # rank-2 product a (x) b -> 9 outputs
    t["outer_product"] = (9, 3, 3, [(3 * i + j, i, j, cf()) for i in range(3) for j in range(3)])
    # 32 terms: every pair of a [3] x b [9] once and five pairs a second time, outputs drawn at random
    pairs = [(i, j) for i in range(3) for j in range(9)]
    pairs += [pairs[k] for k in (0, 7, 13, 20, 26)]
    t["terms32"] = (9, 3, 9, [(int(rng.integers(0, 9)), i, j, cf()) for (i, j) in pairs])
    # one component on both sides (the only shape an odd point count accepts), two terms
    t["scalar_square"] = (1, 1, 1, [(0, 0, 0, 0.5), (0, 0, 0, -1.75)])
    return {k: (v[0], v[1], v[2], _shuffled(v[3], 11 + i)) for i, (k, v) in enumerate(t.items())}


BILINEAR_TABLES = _bilinear_tables()        # name -> (ncomp_out, ncomp_a, ncomp_b, shuffled terms (ic, ia, ib, coef))
BILINEAR_SIZES = (2, 4096, 1048578)
BILINEAR_ODD_CASE = ("scalar_square", 100003)
BILINEAR_CASES = [(name, n) for name in BILINEAR_TABLES for n in BILINEAR_SIZES] + [BILINEAR_ODD_CASE]
BILINEAR_TAGS = {2: ("even", "one_pass"), 4096: ("even", "one_pass"), 1048578: ("even", "multi_pass"),
                 100003: ("odd", "one_pass")}
BILINEAR_CLASSES = (("even", "one_pass"), ("even", "multi_pass"), ("odd", "one_pass"))


def bilinear_inputs(name, n):
    _, na, nb, _ = BILINEAR_TABLES[name]
    rng = np.random.default_rng(abs(hash((len(name), na, nb, n))) % (1 << 31))
    return rng.standard_normal((na, n)), rng.standard_normal((nb, n)) * 3.0


# ---- Cartesian CFL ----------------------------------------------------------------------------------------------------
def _inv_spacing(kind, N, L):
    if kind == "cheb":                      # Gauss-Chebyshev grid: dx = L/2 sin(theta) pi / N, 1 / dx from ~2N/(pi L) to ~4N^2/(pi^2 L)
        theta = np.pi * (np.arange(N) + 0.5) / N
        dx = 0.5 * L * np.sin(theta) * np.pi / N
    elif kind == "geom":                    # geometrically stretched cells
        dx = L / N * 1.37 ** (np.arange(N) * 8.0 / max(N, 8))
    else:                                   # uniform Fourier grid
        dx = np.full(N, L / N)
    return 1.0 / dx


# name -> (shape, comp_axis, spacing kind per COMPONENT, declared tags)
CFL_CASES = {
    "line1000": ((1000,), (0,), ("cheb",), ("axes1", "identity", "not_pow2", "one_pass")),
    "plane64x96": ((64, 96), (0, 1), ("uniform", "cheb"), ("axes2", "identity", "not_pow2", "one_pass")),
    "plane64x96_swapped": ((64, 96), (1, 0), ("cheb", "geom"), ("axes2", "not_pow2", "one_pass", "permuted")),
    "box7x12x5": ((7, 12, 5), (0, 1, 2), ("geom", "cheb", "cheb"), ("axes3", "identity", "not_pow2", "one_pass")),
    "box7x12x5_rotated": ((7, 12, 5), (2, 0, 1), ("cheb", "geom", "cheb"), ("axes3", "not_pow2", "one_pass", "permuted")),
    "box96x1x48": ((96, 1, 48), (0, 1, 2), ("geom", "uniform", "cheb"),
                   ("axes3", "identity", "length1_axis", "not_pow2", "one_pass")),
    "box96x1x48_rotated": ((96, 1, 48), (1, 2, 0), ("uniform", "cheb", "geom"),
                           ("axes3", "length1_axis", "not_pow2", "one_pass", "permuted")),
    "box192x96x48": ((192, 96, 48), (0, 1, 2), ("geom", "geom", "cheb"), ("axes3", "identity", "multi_pass", "not_pow2")),
    "box192x96x48_rotated": ((192, 96, 48), (2, 0, 1), ("cheb", "geom", "geom"),
                             ("axes3", "multi_pass", "not_pow2", "permuted")),
}
CFL_CLASSES = ("axes1", "axes2", "axes3", "identity", "permuted", "length1_axis", "multi_pass", "one_pass", "not_pow2")
PLANTS = ("none", "first", "last", "final_pass", "distinct_indices")
PLANT_FACTOR = 1.0e6


def plant_index(shape, where):
    """flat index of the planted point, or None where the case has no such point"""
    n = int(np.prod(shape))
    if where == "first":
        return 0
    if where == "last":
        return n - 1
    if where == "final_pass":               # reached only in the last grid-stride pass: needs more than one
        if n <= STREAM_PASS:
            return None
        last_start = ((n - 1) // STREAM_PASS) * STREAM_PASS
        return last_start + (n - last_start) // 3
    if where == "distinct_indices":         # per-axis indices pairwise different (and not a reversal of each other's range)
        if len(shape) < 2 or sorted(shape)[-2] < 2:
            return None
        idx, used = [], set()
        for s in shape:
            k = next((k for k in range(min(s - 1, 3), -1, -1) if k not in used), None) if s > 1 else 0
            if k is None:
                return None
            idx.append(k)
            if s > 1:
                used.add(k)
        return int(np.ravel_multi_index(idx, shape))
    return None


def cfl_inputs(name, plant="none"):
    """-> (u [ncomp][n] float64, inverse spacings per component, planted flat index or None)"""
    shape, comp_axis, kinds, _ = CFL_CASES[name]
    ncomp, n = len(comp_axis), int(np.prod(shape))
    rng = np.random.default_rng(sum(shape) + 31 * len(name))
    u = rng.uniform(-1.0, 1.0, (ncomp, n))
    u[:, 1::7] = -0.0                                            # zeros of both signs among the velocities
    u[0, 2::11] = 0.0
    inv = [_inv_spacing(k, shape[comp_axis[c]], 1.0 + c) for c, k in enumerate(kinds)]
    at = plant_index(shape, plant)
    if at is not None:
        u[:, at] = PLANT_FACTOR * np.array([1.0, -0.75, 0.5])[:ncomp]
    return u, inv, at


# ---- spherical CFL ----------------------------------------------------------------------------------------------------
# name -> ((Nphi, Ntheta, Nr), inv_h identically zero?, declared tags)
SPH_CASES = {
    "shell8x4x5": ((8, 4, 5), False, ("one_pass",)),
    "shell64x32x48": ((64, 32, 48), False, ("one_pass",)),
    "shell64x32x48_lmax0": ((64, 32, 48), True, ("inv_h_zero", "one_pass")),
    "shell128x96x72": ((128, 96, 72), False, ("multi_pass",)),
}
SPH_CLASSES = ("one_pass", "multi_pass", "inv_h_zero")
# no "distinct_indices" plant here: the kernel derives one index only, ir = i % nr, and with non-uniform inv_dr and inv_h the
# final_pass plant and the unplanted fields (maximum at a generic point) already return a different value under a wrong ir
SPH_PLANTS = ("none", "first", "last", "final_pass")


def sph_tags(shape, zero_h):
    n = int(np.prod(shape))
    return tuple(sorted((["inv_h_zero"] if zero_h else []) + ["multi_pass" if n > STREAM_PASS else "one_pass"]))


def sph_inputs(name, plant="none"):
    """-> (u [3][Nphi][Ntheta][Nr], inv_h [Nr], inv_dr [Nr], planted flat index or None)"""
    shape, zero_h, _ = SPH_CASES[name]
    nr, n = shape[2], int(np.prod(shape))
    rng = np.random.default_rng(sum(shape) + (5 if zero_h else 0))
    u = rng.uniform(-1.0, 1.0, (3, n))
    u[:, 1::7] = -0.0
    theta = np.pi * (np.arange(nr) + 0.5) / nr
    r = 14.5 - 0.5 * np.cos(theta)                               # Gauss-Chebyshev radii of a shell 14 < r < 15
    inv_dr = 1.0 / (0.5 * np.sin(theta) * np.pi / nr)
    inv_h = np.zeros(nr) if zero_h else np.sqrt(15.0 * 16.0) / r
    at = plant_index(shape, plant)
    if at is not None:
        u[:, at] = PLANT_FACTOR * np.array([0.6, -0.8, 0.5])
    return u.reshape((3,) + shape), inv_h, inv_dr, at


# NaN policy of both reductions: where the single NaN goes (flat index by name) and in which component
NAN_PLANTS = ("first", "last", "final_pass_or_mid")


def nan_index(shape, where):
    n = int(np.prod(shape))
    if where == "first":
        return 0
    if where == "last":
        return n - 1
    last_start = ((n - 1) // STREAM_PASS) * STREAM_PASS        # mid-array of the last (or only) pass
    return last_start + (n - last_start) // 2


# ---- scatter ----------------------------------------------------------------------------------------------------------
SCATTER_SIZES = (1, 255, 257, 70001)        # one thread per entry in blocks of 256: below, across and far above one block
SCATTER_TAGS = {1: ("one_block",), 255: ("one_block",), 257: ("two_blocks",), 70001: ("many_blocks",)}


def scatter_tags(n):
    blocks = -(-n // STREAM_THREADS)
    return ("one_block",) if blocks == 1 else (("two_blocks",) if blocks == 2 else ("many_blocks",))


def scatter_inputs(n):
    """-> (y of 3 n + 17 entries, n unique indices in random order, values)"""
    rng = np.random.default_rng(n)
    m = 3 * n + 17
    y = rng.standard_normal(m)
    idx = rng.permutation(m)[:n].astype(np.int64)
    vals = rng.standard_normal(n) * 10.0 ** rng.integers(-8, 9, n)
    return y, idx, vals
