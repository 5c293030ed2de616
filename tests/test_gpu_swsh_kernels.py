"""GPU: the kernels of dedalus_amd/csrc/ddh_swsh.hip (batched GEMV in three widths, paired and unpaired; LDS-tiled GEMM;
FP64 MFMA GEMM; regularity_kernel<1|3|9>) against the longdouble references of tests/swsh_cases.py, at the edges of their
tiles, lane strides and thread counts (tests/test_swsh_cases_host.py proves the inputs, the references and the coverage).

The bound is derived, not measured (u = 2^-53): every output element satisfies |got - ref| <= (K + 2) u S, K the
contraction length and S = sum |a_k| |x_k| over the contraction.  A sum of K individually rounded products accumulated in
any order has a relative error of at most gamma_K = K u / (1 - K u) against S; fused multiply-adds (FMA, MFMA) round less
often, the mirrored signs are exact, and (K + 2) u covers gamma_K for every K here (K <= 130).  The regularity
recombination adds one multiplication by the radial factor: (NC + 2) u S.  No whole-array norm anywhere in this file.

Poisoning: inputs are NaN wherever the operation names no element, outputs are prefilled with 7.0.  No NaN may reach a
named output, every unnamed output element keeps the bits of 7.0, backward fills exactly the grid slices of groups without
a matrix (paired partners included) with +0.0.  Every case runs twice into fresh outputs and must repeat bit for bit.
With DDH_SWSH_PARITY_OUT=<file> the figures per case are written there (the table for profiles/swsh_kernel_parity.txt)."""
import os

import numpy as np
import pytest

import swsh_cases as sc

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
SEVEN = np.float64(7.0).view(np.uint64)
RECORD = []


@pytest.fixture(scope="module", autouse=True)
def parity_record():
    yield
    path = os.environ.get("DDH_SWSH_PARITY_OUT")
    if path:
        with open(path, "w") as fh:
            fh.write("# tests/test_gpu_swsh_kernels.py: largest |got - ref| / (u S) per case beside the bound K + 2 (u = 2^-53,\n")
            fh.write("# S = sum |a_k| |x_k|), at the element where their quotient is largest; ref: longdouble, tests/swsh_cases.py\n")
            fh.write("%-28s %-9s %-5s %-34s %10s %6s\n" % ("# case", "direction", "path", "shape", "err/(u S)", "K + 2"))
            for row in RECORD:
                fh.write("%-28s %-9s %-5s %-34s %10.3f %6d\n" % row)


@pytest.fixture(scope="module")
def ex():
    from dedalus_amd.executor import HipExecutor
    return HipExecutor()


def make_plan(ex, p):
    mmt = ex.make_grouped_mmt(p.n_grid, p.groups, p.keys, p.fwd, p.bwd)
    if p.paired:
        mmt.set_pairs(p.pair_g, p.pair_c, p.pair_mode, p.parity)
    return mmt


def run(ex, mmt, direction, src, out_shape):
    out = ex.dev.empty(out_shape)
    out.fill_(7.0)
    src_d = ex.from_host(np.array(src))              # (the shared inputs are read-only)
    if direction == "forward":
        mmt.forward(src_d, out)
    else:
        mmt.backward(src_d, out)
    ex.sync()
    return np.array(ex.download(out))


def run_aliased(ex, mmt, direction, src, out_shape):
    """in and out are two views of one device buffer, the second half of in under the first part of out
    -> (out, mask of the out elements that lie over in)"""
    n_in, n_out = src.size, int(np.prod(out_shape))
    lap = min(n_in, n_out) // 2
    buf = ex.dev.empty(n_in - lap + n_out)
    buf.fill_(7.0)
    src_d, out = buf[:n_in].view(src.shape), buf[n_in - lap:].view(out_shape)
    src_d.copy_(ex.from_host(np.array(src)))
    assert src_d.data_ptr() == buf.data_ptr() and out.data_ptr() == buf.data_ptr() + 8 * (n_in - lap)
    if direction == "forward":
        mmt.forward(src_d, out)
    else:
        mmt.backward(src_d, out)
    ex.sync()
    over = np.zeros(n_out, bool)
    over[:lap] = True
    return np.array(ex.download(out)), over.reshape(out_shape)


def check(label, direction, p, got, ref, ignore=None):
    """elementwise bound on the named elements, +0.0 on the zero-filled ones, the bits of 7.0 everywhere else (ignore:
    unnamed elements whose prefill was something else)"""
    named = ref["named"]
    zero = ref.get("zero", np.zeros_like(named))
    assert got.shape == named.shape
    assert not np.isnan(got[named]).any(), (label, direction, "NaN in a named output: a poisoned element was read")
    assert np.all(got[zero].view(np.uint64) == 0), (label, direction, "a slice without a matrix is not +0.0")
    rest = ~(named | zero) if ignore is None else ~(named | zero | ignore)
    assert np.all(got[rest].view(np.uint64) == SEVEN), (label, direction, "an element the operation does not name was written")
    err = np.abs(got[named].astype(sc.LD) - ref["ref"][named])
    S, K = ref["S"][named], ref["K"][named]
    ratio = (err / (U * S)).astype(np.float64)
    k = int(np.argmax(ratio / (K + 2)))
    shape = "n_grid=%d n0=%d count<=%d n3=%d" % (p.n_grid, p.n0, p.max_count, p.n3)
    print("%s %s %s %s: err/(u S) %.3f, K + 2 = %d" % (label, direction, p.path, shape, ratio[k], K[k] + 2))
    if ignore is None:
        RECORD.append((label, direction, p.path, shape, float(ratio[k]), int(K[k] + 2)))
    bad = err > (K + 2) * U * S
    assert not bad.any(), (label, direction, int(bad.sum()), float(ratio[k]), int(K[k] + 2))


def directions(name):
    p = sc.plan(name)
    g, c = sc.inputs(name)
    return p, (("forward", g, p.cshape, sc.forward_reference(name)), ("backward", c, p.gshape, sc.backward_reference(name)))


@pytest.mark.parametrize("name", list(sc.CASES))
def test_grouped_transform(ex, name):
    p, dirs = directions(name)
    mmt = make_plan(ex, p)
    for direction, src, out_shape, ref in dirs:
        got = run(ex, mmt, direction, src, out_shape)
        check(name, direction, p, got, ref)
        again = run(ex, mmt, direction, src, out_shape)
        assert np.array_equal(got.view(np.uint64), again.view(np.uint64)), (name, direction, "not repeatable")


@pytest.mark.parametrize("name", sc.ALIAS_CASES)
def test_out_overlapping_in(ex, name):
    p, dirs = directions(name)
    mmt = make_plan(ex, p)
    for direction, src, out_shape, ref in dirs:
        plain = run(ex, mmt, direction, src, out_shape)
        got, over = run_aliased(ex, mmt, direction, src, out_shape)
        written = ref["named"] | ref.get("zero", False)
        assert over[written].any() and not over[written].all()
        check(name + " aliased", direction, p, got, ref, ignore=over)
        assert np.array_equal(got[written].view(np.uint64), plain[written].view(np.uint64)), (name, direction)


# ---- regularity recombination ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_fac", [False, True])
@pytest.mark.parametrize("ncomp", sc.REG_NCOMP)
def test_regularity_recombine(ex, ncomp, with_fac):
    worst = 0.0
    for n3 in sc.REG_N3:
        data, slot_map, mats, fac = sc.regularity_inputs(ncomp, n3)
        ref, S = sc.regularity_reference(data, slot_map, mats, fac if with_fac else None)
        table = ex.make_recombination(np.array(slot_map), np.array(mats))
        fac_d = ex.from_host(np.array(fac)) if with_fac else None
        runs = []
        for _ in range(2):
            d = ex.from_host(np.array(data))
            ex.regularity_recombine(d, table, fac_d)
            ex.sync()
            runs.append(np.array(ex.download(d)))
        got = runs[0]
        assert np.array_equal(got.view(np.uint64), runs[1].view(np.uint64)), (ncomp, n3, "not repeatable")
        assert not np.isnan(got).any(), (ncomp, n3, "the matrix no slot names was read")
        err = np.abs(got.astype(sc.LD) - ref)
        worst = max(worst, float((err / (U * S)).max()))
        assert np.all(err <= (ncomp + 2) * U * S), (ncomp, n3, float((err / (U * S)).max()))
        dead = slot_map == -1
        want = data[:, dead] * fac if with_fac else data[:, dead]                   # scaled only / untouched
        assert np.array_equal(got[:, dead].view(np.uint64), np.ascontiguousarray(want).view(np.uint64)), (ncomp, n3)
        if ncomp > 1:
            assert not np.array_equal(got[:, ~dead], np.ascontiguousarray(data[:, ~dead] * (fac if with_fac else 1.0)))
    shape = "n1 x n2 = %d x %d, n3 = %d .. %d" % (sc.REG_N12 + (min(sc.REG_N3), max(sc.REG_N3)))
    label = "regularity<%d>%s" % (ncomp, " factor" if with_fac else "")
    print("%s: err/(u S) %.3f, NC + 2 = %d" % (label, worst, ncomp + 2))
    RECORD.append((label, "in place", "reg", shape, worst, ncomp + 2))


def test_regularity_scalar_without_table(ex):
    for n3 in sc.REG_N3:
        data, slot_map, mats, fac = sc.regularity_inputs(1, n3)
        d = ex.from_host(np.array(data))
        ex.regularity_recombine(d, None, None)                          # no table, no factor: writes nothing
        ex.sync()
        assert np.array_equal(np.array(ex.download(d)).view(np.uint64), data.view(np.uint64)), n3
        ex.regularity_recombine(d, None, ex.from_host(np.array(fac)))             # no table: the factor alone
        ex.sync()
        assert np.array_equal(np.array(ex.download(d)).view(np.uint64), (data * fac).view(np.uint64)), n3


# ---- argument checks ---------------------------------------------------------------------------------------------------
def test_argument_checks_launch_nothing(ex):
    from dedalus_amd import libhip
    rng = np.random.default_rng(3)
    N = 6
    F, B = rng.standard_normal((4, N)), rng.standard_normal((N, 4))

    def make(rows, fwd=(F,), bwd=(B,)):
        return ex.make_grouped_mmt(N, np.array(rows, dtype=np.int64), [100], list(fwd), list(bwd))

    # (key, g_start, c_start, count, ell_start, ell_step, n_ell)
    for rows, why in (([(100, 0, 0, 1, 0, 2, 4)], "malformed group"), ([(100, 0, 0, 0, 0, 1, 4)], "malformed group"),
                      ([(100, 0, 0, 1, 0, 1, 5)], "group row count differs from its matrix"),
                      ([(100, -1, 0, 1, 0, 1, 4)], "negative slice start"), ([(100, 0, -1, 1, 0, 1, 4)], "negative slice start"),
                      ([(100, 0, 0, 1, 2, -1, 4)], "negative slice start")):
        with pytest.raises(libhip.DdhError, match=why):
            make(rows)

    folded = make([(100, 0, 0, 1, 0, 1, 4), (100, 1, 1, 1, 3, -1, 4)])
    for args, why in ((([2], [2], [1], [0]), "group count differs from the plan"),
                      (([2, 3], [2, 3], [3, 0], [0, 0]), "bad pair mode"), (([2, 3], [2, 3], [0, -1], [0, 0]), "bad pair mode"),
                      (([2, 3], [2, 3], [0, 1], [0, 0]), "pairs need ell_step = 1"),
                      (([-1, 3], [2, 3], [2, 0], [0, 0]), "pairs need ell_step = 1")):
        with pytest.raises(libhip.DdhError, match=why):
            folded.set_pairs(*args)

    def sevens(shape):
        t = ex.dev.empty(shape)
        t.fill_(7.0)
        return t

    plain = make([(100, 1, 2, 2, 1, 1, 4)])              # grid slices 1, 2; coefficient slices 2, 3; rows 1 .. 4
    for gshape, cshape in (((1, 2, N, 1), (1, 4, 5, 1)), ((1, 3, N, 1), (1, 3, 5, 1)), ((1, 3, N, 1), (1, 4, 4, 1))):
        g, c = sevens(gshape), sevens(cshape)
        for call in (plain.forward, plain.backward):
            with pytest.raises(libhip.DdhError, match="slices exceed the array extents"):
                call(g, c) if call == plain.forward else call(c, g)
        ex.sync()
        assert np.all(ex.download(g) == 7.0) and np.all(ex.download(c) == 7.0)
    paired = make([(100, 0, 0, 1, 0, 1, 4)])
    paired.set_pairs([1], [1], [2], [1])
    g, c = sevens((1, 2, N, 9)), sevens((1, 2, 4, 9))     # ncols = 9
    with pytest.raises(libhip.DdhError, match="paired groups are implemented for the GEMV path"):
        paired.forward(g, c)
    with pytest.raises(libhip.DdhError, match="paired groups are implemented for the GEMV path"):
        paired.backward(c, g)
    g1, c1 = sevens((1, 1, N, 1)), sevens((1, 2, 4, 1))   # the partner's grid slice is beyond the array
    with pytest.raises(libhip.DdhError, match="slices exceed the array extents"):
        paired.forward(g1, c1)

    table = ex.make_recombination(np.zeros((2, 2), dtype=np.int32), np.ones((1, 2, 2)))
    d2, d3 = sevens((2, 2, 2, 5)), sevens((3, 2, 2, 5))
    with pytest.raises(libhip.DdhError, match="tensor rank 0, 1 or 2"):
        ex.regularity_recombine(d2, table)
    with pytest.raises(libhip.DdhError, match="ell map and Q table required"):
        ex.regularity_recombine(d3, None, sevens((5,)))
    ex.sync()
    for t in (g, c, g1, c1, d2, d3):
        assert np.all(ex.download(t) == 7.0)
