"""GPU: the kernels of dedalus_amd/csrc/ddh_dense.hip (single-workgroup Gauss-Jordan instances <false, 12>, <false, 8>,
<true, 4> and the multi-launch path) and the chain that consumes their result (ell_blocks_kernel, ell_prune_kernel,
ell_gemm_kernel of csrc/ddh_sphere.hip, and the device copy into a CgemvBatch) against the longdouble references of
tests/dense_inverse_cases.py at their block edges (tests/test_dense_inverse_cases_host.py proves inputs and references).

Bounds, none of them taken from the kernel's output (u = 2^-53):
  (i)   inverse: err = max |X - X_ref| / max |X_ref| on the valid block <= 16 max(err_lapack, 2 u), err_lapack the same
        figure of numpy.linalg.inv on the float64 a M + b L.  Exact zeros outside [cv] x [rv]; M and L are NaN there and
        the output is prefilled with NaN and followed by 16 NaN doubles that must survive.
  (ii)  per-ell GEMM: rel-L2 < 1e-13 against the longdouble contraction (the bound of test_gpu_sphere.py::test_ell_terms),
        dead slots exactly +0 (or the untouched y0 when accumulating).
  (iii) inverse -> product: |y - y_ref| <= N * (i) * max |X_ref| * max |x| with N the row length of one product.
With DDH_DENSE_PARITY_OUT=<file> the figures of (i) are written there (profiles/dense_inverse_kernel_parity.txt)."""
import ctypes as C
import os

import numpy as np
import pytest

import dense_inverse_cases as dc

pytestmark = pytest.mark.gpu

U = dc.U
RECORD = []


@pytest.fixture(scope="module", autouse=True)
def parity_record():
    yield
    path = os.environ.get("DDH_DENSE_PARITY_OUT")
    if path:
        with open(path, "w") as fh:
            fh.write("# tests/test_gpu_dense_inverse_kernels.py: max |X - X_ld| / max |X_ld| on the valid block of the device\n")
            fh.write("# inverse beside numpy.linalg.inv (float64) on the same a M + b L; both against the longdouble reference\n")
            fh.write("%-44s %5s %-14s %10s %10s %8s\n" % ("# case", "n", "instance", "err", "err_lapack", "ratio"))
            for row in RECORD:
                fh.write("%-44s %5d %-14s %10.2e %10.2e %8.2f\n" % row)


@pytest.fixture(scope="module")
def ex():
    from dedalus_amd.executor import HipExecutor
    return HipExecutor()


def make_inverse(ex, systems, guard=True):
    inv = ex.make_dense_inverse([s.M for s in systems], [s.L for s in systems], [s.rv for s in systems],
                                [s.cv for s in systems], complex_=systems[0].cx)
    assert inv.count == sum(s.n * s.n for s in systems) * (2 if systems[0].cx else 1)
    if guard:
        inv._out = ex.dev.empty((inv.count + dc.GUARD,))
    return inv


def fetch(ex, inv, systems):
    """the output per system; the guard doubles behind it are still NaN and nothing else is"""
    ex.sync()
    flat = np.array(ex.download(inv._out)).reshape(-1)
    assert np.isnan(flat[inv.count:]).all() and flat[inv.count:].size == dc.GUARD, "the guard behind the output was written"
    assert not np.isnan(flat[:inv.count]).any(), "NaN in the output: a masked-out entry leaked or an element was not written"
    flat = flat[:inv.count].view(np.complex128) if systems[0].cx else flat[:inv.count]
    out, pos = [], 0
    for s in systems:
        out.append(flat[pos:pos + s.n * s.n].reshape(s.n, s.n))
        pos += s.n * s.n
    return out


def instance_of(systems, s):
    """the kernels that invert system s of this handle"""
    if s.n > dc.DI_NMAX:
        return "complex multi" if s.cx else "real multi"
    nmax = max(t.n for t in systems if t.n <= dc.DI_NMAX)
    return "complex bs4" if s.cx else "real bs%d" % dc.expected_bs(nmax, False)


def bound_of(s, a, b):
    err_b, scale = dc.lapack_error(s, a, b)
    return 16 * max(err_b, 2 * U), err_b, scale


def check_system(label, inst, s, a, b, got):
    outside = np.ones((s.n, s.n), bool)
    outside[np.ix_(s.cv, s.rv)] = False
    assert np.all(got[outside] == 0), (label, s.n, "not exactly zero outside the valid block")
    if s.nv == 0:
        return
    bound, err_b, scale = bound_of(s, a, b)
    err = float(np.abs(got[np.ix_(s.cv, s.rv)] - s.reference(a, b)).max()) / scale
    ratio = err / max(err_b, 2 * U)
    print("%s n=%d %s a=%g b=%g: err %.3e (LAPACK %.3e) ratio %.2f" % (label, s.n, inst, a, b, err, err_b, ratio))
    RECORD.append(("%s a=%g b=%g" % (label, a, b), s.n, inst, err, err_b, ratio))
    assert err <= bound, (label, s.n, a, b, err, err_b)


@pytest.mark.parametrize("name", list(dc.CASES))
def test_inverse(ex, name):
    systems = dc.case(name)
    inv = make_inverse(ex, systems)
    for a, b in dc.AB_PAIRS:                         # one handle, the second pair computed after the first
        inv._out.fill_(float("nan"))
        assert inv.compute(a, b) is inv._out
        for s, got in zip(systems, fetch(ex, inv, systems)):
            check_system(name, instance_of(systems, s), s, a, b, got)


@pytest.mark.parametrize("name", list(dc.SINGULAR_SETS))
def test_singular_system_is_counted_and_the_others_are_right(ex, name):
    from dedalus_amd import libhip
    systems = dc.singular_set(name)
    bad = dc.SINGULAR_SETS[name][2]
    inv = make_inverse(ex, systems)
    (a0, b0), (a1, b1) = dc.SINGULAR_PAIRS
    inv._out.fill_(float("nan"))
    with pytest.raises(libhip.DdhError, match=r"^1 subproblem matrices are singular"):
        inv.compute(a0, b0)
    count = C.c_int(-1)
    from dedalus_amd.device import ptr
    libhip.call("ddh_dense_inverse_compute", inv.handle, float(a0), float(b0), ptr(inv._out), C.byref(count), ex.dev.stream)
    assert count.value == 1
    ex.sync()
    flat = np.array(ex.download(inv._out)).reshape(-1)
    assert np.isnan(flat[inv.count:]).all()
    flat = flat[:inv.count].view(np.complex128) if systems[0].cx else flat[:inv.count]
    pos = 0
    for i, s in enumerate(systems):
        if i != bad:
            got = flat[pos:pos + s.n * s.n].reshape(s.n, s.n)
            assert not np.isnan(got).any()
            check_system("singular set %s, good" % name, instance_of(systems, s), s, a0, b0, got)
        pos += s.n * s.n
    # the flags are cleared per call: L is regular in all four
    inv._out.fill_(float("nan"))
    inv.compute(a1, b1)
    for s, got in zip(systems, fetch(ex, inv, systems)):
        check_system("singular set %s, after" % name, instance_of(systems, s), s, a1, b1, got)


# ---- the per-ell GEMM chain ---------------------------------------------------------------------------------------------
def rel(a, b):
    return float(np.linalg.norm((a - b).astype(np.float64)) / np.linalg.norm(b.astype(np.float64)))


def apply_terms(ex, terms, x, y0=None):
    """terms.apply into NaN, or the accumulating form into y0"""
    from dedalus_amd import libhip
    from dedalus_amd.device import ptr
    x_d = ex.from_host(np.array(x))                  # (copies: the shared inputs are read-only)
    if y0 is None:
        y_d = ex.dev.empty(x.shape)
        y_d.fill_(float("nan"))
        terms.apply(x_d, y_d)
    else:
        y_d = ex.from_host(np.array(y0))
        libhip.call("ddh_ell_terms_apply_acc", terms.handle, ptr(x_d), ptr(y_d), 1, ex.dev.stream)
    ex.sync()
    return np.array(ex.download(y_d))


@pytest.mark.parametrize("nm,nl,nr,ncomp", dc.GEMM_SHAPES)
def test_ell_gemm_chain(ex, nm, nl, nr, ncomp):
    from dedalus_amd.executor import DenseEllTerms
    (f0, f1, f2), x, y0 = dc.gemm_inputs(nm, nl, nr, ncomp)
    r0, r1, r2 = dc.gemm_references(nm, nl, nr, ncomp)
    live = dc.live_slots(nm, nl)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint64)

    def check(y, ref, what):
        assert not np.isnan(y).any(), (what, "NaN in y: a dead input slot was read or an element was not written")
        assert np.all(bits(y[:, ~live]) == 0), (what, "a dead slot is not +0")
        assert rel(y[:, live], ref[:, live]) < 1e-13, (what, rel(y[:, live], ref[:, live]))

    terms = ex.make_ell_terms_from_dense(nm, nl, nr, ncomp, ex.from_host(np.array(f0)))
    assert isinstance(terms, DenseEllTerms)
    check(apply_terms(ex, terms, x), r0, "first filling")
    # the refill brings back a block that was pruned and prunes one that was full
    again = ex.make_ell_terms_from_dense(nm, nl, nr, ncomp, ex.from_host(np.array(f1)), old=terms)
    assert again is terms
    check(apply_terms(ex, terms, x), r1, "refill")
    # accumulate = 1: y0 + A x on the live slots of components with a block; everything else keeps its bits
    ex.make_ell_terms_from_dense(nm, nl, nr, ncomp, ex.from_host(np.array(f2)), old=terms)
    y = apply_terms(ex, terms, x, y0)
    assert np.array_equal(bits(y[:, ~live]), bits(y0[:, ~live])), "accumulate touched a dead slot"
    want = y0.astype(dc.LD) + r2
    pruned = [ncomp - 1] if ncomp > 1 else []
    for c in range(ncomp):
        if c in pruned:
            assert np.array_equal(bits(y[c]), bits(y0[c])), "accumulate touched a component without blocks"
        else:
            assert rel(y[c][live], want[c][live]) < 1e-13, (c, rel(y[c][live], want[c][live]))
            assert not np.array_equal(y[c][live], y0[c][live])


def test_inverse_to_ell_terms_to_apply(ex):
    """DenseInverse.compute -> make_ell_terms_from_dense -> apply on four masked 128 x 128 per-ell groups among nl = 9"""
    from dedalus_amd.executor import DenseEllTerms
    nm, nl, nr, ncomp = dc.CHAIN_SHAPE
    N = ncomp * nr
    systems = dc.chain_systems()
    live = dc.live_slots(nm, nl)
    rng = np.random.default_rng(5)
    x = rng.standard_normal((ncomp, 2 * nm, nl, nr))
    x[:, ~live] = np.nan
    inv = make_inverse(ex, systems, guard=False)
    terms = None
    for a, b in dc.AB_PAIRS:
        terms = ex.make_ell_terms_from_dense(nm, nl, nr, ncomp, inv.compute(a, b), old=terms)
        assert isinstance(terms, DenseEllTerms)
        y = apply_terms(ex, terms, x)
        assert not np.isnan(y).any()
        assert np.all(np.ascontiguousarray(y[:, ~live]).view(np.uint64) == 0)
        for l, s in enumerate(systems):
            sl = np.flatnonzero(live[:, l])
            got = y[:, sl, l, :].transpose(0, 2, 1).reshape(N, sl.size)
            if s.nv == 0:
                assert np.all(got == 0), (l, "a group without valid rows gives zeros")
                continue
            Xe = s.embedded(s.reference(a, b))
            xv = x[:, sl, l, :].astype(dc.LD).transpose(0, 2, 1).reshape(N, sl.size)
            ref = Xe @ xv
            bound, err_b, scale = bound_of(s, a, b)
            err = float(np.abs(got - ref).max())
            lim = N * bound * scale * float(np.abs(xv).max())
            print("chain ell=%d a=%g b=%g: |y - y_ref| %.3e, bound %.3e" % (l, a, b, err, lim))
            assert err <= lim, (l, a, b, err, lim)


def test_inverse_to_cgemv_batch(ex):
    """the sphere's route: complex per-m inverses copied on the device into a CgemvBatch, refilled through old="""
    nm, nl, ncomp = dc.SPHERE_SHAPE
    systems = dc.sphere_systems()
    rng = np.random.default_rng(6)
    x = rng.standard_normal((ncomp, 2 * nm, nl))
    for m in range(nm):
        x[:, 2 * m:2 * m + 2, :m] = np.nan                                 # no mode there: never read
    inv = make_inverse(ex, systems, guard=False)
    batch = None
    for a, b in dc.AB_PAIRS:
        new = ex.make_cgemv_batch_flat(nm, nl, ncomp, inv.compute(a, b), old=batch)
        assert batch is None or new is batch
        batch = new
        y_d = ex.dev.empty(x.shape)
        y_d.fill_(float("nan"))
        batch.apply(ex.from_host(x), y_d)
        ex.sync()
        y = np.array(ex.download(y_d))
        assert not np.isnan(y).any()
        for m, s in enumerate(systems):
            assert np.all(y[:, 2 * m:2 * m + 2, :m] == 0)                  # no mode below the diagonal
            xv = (x[:, 2 * m, m:] + 1j * x[:, 2 * m + 1, m:]).reshape(-1).astype(dc.CLD)      # unknown j = comp (nl - m) + ell - m
            ref = s.embedded(s.reference(a, b)) @ xv
            got = (y[:, 2 * m, m:] + 1j * y[:, 2 * m + 1, m:]).reshape(-1)
            bound, err_b, scale = bound_of(s, a, b)
            err = float(np.abs(got - ref).max())
            lim = s.n * bound * scale * float(np.abs(xv).max())
            print("cgemv m=%d a=%g b=%g: |y - y_ref| %.3e, bound %.3e" % (m, a, b, err, lim))
            assert err <= lim, (m, a, b, err, lim)
