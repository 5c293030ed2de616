"""GPU: the complex instances of the band LU kernels of dedalus_amd/csrc/ddh_ellband.hip (ddh_ellband_create_complex)
against the clongdouble references of tests/ellband_complex_cases.py, at the edges of their compiled windows, block loops
and pair handling (tests/test_ellband_complex_cases_host.py proves the inputs and the references).

Bounds: those of tests/test_gpu_ellband_kernels.py with LAPACK's complex routines as the baseline, none of them taken from
the kernel's output (u = 2^-53):
  (i)   backward error eta = |A y - r|_inf / (|A|_inf |y|_inf + |r|_inf) of the kernel's y, in clongdouble, per group and
        column: <= 8 max(eta of zgbtrf / zgbtrs on the same case, u).
  (ii)  max |x - x_ref| / max |x_ref| over the case <= 16 max(the same figure of the LAPACK baseline, 2 u).
  (iii) the recombination (real P on either part): |z - (y + sum_s P_s y_s)| <= (mp + 2) u (|y| + sum_s |P_s y_s|), entry by
        entry and per real slot.
The kernel's y is the solution of the twin plan whose recombination band vanishes.  Right-hand sides are NaN wherever no
live (group, row, pair) names them and x is prefilled with 7.0: no NaN may reach x, dead slots hold 7.0 or +0.0, and
nothing outside the named elements changes.
With DDH_ELLBAND_PARITY_OUT=<file> the figures per case are written there (profiles/ellband_complex_kernel_parity.txt)."""
import ctypes as C
import os

import numpy as np
import pytest

import ellband_cases as ec
import ellband_complex_cases as cc

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
SEVEN = np.float64(7.0).view(np.uint64)
RECORD = []


@pytest.fixture(scope="module", autouse=True)
def parity_record():
    yield
    path = os.environ.get("DDH_ELLBAND_PARITY_OUT")
    if path:
        with open(path, "w") as fh:
            fh.write("# tests/test_gpu_ellband_complex_kernels.py: backward error eta and forward error of the complex device band LU\n")
            fh.write("# beside LAPACK's (zgbtrf / zgbtrs, complex128) on the same case; both against the clongdouble reference of\n")
            fh.write("# tests/ellband_complex_cases.py\n")
            fh.write("%-44s %10s %10s %10s %10s %8s\n" % ("# case", "eta", "eta_lapack", "err", "err_lapack", "z_bound"))
            for row in RECORD:
                fh.write("%-44s %10.2e %10.2e %10.2e %10.2e %8.3f\n" % row)


@pytest.fixture(scope="module")
def ex():
    from dedalus_amd.executor import HipExecutor
    return HipExecutor()


def make_band(ex, plan, nslots, lim, layout="default"):
    rowoff, coloff, stride, size = ec.offsets(plan, nslots, layout)
    off = None if layout == "default" else (rowoff, coloff, stride)
    band = ex.make_ell_band(plan, plan.ncomp, nslots, plan.nl, plan.nr, lim, offsets=off)
    assert band.cx
    return band


def run_solve(ex, band, index, rhs, size):
    rhs_d = ex.from_host(rhs)
    x_d = ex.dev.empty(size)
    x_d.fill_(7.0)
    band.solve(index, rhs_d, x_d)
    ex.sync()
    return np.array(ex.download(x_d)).reshape(-1)


def check(label, plan, nslots, lim, layout, a, b, cols, sol, x, xy, skip=()):
    """x: the kernel's solution vector, xy: that of the twin plan without P (None where mp = 0)"""
    rowoff, coloff, stride, size = ec.offsets(plan, nslots, layout)
    assert x.size == size and not np.isnan(x).any(), "NaN in x: a poisoned element was read"
    named = np.zeros(size, bool)
    eta = eta_b = err = err_b = ref = zr = 0.0
    for g in range(plan.nl):
        n, k = int(plan.n[g]), int(lim[g])
        if n == 0:
            continue
        at = coloff[g, :n, None] + np.arange(nslots)[None, :] * stride
        named[at] = True
        dead = x[at[:, k:]].view(np.uint64)
        assert np.all((dead == SEVEN) | (dead == 0)), (g, "dead slots hold something else than 7.0 or +0.0")
        if k == 0 or g in skip:
            continue
        s = sol[g]
        zs = x[at[:, :k]]                                           # real slots
        ys = zs if xy is None else xy[at[:, :k]]
        z, y = cc.from_slots(zs), cc.from_slots(ys)
        eta = max(eta, cc.backward_error(plan, g, a, b, cols[g], y))
        eta_b = max(eta_b, s["eta_b"])
        err = max(err, float(np.abs(z - s["z"]).max()))
        err_b = max(err_b, float(np.abs(s["zb"] - s["z"]).max()))
        ref = max(ref, float(np.abs(s["z"]).max()))
        if xy is not None:
            yl = ys.astype(ec.LD)
            zl, mag = yl.copy(), np.abs(yl)
            for sd in range(min(plan.mp, n - 1)):
                p = plan.P[g, :n - 1 - sd, sd, None].astype(ec.LD) * yl[1 + sd:]
                zl[:n - 1 - sd] += p
                mag[:n - 1 - sd] += np.abs(p)
            zr = max(zr, float((np.abs(zs - zl) / ((plan.mp + 2) * U * mag)).max()))
    assert np.all(x[~named].view(np.uint64) == SEVEN), "an element no (group, row) names was written"
    err, err_b = err / ref, err_b / ref
    print("%s eta %.3e (LAPACK %.3e) err %.3e (LAPACK %.3e) z/bound %.3f" % (label, eta, eta_b, err, err_b, zr))
    RECORD.append((label, eta, eta_b, err, err_b, zr))
    assert zr <= 1.0, (label, zr)
    assert eta <= 8 * max(eta_b, U), (label, eta, eta_b)
    assert err <= 16 * max(err_b, 2 * U), (label, err, err_b)


def factor_and_check(ex, label, plan, nslots, lim, layout, pairs, cols, sols):
    band = make_band(ex, plan, nslots, lim, layout)
    twin = make_band(ex, plan.without_P(), nslots, lim, layout) if plan.mp else None
    size = ec.offsets(plan, nslots, layout)[3]
    rhs = cc.make_rhs(plan, nslots, lim, layout, cols)
    for (a, b), sol in zip(pairs, sols):
        band.factor(a, b, index=0)
        x = run_solve(ex, band, 0, rhs, size)
        assert np.array_equal(run_solve(ex, band, 0, rhs, size).view(np.uint64), x.view(np.uint64)), "repeated solves differ"
        xy = None
        if twin:
            twin.factor(a, b, index=0)
            xy = run_solve(ex, twin, 0, rhs, size)
        check("%s a=%g b=%g" % (label, a, b), plan, nslots, lim, layout, a, b, cols, sol, x, xy)
    return band


@pytest.mark.parametrize("name,layout", cc.CX_CASE_LAYOUTS)
def test_factor_and_solve(ex, name, layout):
    plan, nslots, lim = cc.get_case(name, layout)
    sols = [cc.solved(name, layout, a, b) for a, b in ec.AB_PAIRS]
    band = factor_and_check(ex, "cx %s %s" % (name, layout), plan, nslots, lim, layout, ec.AB_PAIRS, cc.rhs_columns(name, layout), sols)
    info = band.info()
    assert (info["nw"], info["wt"]) == ec.CASES[name][2:4]


@pytest.mark.parametrize("name", cc.CX_WIDEST)
def test_no_interchange_and_one_interchange_at_offset_kl(ex, name):
    plan, nslots, lim = cc.pivot_case(name)
    cols = cc.random_columns(plan, lim, 78)
    sols = [cc.solve_all(plan, lim, cols, a, b) for a, b in ec.AB_PAIRS]
    band = factor_and_check(ex, "cx %s pivots" % name, plan, nslots, lim, "default", ec.AB_PAIRS, cols, sols)
    info = band.info()
    assert (info["nw"], info["wt"]) == ec.CASES[name][2:4]


def test_factorizations_alive_together(ex):
    """two factorizations at once and a refill in place (see tests/test_gpu_ellband_kernels.py)"""
    name = cc.ALIVE_CASE
    plan, nslots, lim = cc.case(name)
    assert plan.mp == 16
    cols = cc.rhs_columns(name)
    size = ec.offsets(plan, nslots, "default")[3]
    rhs = cc.make_rhs(plan, nslots, lim, "default", cols)
    runs = []
    for p in (plan, plan.without_P()):
        band = make_band(ex, p, nslots, lim)
        assert (band.info()["nw"], band.info()["wt"]) == (28, 56)
        assert band.factor(1.0, 0.37) == 0 and band.factor(1.0, 0.11) == 1
        x0, x1 = run_solve(ex, band, 0, rhs, size), run_solve(ex, band, 1, rhs, size)
        assert band.factor(0.5, 1.0, index=0) == 0 and band.count == 2
        x0n = run_solve(ex, band, 0, rhs, size)
        assert np.array_equal(run_solve(ex, band, 1, rhs, size).view(np.uint64), x1.view(np.uint64))
        assert np.array_equal(run_solve(ex, band, 0, rhs, size).view(np.uint64), x0n.view(np.uint64))
        assert not np.array_equal(x0n, x0)
        runs.append((x0, x1, x0n))
    for k, (what, a, b) in enumerate((("index 0", 1.0, 0.37), ("index 1", 1.0, 0.11), ("index 0 refilled", 0.5, 1.0))):
        check("cx %s alive %s" % (name, what), plan, nslots, lim, "default", a, b, cols, cc.solve_all(plan, lim, cols, a, b),
              runs[0][k], runs[1][k])


def test_zero_pivots_are_counted_not_faulted(ex):
    from dedalus_amd import libhip
    plan, nslots, lim, singular = cc.zero_pivot_case()
    cols = cc.random_columns(plan, lim, 79)
    a, b = ec.AB_PAIRS[0]
    size = ec.offsets(plan, nslots, "default")[3]
    rhs = cc.make_rhs(plan, nslots, lim, "default", cols)
    xs = []
    for p in (plan, plan.without_P()):
        band = make_band(ex, p, nslots, lim)
        with pytest.raises(libhip.DdhError):
            band.factor(a, b)
        bad = C.c_int(0)
        libhip.call("ddh_ellband_factor", band.handle, 0, float(a), float(b), C.byref(bad), ex.dev.stream)
        assert bad.value >= 2
        xs.append(run_solve(ex, band, 0, rhs, size))
    sol = cc.solve_all(plan, lim, cols, a, b, skip=singular)
    check("cx zero pivots in groups 1 and 3", plan, nslots, lim, "default", a, b, cols, sol, xs[0], xs[1], skip=singular)


def test_argument_checks_launch_nothing(ex):
    from dedalus_amd import libhip
    for kl, ku, mp, nbc, nslots, lim, why in ((36, 0, 0, 0, 4, [4], "compiled windows"), (35, 30, 0, 0, 4, [4], "complex windows"),
                                              (35, 61, 0, 0, 4, [4], "complex windows"), (3, 4, 0, 9, 4, [4], "boundary rows"),
                                              (3, 4, 17, 0, 4, [4], "recombination band"), (3, 4, 0, 0, 5, [4], "odd number of slots"),
                                              (3, 4, 0, 0, 4, [3], "odd slot limit")):
        with pytest.raises(libhip.DdhError, match=why):
            make_band(ex, cc.ComplexPlan(kl, ku, mp, nbc, [12], 1, 5), nslots, lim)
    plan = cc.ComplexPlan(3, 4, 0, 0, [12], 1, 5)
    lim = [4]
    band = make_band(ex, plan, 4, lim)
    size = ec.offsets(plan, 4, "default")[3]
    rhs, x = ex.from_host(np.zeros(size)), ex.from_host(np.full(size, 7.0))
    with pytest.raises(libhip.DdhError, match="no such factorization"):
        band.solve(0, rhs, x)
    with pytest.raises(libhip.DdhError, match="bad factorization index"):
        band.factor(1.0, 0.37, index=1)
    assert band.factor(1.0, 0.37) == 0
    with pytest.raises(libhip.DdhError, match="in-place"):
        band.solve(0, x, x)
    ex.sync()
    assert np.all(np.array(ex.download(x)) == 7.0)
