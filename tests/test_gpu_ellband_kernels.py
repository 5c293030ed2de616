"""GPU: the band LU kernels of dedalus_amd/csrc/ddh_ellband.hip against the longdouble references of
tests/ellband_cases.py, at the edges of their compiled windows, block loops and slot handling
(tests/test_ellband_cases_host.py proves the inputs and the references).

Bounds, none of them taken from the kernel's output (u = 2^-53):
  (i)   backward error eta = |A y - r|_inf / (|A|_inf |y|_inf + |r|_inf) of the kernel's y, in longdouble, per group and
        column: <= 8 max(eta of LAPACK's dgbtrf / dgbtrs on the same case, u).
  (ii)  max |x - x_ref| / max |x_ref| over the case <= 16 max(the same figure of the LAPACK baseline, 2 u).
  (iii) the recombination: |z - (y + sum_s P_s y_s)| <= (mp + 2) u (|y| + sum_s |P_s y_s|) entry by entry (a sum of
        mp + 1 terms in any order, with or without FMA contraction).
The kernel's y is the solution of the twin plan whose recombination band vanishes (same mp: the same kernels, and the
same y bit for bit, because P enters only the last addition of a row).  Inverting P on the host instead would multiply
the float64 rounding of z by |P^-1| ~ 1e3 (see the host test's docstring), for LAPACK's z as much as for the kernel's.
Right-hand sides are NaN wherever no live (group, row, slot) names them and x is prefilled with 7.0: no NaN may reach x,
dead slots hold 7.0 or +0.0, and nothing outside the named elements changes.
With DDH_ELLBAND_PARITY_OUT=<file> the figures per case are written there (profiles/ellband_kernel_parity.txt)."""
import ctypes as C
import os

import numpy as np
import pytest

import ellband_cases as ec

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
            fh.write("# tests/test_gpu_ellband_kernels.py: backward error eta and forward error of the device band LU beside LAPACK's\n")
            fh.write("# (dgbtrf / dgbtrs, float64) on the same case; both against the longdouble reference of tests/ellband_cases.py\n")
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
    return ex.make_ell_band(plan, plan.ncomp, nslots, plan.nl, plan.nr, lim, offsets=off)


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
        z = x[at[:, :k]]
        y = z if xy is None else xy[at[:, :k]]
        eta = max(eta, ec.backward_error(plan, g, a, b, cols[g], y))
        eta_b = max(eta_b, s["eta_b"])
        err = max(err, float(np.abs(z - s["z"]).max()))
        err_b = max(err_b, float(np.abs(s["zb"] - s["z"]).max()))
        ref = max(ref, float(np.abs(s["z"]).max()))
        if xy is not None:
            yl = y.astype(ec.LD)
            zl, mag = yl.copy(), np.abs(yl)
            for sd in range(min(plan.mp, n - 1)):
                p = plan.P[g, :n - 1 - sd, sd, None].astype(ec.LD) * yl[1 + sd:]
                zl[:n - 1 - sd] += p
                mag[:n - 1 - sd] += np.abs(p)
            zr = max(zr, float((np.abs(z - zl) / ((plan.mp + 2) * U * mag)).max()))
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
    rhs = ec.make_rhs(plan, nslots, lim, layout, cols)
    for (a, b), sol in zip(pairs, sols):
        band.factor(a, b, index=0)
        x = run_solve(ex, band, 0, rhs, size)
        xy = None
        if twin:
            twin.factor(a, b, index=0)
            xy = run_solve(ex, twin, 0, rhs, size)
        check("%s a=%g b=%g" % (label, a, b), plan, nslots, lim, layout, a, b, cols, sol, x, xy)
    return band


# ---- factor + solve over the table -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,layout", ec.CASE_LAYOUTS)
def test_factor_and_solve(ex, name, layout):
    plan, nslots, lim = ec.get_case(name, layout)
    sols = [ec.solved(name, layout, a, b) for a, b in ec.AB_PAIRS]
    band = factor_and_check(ex, "%s %s" % (name, layout), plan, nslots, lim, layout, ec.AB_PAIRS, ec.rhs_columns(name, layout), sols)
    info = band.info()
    assert (info["nw"], info["wt"]) == ec.CASES[name][2:4]


@pytest.mark.parametrize("name", ec.WIDEST)
def test_no_interchange_and_one_interchange_at_offset_kl(ex, name):
    plan, nslots, lim = ec.pivot_case(name)
    cols = ec.random_columns(plan, lim, 78)
    sols = [ec.solve_all(plan, lim, cols, a, b) for a, b in ec.AB_PAIRS]
    band = factor_and_check(ex, "%s pivots" % name, plan, nslots, lim, "default", ec.AB_PAIRS, cols, sols)
    info = band.info()
    assert (info["nw"], info["wt"]) == ec.CASES[name][2:4]


def test_factorizations_alive_together(ex):
    """two factorizations at once and a refill in place, with the recombination band in the factor rows: the refill must
    leave P (written once per storage) and the other factorization alone.  The twin handle without P goes through the
    same sequence and supplies y."""
    name = ec.ALIVE_CASE
    plan, nslots, lim = ec.case(name)
    assert plan.mp == 16
    cols = ec.rhs_columns(name)
    size = ec.offsets(plan, nslots, "default")[3]
    rhs = ec.make_rhs(plan, nslots, lim, "default", cols)
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
        check("%s alive %s" % (name, what), plan, nslots, lim, "default", a, b, cols, ec.solve_all(plan, lim, cols, a, b),
              runs[0][k], runs[1][k])


def test_zero_pivots_are_counted_not_faulted(ex):
    from dedalus_amd import libhip
    plan, nslots, lim, singular = ec.zero_pivot_case()
    cols = ec.random_columns(plan, lim, 79)
    a, b = ec.AB_PAIRS[0]
    size = ec.offsets(plan, nslots, "default")[3]
    rhs = ec.make_rhs(plan, nslots, lim, "default", cols)
    xs = []
    for p in (plan, plan.without_P()):
        band = make_band(ex, p, nslots, lim)
        with pytest.raises(libhip.DdhError):
            band.factor(a, b)
        bad = C.c_int(0)
        libhip.call("ddh_ellband_factor", band.handle, 0, float(a), float(b), C.byref(bad), ex.dev.stream)
        assert bad.value >= 2
        xs.append(run_solve(ex, band, 0, rhs, size))
    sol = ec.solve_all(plan, lim, cols, a, b, skip=singular)
    check("zero pivots in groups 1 and 3", plan, nslots, lim, "default", a, b, cols, sol, xs[0], xs[1], skip=singular)


def test_argument_checks_launch_nothing(ex):
    from dedalus_amd import libhip
    lim = [4]
    for kl, ku, mp, nbc, why in ((36, 0, 0, 0, "compiled windows"), (35, 62, 0, 0, "compiled windows"),
                                 (3, 4, 0, 9, "boundary rows"), (3, 4, 17, 0, "recombination band")):
        with pytest.raises(libhip.DdhError, match=why):
            make_band(ex, ec.SyntheticPlan(kl, ku, mp, nbc, [12], 1, 5), 4, lim)
    plan = ec.SyntheticPlan(3, 4, 0, 0, [12], 1, 5)
    band = make_band(ex, plan, 4, lim)
    size = ec.offsets(plan, 4, "default")[3]
    rhs, x = ex.from_host(np.zeros(size)), ex.from_host(np.full(size, 7.0))
    with pytest.raises(libhip.DdhError, match="no such factorization"):
        band.solve(0, rhs, x)                      # never factored
    with pytest.raises(libhip.DdhError, match="bad factorization index"):
        band.factor(1.0, 0.37, index=1)            # count + 1
    assert band.factor(1.0, 0.37) == 0
    with pytest.raises(libhip.DdhError, match="in-place"):
        band.solve(0, x, x)                        # in place
    with pytest.raises(libhip.DdhError):
        band.solve(1, rhs, x)
    with pytest.raises(libhip.DdhError):
        band.factor(1.0, 0.37, index=2)
    ex.sync()
    assert np.all(np.array(ex.download(x)) == 7.0)


# ---- ddh_ellband_gather_complex_inverse --------------------------------------------------------------------------------
@pytest.mark.parametrize("R,nl,nm,nslots", ec.GATHER_SHAPES)
def test_gather_complex_inverse(ex, R, nl, nm, nslots):
    from dedalus_amd import libhip
    from dedalus_amd.device import ptr
    off, count = ec.gather_offsets(R, nl, nm)
    assert ((R * nl) ** 2 > ec.GATHER_SINGLE_PASS) == (nl == 260)
    x = np.random.default_rng(nl).standard_normal(2 * R * nslots * nm * nl)
    out_d = ex.dev.empty(2 * count + ec.GUARD)
    out_d.fill_(float("nan"))
    x_d, off_d = ex.from_host(x), ex.from_host_int64(off)
    libhip.call("ddh_ellband_gather_complex_inverse", ptr(x_d), ptr(out_d), ptr(off_d), R, nl, nm, nslots, ex.dev.stream)
    ex.sync()
    got = np.array(ex.download(out_d)).reshape(-1)
    want = np.full(2 * count + ec.GUARD, np.nan)
    ec.gather_complex_inverse(x, R, nl, nm, nslots, want.view(np.complex128))
    assert np.isnan(got[2 * count:]).all() and not np.isnan(got[:2 * count]).any()
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))


# ---- ddh_ellband_bordered_inverse --------------------------------------------------------------------------------------
def _bordered(ex, X, n, j0, wM, wL, dM, dL, a, b):
    from dedalus_amd import libhip
    from dedalus_amd.device import ptr
    out_d = ex.dev.empty((n + 1) * (n + 1) + ec.GUARD)
    out_d.fill_(float("nan"))
    X_d, wM_d, wL_d = ex.from_host(X), ex.from_host(wM), ex.from_host(wL)
    libhip.call("ddh_ellband_bordered_inverse", ptr(X_d), n, j0, ptr(wM_d), ptr(wL_d), float(dM), float(dL), float(a), float(b),
                ptr(out_d), ex.dev.stream)
    ex.sync()
    return np.array(ex.download(out_d)).reshape(-1)


@pytest.mark.parametrize("n", ec.BORDERED_SIZES)
def test_bordered_inverse(ex, n):
    from dedalus_amd import libhip
    N = n + 1
    for j0 in sorted({0, n // 2, n - 1}):
        X, wM, wL, dM, dL, a, b = ec.bordered_inputs(n, j0)
        got = _bordered(ex, X, n, j0, wM, wL, dM, dL, a, b)
        assert np.isnan(got[N * N:]).all() and not np.isnan(got[:N * N]).any()
        got = got[:N * N].reshape(N, N)
        want = np.zeros((N, N))
        want[:n, :n] = X
        want[n, :n] = X[j0]
        rows = np.arange(N) != j0
        assert np.array_equal(got[rows].view(np.uint64), want[rows].view(np.uint64))
        row, mag = ec.bordered_row(X, wM, wL, dM, dL, a, b)
        assert np.all(np.abs(got[j0].astype(ec.LD) - row) <= 4 * n * U * mag), (n, j0)
    X, wM, wL, dM, dL, a, b = ec.bordered_inputs(n, 0)
    with pytest.raises(libhip.DdhError, match="gauge row"):
        _bordered(ex, X, n, 0, wM, wL, 0.0, 0.0, a, b)                # d = a dM + b dL = 0


def test_bordered_band_inverse_end_to_end(ex):
    from dedalus_amd.executor import BorderedBandInverse
    M, L, j0 = ec.bordered_system()
    n = M.shape[0] - 1
    a, b = ec.AB_PAIRS[0]
    inv = BorderedBandInverse(ex, M, L, n, j0)
    assert (inv.kl, inv.ku) == (5, 6)
    out = inv.compute(a, b)
    ex.sync()
    got = np.array(ex.download(out)).reshape(n + 1, n + 1)
    A = ec.LD(a) * M.astype(ec.LD) + ec.LD(b) * L.astype(ec.LD)
    ref = ec.ld_solve(A, np.eye(n + 1))
    err_np = float(np.abs(np.linalg.inv(a * M + b * L) - ref).max() / np.abs(ref).max())
    err = float(np.abs(got - ref).max() / np.abs(ref).max())
    print("bordered end to end: err %.3e (numpy inv %.3e)" % (err, err_np))
    RECORD.append(("bordered inverse n=130 (5, 6) end to end", 0.0, 0.0, err, err_np, 0.0))
    assert err <= 16 * max(err_np, 2 * U)
