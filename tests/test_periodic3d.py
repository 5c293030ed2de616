"""CPU: triply periodic boxes (three RealFourier bases) on the NumPy test executor, i.e. through the band LU over the
Fourier pencil axis, against the reference's results in tests/golden/periodic3d.npz (tools/make_golden_periodic3d.py)."""
import os

import numpy as np
import pytest

import dedalus_amd.public as d3
import periodic3d_cases as pc
from oracle.np_executor import NumpyExecutor

TOL = 1e-10                 # of the field's maximum: the project's bound for reference end states


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "periodic3d.npz"))


def oracle_kw():
    return dict(executor=NumpyExecutor())


def assert_fields(res, gold, prefix, tol=TOL):
    for k, v in res.items():
        ref = gold[prefix + k]
        assert v.shape == ref.shape, (k, v.shape, ref.shape)
        scale = max(np.abs(ref).max(), 1e-300) if not k.startswith("tau") else 1.0
        err = np.abs(v - ref).max() / scale
        print("%s%s: %.2e" % (prefix, k, err))
        assert err <= tol, (prefix + k, err)


@pytest.mark.parametrize("shape", pc.TG_SHAPES)
@pytest.mark.parametrize("ts", pc.TG_STEPPERS)
def test_taylor_green_end_state(gold, shape, ts):
    solver, start, end = pc.run_ivp(d3, pc.taylor_green, shape=shape, timestepper=ts, dist_kw=oracle_kw())
    assert solver.dist.storage_order == (2, 0, 1) and solver.nf == 2
    assert solver.modal is None                         # (the test executor has no modal solve: band LU over the pencil)
    assert_fields(end, gold, "tg/%dx%dx%d/%s/" % (shape + (ts,)))


@pytest.mark.parametrize("ts", pc.BOUSSINESQ_STEPPERS)
def test_rotating_stratified_boussinesq_end_state(gold, ts):
    solver, start, end = pc.run_ivp(d3, pc.boussinesq, timestepper=ts, dist_kw=oracle_kw())
    assert_fields(end, gold, "boussinesq/%s/" % ts)


def test_adaptive_cfl_sequence(gold):
    solver, dts, end = pc.run_cfl(d3, dist_kw=oracle_kw())
    assert np.allclose(dts, gold["cfl/dts"], rtol=1e-11, atol=0), np.max(np.abs(dts - gold["cfl/dts"]))
    assert_fields(end, gold, "cfl/", tol=1e-9)


def test_periodic_poisson_lbvp(gold):
    solver, res = pc.run_poisson(d3, dist_kw=oracle_kw())
    assert_fields(res, gold, "lbvp/")


def _cell_combination(infos, nz, sign):
    """T with (T v)[component, z mode] = P (sign +1) or Q (sign -1) of the reference's slots v[component][x part][y part]
    [z mode] of every field in `infos` = [(ncomp, has bases)]; the msin slot of kz = 0 (no mode) is left out."""
    rows, cols, vals, msin = [], [], [], []
    r = c0 = 0
    for ncomp, full in infos:
        if not full:
            rows.append(r); cols.append(c0); vals.append(1.0)
            msin.append((False, False))
            r += 1
            c0 += 1
            continue
        msin += [(xs == 1, ys == 1) for c in range(ncomp) for xs in range(2) for ys in range(2) for zi in range(nz)]
        for c in range(ncomp):
            for zi in range(nz):
                if zi != 1:
                    for (xs, ys, w) in ((0, 0, 1.0), (0, 1, 1j), (1, 0, 1j * sign), (1, 1, -1.0 * sign)):
                        rows.append(r); cols.append(c0 + ((c * 2 + xs) * 2 + ys) * nz + zi); vals.append(w)
                    r += 1
        c0 += ncomp * 4 * nz
    T = np.zeros((r, c0), dtype=complex)
    T[rows, cols] = vals
    return T, np.array(msin)


def test_pencil_matrices_equal_the_reference_subproblem_matrices(gold):
    """The assembled M and L of a (kx, ky) pencil against the reference's real matrices R of the same group.  Documented
    map: fields in problem order; the reference keeps 2 x 2 real slots (cos / msin along x, y) per z mode, this project
    the complex systems P = (cc - ss) + i (cs + sc) and Q = (cc + ss) + i (cs - sc) with symbols lambda(+-kx, ky):
    T R = A(+-kx, ky) T for T = the P (Q) combination of the slots; the msin slot of kz = 0 holds no mode on either side."""
    solver, f = pc.taylor_green(d3, (12, 20, 8), "RK222", dist_kw=oracle_kw())
    nz = 8
    nf, nx, ny, kx, ky = solver.evaluator_core.geom()
    for (gx, gy) in pc.MATRIX_GROUPS:
        mean = (gx, gy) == (0, 0)

        def ours(infos):
            idx = []
            for i in infos:
                if i["interior"]:
                    idx += [i["row0"] + c * nz + zi for c in range(i["ncomp"]) for zi in range(nz) if zi != 1]
                elif mean:
                    idx += list(range(i["row0"], i["row0"] + i["rows"]))
            return idx

        layout = lambda infos: [(i["ncomp"], i["interior"]) for i in infos if i["interior"] or mean]
        ri, ci = ours(solver.eq_info), ours(solver.var_info)
        for name, tl in (("M", solver.M_tl), ("L", solver.L_tl)):
            R = gold["mat/%d_%d/%s" % (gx, gy, name)]
            for sign in (1, -1):
                A = tl.dense(kx[gx], ky[gy], gx, gy, sign)[np.ix_(ri, ci)]
                Te, _ = _cell_combination(layout(solver.eq_info), nz, sign)
                Tv, msin = _cell_combination(layout(solver.var_info), nz, sign)
                assert Te.shape[1] == R.shape[0] and Tv.shape[1] == R.shape[1], (Te.shape, Tv.shape, R.shape)
                # columns of the slot without a mode act on nothing: compared on vectors that are zero there
                live = np.abs(Tv).sum(axis=0) > 0
                if gx == 0:                             # (likewise the msin slots of kx = 0 and of ky = 0)
                    live &= ~msin[:, 0]
                if gy == 0:
                    live &= ~msin[:, 1]
                err = np.abs((Te @ R)[:, live] - (A @ Tv)[:, live]).max()
                assert err <= 1e-12 * np.abs(R).max(), (name, gx, gy, sign, err)
                assert np.abs(A).max() > 0


def test_invalid_mode_is_inert_and_band_is_narrow():
    solver, f = pc.taylor_green(d3, (12, 20, 8), "RK222", dist_kw=oracle_kw())
    assert len(solver.inert_rows) == 4 and len(solver.inert_cols) == 4      # msin slot of kz = 0: u (3), p
    for tl in (solver.M_tl,):
        assert not np.isin(tl.row, solver.inert_rows).any() and not np.isin(tl.col, solver.inert_cols).any()
    L = solver.L_tl
    on = np.isin(L.row, solver.inert_rows) | np.isin(L.col, solver.inert_cols)
    assert on.sum() == 4 and np.all(L.coef[on] == 1.0) and np.isin(L.row[on], solver.inert_rows).all() \
        and np.isin(L.col[on], solver.inert_cols).all()
    assert solver.real_grading is not None and solver.kl <= solver.BAND_KLMAX


def test_one_and_two_fourier_axes_take_the_old_path():
    import problems
    solver, f = problems.poisson_2d(d3, dist_kw=oracle_kw())
    assert not solver.dist._pencil_fourier and len(solver.inert_rows) == 0 and solver.modal is None
    solver, f = problems.kdv_burgers(d3, dist_kw=oracle_kw())
    assert not solver.dist._pencil_fourier and solver.dist.storage_order == (0,)


def test_refusals_keep_their_messages():
    coords, dist, B = pc._bases(d3, (8, 8, 8), oracle_kw())
    u = dist.Field(name='u', bases=B)
    tau = dist.Field(name='tau')
    problem = d3.LBVP([u, tau], namespace=dict(u=u, tau=tau, lap=d3.lap, integ=d3.integ))
    problem.add_equation("lap(u) + tau = 0")
    with pytest.raises(NotImplementedError, match="interpolation along a Fourier axis couples all modes"):
        problem.add_equation("u(z=0) = 0")
        problem.build_solver()
