"""GPU: triply periodic boxes on HipExecutor -- the matrix-free modal solve (csrc/ddh_modal.hip) and, with DDH_MODAL=0,
the band LU over the Fourier pencil axis -- against the reference's results in tests/golden/periodic3d.npz."""
import ctypes as C
import os

import numpy as np
import pytest

import periodic3d_cases as pc
from test_periodic3d import assert_fields

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "periodic3d.npz"))


def modal_launches():
    from dedalus_amd import libhip
    n = C.c_long(0)
    libhip.call("ddh_modal_launches", C.byref(n))
    return n.value


def assert_modal_ran(solver, n0):
    assert solver.modal is not None and modal_launches() > n0
    assert solver.factor_bytes() == 0 and getattr(solver, "factor_calls", 0) == 0


@pytest.mark.parametrize("shape", pc.TG_SHAPES)
@pytest.mark.parametrize("ts", pc.TG_STEPPERS)
def test_taylor_green_modal(gold, shape, ts):
    import dedalus_amd.public as d3
    n0 = modal_launches()
    solver, start, end = pc.run_ivp(d3, pc.taylor_green, shape=shape, timestepper=ts)
    assert_modal_ran(solver, n0)
    assert_fields(end, gold, "tg/%dx%dx%d/%s/" % (shape + (ts,)))


@pytest.mark.parametrize("ts", pc.BOUSSINESQ_STEPPERS)
def test_boussinesq_modal(gold, ts):
    import dedalus_amd.public as d3
    n0 = modal_launches()
    solver, start, end = pc.run_ivp(d3, pc.boussinesq, timestepper=ts)
    assert_modal_ran(solver, n0)
    assert solver.modal.plan.rc == 6
    assert_fields(end, gold, "boussinesq/%s/" % ts)


def test_adaptive_cfl_modal_never_factors(gold):
    import dedalus_amd.public as d3
    n0 = modal_launches()
    solver, dts, end = pc.run_cfl(d3)
    assert len(set(np.round(dts, 12))) > 2              # the timestep did change mid-run ...
    assert_modal_ran(solver, n0)                        # ... and no factor call was made
    assert np.allclose(dts, gold["cfl/dts"], rtol=1e-11, atol=0), np.max(np.abs(dts - gold["cfl/dts"]))
    assert_fields(end, gold, "cfl/", tol=1e-9)


def test_poisson_lbvp_modal(gold):
    import dedalus_amd.public as d3
    n0 = modal_launches()
    solver, res = pc.run_poisson(d3)
    assert_modal_ran(solver, n0)
    assert_fields(res, gold, "lbvp/")


@pytest.mark.parametrize("case", ["tg", "boussinesq", "lbvp"])
def test_band_lu_fallback_with_ddh_modal_0(gold, monkeypatch, case):
    import dedalus_amd.public as d3
    monkeypatch.setenv("DDH_MODAL", "0")
    n0 = modal_launches()
    if case == "tg":
        solver, start, end = pc.run_ivp(d3, pc.taylor_green, shape=(12, 20, 8), timestepper="RK222")
        prefix = "tg/12x20x8/RK222/"
    elif case == "boussinesq":
        solver, start, end = pc.run_ivp(d3, pc.boussinesq, timestepper="RK222")
        prefix = "boussinesq/RK222/"
    else:
        solver, end = pc.run_poisson(d3)
        prefix = "lbvp/"
    assert solver.modal is None and modal_launches() == n0
    assert solver.factor_calls > 0 and solver.factor_bytes() > 0
    assert_fields(end, gold, prefix)


def test_flow_properties_file_handler_and_load_state(tmp_path):
    """GlobalFlowProperty, a file handler with full and reduced tasks (an integral over the box, a slice across the Fourier
    pencil axis) and load_state, on a periodic box; the reduced tasks against the grid data of the same state."""
    import dedalus_amd.public as d3
    from dedalus_amd.tools import h5lite
    solver, f = pc.taylor_green(d3, (12, 20, 8), "RK222")
    u = f["u"]
    flow = d3.GlobalFlowProperty(solver, cadence=1)
    flow.add_property(u @ u, name="ke")
    snap = solver.evaluator.add_file_handler(str(tmp_path / "snap"), iter=4)
    snap.add_tasks(solver.state)
    snap.add_task(d3.integ(u @ u), name="E")
    z1 = pc.LZ / 8                                      # the second grid plane at scale 1
    snap.add_task(u(z=z1), name="slice", layout="g", scales=1)
    for _ in range(5):
        solver.step(pc.DT)                              # (handlers run at the start of a step: writes at iterations 0 and 4)
    snap.close()                                        # (the last write is staged asynchronously)
    r = h5lite.read(str(tmp_path / "snap" / "snap_s1.h5"))
    assert np.array_equal(r["scales/iteration"].read(), [0, 4])
    solver2, f2 = pc.taylor_green(d3, (12, 20, 8), "RK222")
    solver2.load_state(str(tmp_path / "snap" / "snap_s1.h5"), index=1)
    assert solver2.iteration == 4 and abs(solver2.sim_time - 4 * pc.DT) < 1e-14
    solver2.step(pc.DT)
    assert np.abs(np.array(f2["u"]["c"]) - np.array(u["c"])).max() <= 1e-13
    # the written reductions belong to the state at iteration 4 = the loaded state before its step: recompute from a reload
    solver3, f3 = pc.taylor_green(d3, (12, 20, 8), "RK222")
    solver3.load_state(str(tmp_path / "snap" / "snap_s1.h5"), index=1)
    f3["u"].change_scales(1)
    g = np.array(f3["u"]["g"])
    E = float(np.asarray(r["tasks/E"].read(1)).ravel()[0])
    assert abs(E - (g ** 2).sum(axis=0).mean() * pc.LX * pc.LY * pc.LZ) <= 1e-12 * abs(E)
    sl = np.asarray(r["tasks/slice"].read(1)).reshape(3, 12, 20)
    assert np.abs(sl - g[:, :, :, 1]).max() <= 1e-13
    assert 0.5 < flow.max("ke") < 1.5                   # (|u|^2 of the vortex, sampled at the start of the last step)


def test_repeated_runs_and_graph_replay_are_bit_identical():
    import dedalus_amd.public as d3
    runs = []
    for graph in (False, False, True):
        solver, f = pc.taylor_green(d3, (16, 16, 8), "RK222")
        solver.enable_step_graph(graph)
        for _ in range(8):
            solver.step(pc.DT)
        if graph:
            assert solver._graph["graphs"] and not solver._graph["failed"]
        assert solver.modal is not None
        runs.append({k: np.array(v['c']) for k, v in f.items()})
    for k in runs[0]:
        assert np.array_equal(runs[0][k], runs[1][k]), k
        assert np.array_equal(runs[0][k], runs[2][k]), k


def test_solve_lincomb_term_counts_and_probe_on_the_modal_solve():
    """SolverBase.solve_lincomb on the modal solve at 12 x 20 x 8: 1 and 8 terms go to the kernel as they are, 9 terms (more
    than it takes) and a probed call through one materialised right-hand side.  Same right-hand side, same solution, and a
    modal launch every time."""
    import dedalus_amd.public as d3
    from test_periodic3d import TOL
    solver, f = pc.taylor_green(d3, (12, 20, 8), "RK222")
    assert solver.modal is not None and solver.modal.MAX_RHS_TERMS == 8
    ex, shape = solver.ex, (solver.R, solver.nx, solver.ny)
    lu = solver.factor(1.0, 0.5 * pc.DT)
    rhs = np.random.default_rng(11).normal(size=shape)
    parts = [ex.from_host(rhs * w) for w in (0.5, 0.25, 0.125, 0.0625, 0.03125, 0.015625, 0.0078125, 0.00390625, 0.00390625)]
    whole = ex.from_host(rhs)

    def run(xs, alphas):
        out, n0 = ex.zeros(shape), modal_launches()
        solver.solve_lincomb(lu, xs, alphas, out)
        ex.sync()
        assert modal_launches() > n0
        return np.array(ex.download(out))

    x1 = run([whole], [1.0])
    x8 = run(parts[:7] + [parts[7]], [1.0] * 7 + [2.0])
    x9 = run(parts, [1.0] * 9)
    solver.solve_probe = dict(groups=pc.MATRIX_GROUPS, records=[])
    xp = run(parts[:7] + [parts[7]], [1.0] * 7 + [2.0])
    recs, solver.solve_probe = solver.solve_probe["records"], None
    assert [r["path"] for r in recs] == ["ddh_pencil_solve_recombined (one materialised right-hand side)"]
    assert recs[0]["terms"] == 1 and (recs[0]["a"], recs[0]["b"]) == (1.0, 0.5 * pc.DT)
    assert solver.factor_calls == 0 and solver.factor_bytes() == 0
    scale = np.abs(x1).max()
    assert scale > 0 and np.isfinite(x1).all()
    for name, x in (("8 terms", x8), ("9 terms", x9), ("probed", xp)):
        err = np.abs(x - x1).max() / scale
        print("%s: %.2e" % (name, err))
        assert err <= TOL, (name, err)
