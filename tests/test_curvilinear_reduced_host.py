"""Reduced analysis tasks of sphere and shell fields on the NumPy oracle executor: the host logic (stages, weights, scaling,
shapes) against the unmodified reference (tests/golden/curvilinear_reduced.npz, tools/make_golden_curvilinear_reduced.py),
against the full grid data where the reduction falls on a grid node, and the refusals.

Bound against the reference: max-abs error <= 1e-11 x max|golden| (the figure tests/test_shell_fields.py::check_analysis uses
for the shell's analysis tasks); self-consistency: 1e-12 relative."""
import os

import numpy as np
import pytest

import curvilinear_reduced_cases as cc
from oracle.np_executor import NumpyExecutor

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "curvilinear_reduced.npz")
TOL = 1e-11


@pytest.fixture(scope="module")
def d3():
    import dedalus_amd.public as d3
    return d3


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def _kw():
    return dict(executor=NumpyExecutor())


def _setup(d3, gold, case, dist_kw=None):
    dist, coords, basis, f = cc.build(d3, case, dist_kw=_kw() if dist_kw is None else dist_kw)
    cc.load_inputs(gold, case, f)
    return dist, coords, basis, f


def compare(gold, case, name, out, what="evaluate"):
    """every scale the golden file holds for this task"""
    keys = [cc.out_key(s) for s in cc.SCALES if "%s/%s/%s" % (case, name, cc.out_key(s)) in gold.files]
    assert "g15" in keys
    for scale in cc.SCALES:
        if cc.out_key(scale) not in keys:
            continue
        ref = gold["%s/%s/%s" % (case, name, cc.out_key(scale))]
        out.change_scales(scale)
        got = np.asarray(out["g"])
        assert got.shape == ref.shape, (what, case, name, scale, got.shape, ref.shape)
        err = np.abs(got - ref).max() / np.abs(ref).max()
        print("%s %s/%s scale %g: max-abs error / max|golden| = %.3e" % (what, case, name, scale, err))
        assert err <= TOL, (what, case, name, scale, err)


def test_golden_inputs_have_energy_everywhere(gold):
    for case in cc.CASES:
        for k in cc.input_names(case):
            c = gold["%s/in/%s" % (case, k)]
            assert c.dtype == np.float32 and np.count_nonzero(c) > 0.4 * c.size
    for case in ("shell_16_12_8", "shell_16_10_6"):
        assert np.abs(gold[case + "/ave_S2_b/g15"]).max() > 0.5          # (not a comparison of zeros)


@pytest.mark.parametrize("case", list(cc.CASES))
def test_tasks_match_reference(d3, gold, case):
    dist, coords, basis, f = _setup(d3, gold, case)
    tasks = cc.tasks(d3, case, coords, f)
    assert len(tasks) == (11 if cc.CASES[case][0] == "shell" else 9)
    for name, expr in tasks.items():
        compare(gold, case, name, expr.evaluate())


@pytest.mark.parametrize("case", list(cc.CASES))
def test_reductions_on_grid_nodes_are_rows_of_the_grid_data(d3, gold, case):
    dist, coords, basis, f = _setup(d3, gold, case)
    for scale in cc.SCALES:
        grids = basis.grids((scale,) * dist.dim)
        for k in cc.input_names(case):
            fld = f[k]
            fld.change_scales(scale)
            g = np.array(fld["g"])
            fld["c"] = gold["%s/in/%s" % (case, k)].astype(np.float64)      # (back to the coefficients as given)
            ax = fld.rank
            jp, jt = 5, 3
            for what, expr, ref in (
                    ("theta", fld(theta=float(grids[1][jt])), np.take(g, [jt], axis=ax + 1)),
                    ("phi", fld(phi=float(grids[0][jp])), np.take(g, [jp], axis=ax)),
                    ("zonal mean", d3.ave(fld, "phi"), g.mean(axis=ax, keepdims=True))):
                out = expr.evaluate()
                out.change_scales(scale)
                got = np.asarray(out["g"])
                assert got.shape == ref.shape
                err = np.abs(got - ref).max() / np.abs(ref).max()
                print("%s %s %s scale %g: %.3e" % (case, k, what, scale, err))
                assert err <= 1e-12, (case, k, what, scale, err)


def test_shell_average_is_the_quadrature_mean(d3, gold):
    """ave(b, S2) against the Gauss-weighted mean of the grid data over every sphere r = const (scale 1)"""
    from dedalus_amd.tools import sphere as sph
    case = "shell_16_12_8"
    dist, coords, basis, f = _setup(d3, gold, case)
    g = np.array(f["b"]["g"])
    f["b"]["c"] = gold[case + "/in/b"].astype(np.float64)
    _, w = sph.quadrature(g.shape[1])
    ref = (g.mean(axis=0) * np.asarray(w, dtype=np.float64)[:, None]).sum(axis=0) / 2
    for expr in (d3.ave(f["b"], coords.S2coordsys), d3.Average(f["b"], coords.S2coordsys), d3.ave(f["b"])):
        got = np.asarray(expr.evaluate()["g"])
        assert got.shape == (1, 1, 8)
        assert np.abs(got[0, 0] - ref).max() <= 1e-12 * np.abs(ref).max()


def test_coordinate_spellings(d3, gold):
    case = "shell_16_12_8"
    dist, coords, basis, f = _setup(d3, gold, case)
    b = f["b"]
    ref = np.asarray(d3.Average(b, coords["phi"]).evaluate()["g"])
    for expr in (d3.ave(b, "phi"), d3.ave(b, coords["phi"]), d3.Average(b, "phi")):
        assert np.array_equal(np.asarray(expr.evaluate()["g"]), ref)
    assert type(d3.ave(b, coords.S2coordsys)) is type(d3.ave(b, ("phi", "theta")))


def test_composed_reductions_and_tensors_raise_by_name(d3, gold):
    case = "shell_16_12_8"
    dist, coords, basis, f = _setup(d3, gold, case)
    b, u = f["b"], f["u"]
    with pytest.raises(NotImplementedError, match="reduc"):
        b(theta=0.7)(r=1.0).evaluate()
    with pytest.raises(NotImplementedError, match="reduc"):
        b(r=1.0)(theta=0.7).evaluate()
    with pytest.raises(NotImplementedError, match="reduc"):
        b(phi=0.3)(theta=0.7).evaluate()
    with pytest.raises(NotImplementedError, match="reduc"):
        d3.ave(b(theta=0.7), "phi")
    with pytest.raises(NotImplementedError, match="shell average of a tensor"):
        d3.ave(u, coords.S2coordsys)
    with pytest.raises(NotImplementedError, match="output task"):
        (2 * b(theta=0.7)).evaluate()
    with pytest.raises(NotImplementedError, match="coefficient data"):
        b(theta=0.7).evaluate()["c"]
    # the sphere
    dist2, c2, sb, f2 = _setup(d3, gold, "sphere_16_8")
    with pytest.raises(NotImplementedError, match="reduc"):
        f2["h"](phi=0.3)(theta=0.7)
    with pytest.raises(NotImplementedError, match="reduc"):
        d3.ave(f2["h"](theta=0.7), "phi")


def test_reductions_are_refused_in_equations(d3, gold):
    case = "shell_16_12_8"
    dist, coords, basis, f = _setup(d3, gold, case)
    b = f["b"]
    for expr, what in ((b(theta=0.7), "colatitude interpolation"), (b(phi=0.7), "azimuthal interpolation"),
                       (d3.ave(b, "phi"), "zonal mean"), (d3.ave(b, coords.S2coordsys), "shell average")):
        problem = d3.IVP([b], namespace={})
        with pytest.raises(ValueError, match=what):
            problem.add_equation((d3.dt(b) + expr, 0))


def test_sharded_runs_refuse_all_but_the_meridional_slice_by_name(d3, gold):
    """on several ranks the colatitude slice, the zonal mean and the shell average contract while m is distributed:
    refused when evaluated (the meridional slice contracts after the exchange, where all m are local)"""
    import types
    case = "shell_16_12_8"
    dist, coords, basis, f = _setup(d3, gold, case)
    b = f["b"]
    exprs = (b(theta=0.7), d3.ave(b, "phi"), d3.ave(b, coords.S2coordsys))
    outs = [e.evaluate() for e in exprs]
    for o in outs:
        o.dist = types.SimpleNamespace(size=2)
        with pytest.raises(NotImplementedError, match="several ranks"):
            o["g"]


def test_file_handler_writes_constant_axes(d3, gold, tmp_path):
    import types
    from dedalus_amd.core.output import DictionaryHandler, FileHandler
    from dedalus_amd.tools import h5lite
    for case, consts in (("shell_16_12_8", dict(b_theta=[False, True, False], b_phi=[True, False, False],
                                                ave_phi_u=[True, False, False], ave_S2_b=[True, True, False])),
                         ("sphere_16_8", dict(h_theta=[False, True], v_phi=[True, False], ave_phi_v=[True, False]))):
        dist, coords, basis, f = _setup(d3, gold, case)
        tasks = cc.tasks(d3, case, coords, f)
        solver = types.SimpleNamespace(dist=dist, problem=None)
        fh = FileHandler(str(tmp_path / case), solver, iter=1)
        dh = DictionaryHandler(solver, iter=1)
        for name, expr in tasks.items():
            fh.add_task(expr, layout="g", scales=cc.DEALIAS, name=name)
            dh.add_task(expr, layout="g", scales=cc.DEALIAS, name=name)
        for it in range(2):
            fh.evaluate()
            fh.process(iteration=it, wall_time=0.0, sim_time=0.1 * it, timestep=0.1)
        fh.close()
        dh.evaluate()
        dh.process(iteration=0, wall_time=0.0, sim_time=0.0, timestep=0.1)
        r = h5lite.read(str(tmp_path / case / (case + "_s1.h5")))
        assert r.attrs["writes"] == 2
        for name in tasks:
            ref = gold["%s/%s/g15" % (case, name)]
            d = r["tasks/" + name]
            for write in range(2):
                got = d.read(write)
                assert got.shape == ref.shape and np.abs(got - ref).max() <= TOL * np.abs(ref).max(), (case, name)
            got = np.asarray(dh[name]["g"])
            assert got.shape == ref.shape and np.abs(got - ref).max() <= TOL * np.abs(ref).max(), (case, name)
            if name in consts:
                assert list(d.attrs["constant"]) == consts[name], (name, d.attrs["constant"])
                labels = d.attrs["DIMENSION_LABELS"][-len(consts[name]):]
                assert [lab == "constant" for lab in labels] == consts[name]
