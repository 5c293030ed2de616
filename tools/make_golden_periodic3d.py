"""Golden data of the triply periodic problems: runs the unmodified reference on the CPU (oracle.refshim) over the
problems of tests/periodic3d_cases.py and writes tests/golden/periodic3d.npz (data only, well under 1 MB).

    python tools/make_golden_periodic3d.py

`tg/<nx>x<ny>x<nz>/<timestepper>/<variable>`, `boussinesq/<timestepper>/<variable>`: coefficient end states after STEPS
fixed steps; `cfl/dts`, `cfl/<variable>`: the adaptive run; `lbvp/<variable>`: the periodic Poisson solution;
`mat/<gx>_<gy>/M`, `.../L`: the reference's matrices of one (kx, ky) group of Taylor-Green (12, 20, 8), rows = the
equations in problem order, columns = the variables in problem order, each field's slots [component][x part][y part]
[z mode] in C order (cos, msin); fields without bases are left out except in the group (0, 0).
Asserted before anything is written: cond(M + dt L) < 1e8 (LBVP: cond(L)) for every subproblem of the reference, and every
end state differs from its initial state by more than 1e-3 of its maximum."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from oracle import refshim  # noqa: E402
import periodic3d_cases as pc  # noqa: E402

COND_MAX = 1e8


def assert_regular(solver, names, combine, what):
    solver.build_matrices(solver.subproblems, names)
    worst = 0.0
    for sp in solver.subproblems:
        A = combine(*[getattr(sp, n + "_min").toarray() for n in names])
        assert A.shape[0] == A.shape[1], (what, sp.group, A.shape)
        if A.shape[0] == 0:
            continue
        sv = np.linalg.svd(A, compute_uv=False)
        cond = sv[0] / sv[-1]
        assert np.isfinite(cond) and cond < COND_MAX, (what, sp.group, cond)
        worst = max(worst, cond)
    print("%s: %d subproblems, worst cond %.3e" % (what, len(solver.subproblems), worst))


def assert_moved(what, start, end):
    for k in end:
        if k.startswith("tau"):
            continue
        d = np.abs(end[k] - start[k]).max()
        assert d > 1e-3 * np.abs(end[k]).max(), (what, k, d)


def group_matrices(solver, fields):
    out = {}
    variables = solver.problem.variables
    for sp in solver.subproblems:
        g = tuple(int(x) for x in sp.group[:2])             # (the reference keeps its last axis coupled: pencils in z)
        if g not in pc.MATRIX_GROUPS:
            continue
        keep_v = [v for v in variables if v.domain.bases or g == (0, 0)]
        for name in ("M", "L"):
            rows = []
            for eq in solver.problem.equations:
                if not (eq["domain"].bases or g == (0, 0)):
                    continue
                mats = eq[name].expression_matrices(sp, variables) if eq[name] != 0 else {}
                n_eq = sp.field_size(eq["LHS"])
                blocks = []
                for v in keep_v:
                    n_v = sp.field_size(v)
                    m = mats.get(v)
                    blocks.append(np.zeros((n_eq, n_v)) if m is None else np.asarray(m.toarray()).reshape(n_eq, n_v))
                rows.append(np.concatenate(blocks, axis=1))
            out["mat/%d_%d/%s" % (g + (name,))] = np.concatenate(rows, axis=0)
    assert len(out) == 2 * len(pc.MATRIX_GROUPS), sorted(out)
    return out


def main():
    d3 = refshim.load_reference()
    try:
        import numexpr
        numexpr.evaluate("a + 1", local_dict=dict(a=np.zeros(1)))
    except Exception:
        from make_golden_shell_vector_ops import numexpr_stand_in
        numexpr_stand_in()
    out = {}
    for shape in pc.TG_SHAPES:
        for ts in pc.TG_STEPPERS:
            solver, start, end = pc.run_ivp(d3, pc.taylor_green, shape=shape, timestepper=ts)
            if ts == "RK222":
                assert_regular(solver, ["M", "L"], lambda M, L: M + pc.DT * L, "TG %s M + dt L" % (shape,))
                if shape == (12, 20, 8):
                    out.update(group_matrices(solver, None))
            assert_moved("TG %s %s" % (shape, ts), start, end)
            for k, v in end.items():
                out["tg/%dx%dx%d/%s/%s" % (shape + (ts, k))] = v
    for ts in pc.BOUSSINESQ_STEPPERS:
        solver, start, end = pc.run_ivp(d3, pc.boussinesq, timestepper=ts)
        if ts == "RK222":
            assert_regular(solver, ["M", "L"], lambda M, L: M + pc.DT * L, "Boussinesq M + dt L")
        assert_moved("Boussinesq %s" % ts, start, end)
        for k, v in end.items():
            out["boussinesq/%s/%s" % (ts, k)] = v
    solver, dts, end = pc.run_cfl(d3)
    assert len(set(np.round(dts, 12))) > 2, dts
    out["cfl/dts"] = dts
    for k, v in end.items():
        out["cfl/" + k] = v
    solver, f = pc.poisson(d3)
    assert_regular(solver, ["L"], lambda L: L, "LBVP L")
    solver.solve()
    for k in ("phi", "tau"):
        out["lbvp/" + k] = np.array(f[k]['c'])
    assert np.abs(out["lbvp/phi"]).max() > 1e-3
    for k, v in out.items():
        print(k, v.shape, float(np.abs(v).max()))
    path = os.path.join(ROOT, "tests", "golden", "periodic3d.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1000000


if __name__ == "__main__":
    main()
