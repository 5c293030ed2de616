"""Golden data of SphericalEllProduct on the shell and of the problems with insulating (potential-field) walls: runs the
unmodified reference on the CPU (oracle.refshim; the spin recombination needs oracle/_ref from `python oracle/build_ref.py`)
over the cases of tests/shell_ellproduct_cases.py and writes tests/golden/shell_ellproduct_ops.npz and
tests/golden/shell_ellproduct_ivp.npz (each well under 1 MB).

    python tools/make_golden_shell_ellproduct.py

Operators, per shape `<shape>/`: the input coefficients `in_s`, `in_v`, `in_t` (float32 values) of a scalar, a vector and a
rank-2 tensor, and the reference's result of every task of shell_ellproduct_cases.op_tasks as coefficients.

Problems (equations as recorded in shell_ellproduct_cases._potential_problem, the same text for both codes):

    -div(grad_A) + grad(phi) + lift(tau_A2) = J                  (LBVP)
    dt(A) - eta*div(grad_A) + grad(phi) + lift(tau_A2) = cross(u0, curl(A))      (IVP)
    trace(grad_A) + tau_phi = 0
    integ(phi) = 0
    radial(grad(A)(r=Ro)) + SphericalEllProduct(A, coords, ellp1)(r=Ro)/Ro = 0
    radial(grad(A)(r=Ri)) + SphericalEllProduct(A, coords, ellm)(r=Ri)/Ri = 0
    grad_A = grad(A) + rvec*lift(tau_A1), ellp1 = l + 1, ellm = - l

`lbvp/in_J`, `lbvp/<variable>`: right-hand side and solution; `ivp/in_A`: the initial potential; `<timestepper>/<variable>`:
the end state after IVP_STEPS fixed steps; `rows/outer`, `rows/inner` [nl][3][3 Nr]: the reference's boundary rows per ell
(spin components of the condition x regularity components of A, n fastest), zero where the mode does not exist; `rows/ells`:
the ell that have a subproblem.
Before anything is written the reference's own subproblem matrices are shown to be regular for every ell: L of the LBVP
and M + dt L of the IVP (asserted: condition number below COND_MAX)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import refshim  # noqa: E402
import shell_ellproduct_cases as se  # noqa: E402
from make_golden_shell_vector_ops import random_input, numexpr_stand_in  # noqa: E402

COND_MAX = 1e8


def assert_regular(solver, names, combine, what):
    solver.build_matrices(solver.subproblems, names)
    ells = []
    for sp in solver.subproblems:
        A = combine(*[getattr(sp, n + "_min").toarray() for n in names])
        assert A.shape[0] == A.shape[1], (what, sp.group, A.shape)
        sv = np.linalg.svd(A, compute_uv=False)
        cond = sv[0] / sv[-1]
        print("%s group %s: %d x %d, cond %.3e" % (what, sp.group, A.shape[0], A.shape[1], cond))
        assert np.isfinite(cond) and cond < COND_MAX, (what, sp.group, cond)
        ells.append(sp.group[1])
    return ells


def boundary_rows(d3, solver, f, eq_index, shell):
    """[nl][3][3 Nr]: the rows of one wall condition acting on A, from the reference's expression matrices"""
    eq = solver.problem.equations[eq_index]
    nl, Nr = shell.shape[1], shell.shape[2]
    rows = np.zeros((nl, 3, 3 * Nr))
    for sp in solver.subproblems:
        ell = sp.group[1]
        m = eq["L"].expression_matrices(sp, [f["A"]])[f["A"]].toarray()
        # real dtype: every component carries the (cos, msin) pair of the group's m = 0; the rows do not mix the two parts
        assert m.shape == (6, 6 * Nr) and np.isrealobj(m), (ell, m.shape, m.dtype)
        m = m.reshape(3, 2, 3, 2, Nr)
        assert not np.any(m[:, 0, :, 1]) and not np.any(m[:, 1, :, 0])
        rows[ell] = m[:, 0, :, 0].reshape(3, 3 * Nr)
    return rows


def main():
    d3 = refshim.load_reference()
    try:
        import numexpr
        numexpr.evaluate("a + 1", local_dict=dict(a=np.zeros(1)))
    except Exception:
        numexpr_stand_in()
    ops = {}
    for si, shape in enumerate(se.OP_SHAPES):
        coords, dist, shell, fields = se.build(d3, shape)
        key = se.tag(shape) + "/"
        for j, (k, X) in enumerate(fields.items()):
            ops[key + "in_" + k] = random_input(X, 23 + 10 * si + j)
        for name, expr in se.op_tasks(d3, coords, fields, shape in se.PLAIN_ONLY).items():
            for k, X in fields.items():                       # every task starts from the stored coefficients
                X.change_scales(1)
                X["c"] = ops[key + "in_" + k].astype(np.float64)
            res = expr.evaluate()
            res.change_scales(1)
            ops[key + name] = np.array(res["c"])
            print(key + name, ops[key + name].shape, float(np.abs(ops[key + name]).max()))

    out = {}
    solver, f = se.potential_lbvp(d3)
    ells = assert_regular(solver, ["L"], lambda L: L, "LBVP L")
    assert sorted(ells) == list(range(len(ells))) and len(ells) >= se.SOLVER_SHAPE[1] - 1, ells      # (the last ell may hold no mode)
    out["rows/ells"] = np.array(sorted(ells))
    shell = f["A"].domain.bases[0]
    out["rows/outer"] = boundary_rows(d3, solver, f, 3, shell)
    out["rows/inner"] = boundary_rows(d3, solver, f, 4, shell)
    out["lbvp/in_J"] = random_input(f["J"], 5)
    solver.solve()
    for k in se.VARIABLES:
        out["lbvp/" + k] = se.end_state(f)[k]
    out["ivp/in_A"] = np.array(out["lbvp/A"]).astype(np.float32)      # a potential that meets the walls (to float32)
    for ts in ("RK222", "SBDF2"):
        solver, f = se.potential_induction(d3, ts)
        assert_regular(solver, ["M", "L"], lambda M, L: M + se.IVP_DT * L, "IVP M + dt L")
        solver, f, res = se.run_potential_induction(d3, ts, out["ivp/in_A"])
        for k, v in res.items():
            out["%s/%s" % (ts, k)] = v
    for k, v in out.items():
        print(k, v.shape, float(np.abs(v).max()))
    for fname, d in (("shell_ellproduct_ops.npz", ops), ("shell_ellproduct_ivp.npz", out)):
        path = os.path.join(ROOT, "tests", "golden", fname)
        np.savez_compressed(path, **d)
        print("wrote", path, os.path.getsize(path), "bytes")
        assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
