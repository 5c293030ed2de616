"""Golden data of the curl on a shell left-hand side: runs the unmodified reference on the CPU (oracle.refshim; needs
oracle/_ref from `python oracle/build_ref.py`) over the problems of tests/shell_curl_lhs_cases.py and writes
tests/golden/shell_curl_lhs.npz (data only, well under 1 MB).

    python tools/make_golden_shell_curl_lhs.py

`lbvp/in_J`, `lbvp/<variable>`: right-hand side and solution of the Beltrami-like LBVP; `ivp/in_B`: the initial field (the
LBVP's B to float32: it meets the walls); `<timestepper>/<variable>`: the end state of the alpha^2 dynamo after IVP_STEPS
fixed steps; `L/ells`, `L/<ell>` [6 Nr][6 Nr]: the reference's real-form matrix of the IVP's first equation acting on B
(SphericalCurl.subproblem_matrix, real-dtype branch with mult_1j, core/operators.py:3903-3942, among its terms), indices
(component, part, n) with n fastest.
Asserted before anything is written: cond < 1e8 for every ell of the reference's own L (LBVP) and M + dt L (IVP), and on
every stored ell the part-mixing entries (the imaginary part of the complex system) reach 1e-3 of the part-preserving ones,
so that the fixture cannot be met with the imaginary part dropped."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from oracle import refshim  # noqa: E402
import shell_curl_lhs_cases as sc  # noqa: E402
from make_golden_shell_vector_ops import random_input, numexpr_stand_in  # noqa: E402
from make_golden_shell_ellproduct import assert_regular  # noqa: E402


def real_form_L(solver, f, Nr):
    eq = solver.problem.equations[0]
    out = {}
    for sp in solver.subproblems:
        ell = sp.group[1]
        if ell not in sc.MATRIX_ELLS:
            continue
        m = eq["L"].expression_matrices(sp, solver.problem.variables, ncc_cutoff=solver.ncc_cutoff, max_ncc_terms=solver.max_ncc_terms)[f["B"]].toarray()      # (NCC matrices: the variables they were built with)
        assert m.shape == (6 * Nr, 6 * Nr) and np.isrealobj(m), (ell, m.shape, m.dtype)
        m6 = m.reshape(3, 2, Nr, 3, 2, Nr)
        Lr, Li = m6[:, 0, :, :, 0, :], m6[:, 1, :, :, 0, :]
        assert np.array_equal(m6[:, 1, :, :, 1, :], Lr) and np.array_equal(m6[:, 0, :, :, 1, :], -Li)
        ratio = np.abs(Li).max() / np.abs(Lr).max()
        print("L ell %d: max |L_i| / max |L_r| = %.3e" % (ell, ratio))
        assert ratio >= 1e-3, (ell, ratio)
        out[ell] = m
    assert sorted(out) == sorted(sc.MATRIX_ELLS), sorted(out)
    return out


def main():
    d3 = refshim.load_reference()
    try:
        import numexpr
        numexpr.evaluate("a + 1", local_dict=dict(a=np.zeros(1)))
    except Exception:
        numexpr_stand_in()
    out = {}
    solver, f = sc.beltrami_lbvp(d3)
    assert_regular(solver, ["L"], lambda L: L, "LBVP L")
    out["lbvp/in_J"] = random_input(f["J"], 5)
    solver.solve()
    for k in sc.VARIABLES:
        out["lbvp/" + k] = sc.end_state(f)[k]
    out["ivp/in_B"] = np.array(out["lbvp/B"]).astype(np.float32)
    for ts in ("RK222", "SBDF2"):
        solver, f = sc.alpha2_dynamo(d3, ts)
        assert_regular(solver, ["M", "L"], lambda M, L: M + sc.IVP_DT * L, "IVP M + dt L")
        assert_regular(solver, ["L"], lambda L: L, "IVP L")
        if ts == "RK222":
            mats = real_form_L(solver, f, sc.SOLVER_SHAPE[2])
            out["L/ells"] = np.array(sorted(mats))
            for ell, m in mats.items():
                out["L/%d" % ell] = m
        solver, f, res = sc.run_alpha2_dynamo(d3, ts, out["ivp/in_B"])
        for k, v in res.items():
            out["%s/%s" % (ts, k)] = v
    for k, v in out.items():
        print(k, v.shape, float(np.abs(v).max()))
    path = os.path.join(ROOT, "tests", "golden", "shell_curl_lhs.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 65333          # (the size of shell_ellproduct_ivp.npz, the sibling problem fixture)


if __name__ == "__main__":
    main()
