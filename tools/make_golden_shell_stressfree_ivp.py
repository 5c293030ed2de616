"""Golden data of the shell problems with stress-free walls (tests/shell_tensor_cases.py::stressfree_lbvp and
stressfree_convection): runs the unmodified reference on the CPU (oracle.refshim) and writes
tests/golden/shell_stressfree_ivp.npz.

    python tools/make_golden_shell_stressfree_ivp.py

`lbvp/in_f` (float32 values), `lbvp/<variable>`: right-hand side and solution of the LBVP; `<timestepper>/<variable>`: the
end state of the convection run after IVP_STEPS fixed steps."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import refshim  # noqa: E402
import shell_tensor_cases as st  # noqa: E402
from make_golden_shell_vector_ops import random_input, numexpr_stand_in  # noqa: E402


def main():
    d3 = refshim.load_reference()
    try:
        import numexpr
        numexpr.evaluate("a + 1", local_dict=dict(a=np.zeros(1)))
    except Exception:
        numexpr_stand_in()
    out = {}
    solver, f = st.stressfree_lbvp(d3)
    out["lbvp/in_f"] = random_input(f["f"], 5)
    solver.solve()
    for k in ("u", "tau_u1", "tau_u2"):
        f[k].change_scales(1)
        out["lbvp/" + k] = np.array(f[k]["c"])
    for ts in ("RK222", "SBDF2"):
        solver, res = st.run_stressfree_convection(d3, ts)[:2]
        for k, v in res.items():
            out["%s/%s" % (ts, k)] = v
    for k, v in out.items():
        print(k, v.shape, float(np.abs(v).max()))
    path = os.path.join(ROOT, "tests", "golden", "shell_stressfree_ivp.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
