"""Golden data of the rotating shell convection run (case (c) of tests/shell_vector_cases.py): the unmodified reference on
the CPU (oracle.refshim) -> tests/golden/shell_vector_ivp.npz.  Kept apart from shell_vector_ops.npz, which fills most
of the size a committed file may have.

    python tools/make_golden_shell_vector_ivp.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from oracle import refshim  # noqa: E402
import shell_vector_cases as sv  # noqa: E402
from make_golden_shell_vector_ops import numexpr_stand_in  # noqa: E402


def main():
    d3 = refshim.load_reference()
    try:
        import numexpr
        numexpr.evaluate("a + 1", local_dict=dict(a=np.zeros(1)))
    except Exception:
        numexpr_stand_in()
    solver, res = sv.run_rotating_convection(d3)
    out = {"end/" + k: v for k, v in res.items()}
    out["shape"], out["steps"], out["dt"], out["ekman"] = np.array(sv.IVP_SHAPE), sv.IVP_STEPS, sv.IVP_DT, sv.EKMAN
    for k, v in res.items():
        print(k, v.shape, float(np.abs(v).max()))
    path = os.path.join(ROOT, "tests", "golden", "shell_vector_ivp.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
