"""Golden dt sequences of the adaptive runs of tests/cfl_terms_cases.py (several CFL velocities, scalar frequencies, a
velocity component without a basis, the three geometries): runs the unmodified reference on the CPU (oracle.refshim) and
writes tests/golden/cfl_terms.npz, one array `<case>` of timesteps per case (data only, a few kB).

    python tools/make_golden_cfl_terms.py

Asserted before anything is written: every sequence is finite, and leaves the start-up ramp of max_change (at least
one timestep is set by the CFL frequency or by the cap of the case, not by 1.5 x the previous one)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from oracle import refshim  # noqa: E402
import cfl_terms_cases as tc  # noqa: E402


def main():
    d3 = refshim.load_reference()
    try:
        import numexpr
        numexpr.evaluate("a + 1", local_dict=dict(a=np.zeros(1)))
    except Exception:
        from make_golden_shell_vector_ops import numexpr_stand_in
        numexpr_stand_in()
    out = {}
    for name, case in tc.CASES.items():
        solver, dts = case(d3)
        assert np.isfinite(dts).all() and (dts > 0).all(), (name, dts)
        ratio = dts[1:] / dts[:-1]
        assert np.any((ratio != 1.0) & (np.abs(ratio - 1.5) > 1e-9)) or name == "rb_profile_capped", (name, dts)
        print(name, " ".join("%.17g" % v for v in dts))
        out[name] = dts
    path = os.path.join(ROOT, "tests", "golden", "cfl_terms.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 100000


if __name__ == "__main__":
    main()
