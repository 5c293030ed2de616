"""Golden end state of the under-dealiased fused stage: runs the unmodified reference on the CPU (oracle.refshim) over the
Rayleigh-Benard box of tests/fused_stage_cases.py (8 x 128 x 8 modes, dealias = 1: the y axis has 128 modes on 128 points)
and writes tests/golden/fused_dealias1.npz (data only).

    python tools/make_golden_fused_dealias1.py

`<variable>`: coefficient end states after E2E_STEPS RK222 steps of E2E_DT.  Asserted before anything is written: every
dynamical field moved by more than 1e-3 of its norm, and the y spectrum of the end state is broad (the upper third of the
wavenumbers, whose products alias on 128 points, holds more than 1e-3 of the velocity)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from oracle import refshim  # noqa: E402
import fused_stage_cases as fc  # noqa: E402


def main():
    d3 = refshim.load_reference()
    try:
        import numexpr
        numexpr.evaluate("a + 1", local_dict=dict(a=np.zeros(1)))
    except Exception:
        from make_golden_shell_vector_ops import numexpr_stand_in
        numexpr_stand_in()
    solver, start, end = fc.run_dealias1(d3)
    for k in ("b", "u", "p"):
        d = np.linalg.norm(end[k] - start[k])
        assert d > 1e-3 * np.linalg.norm(end[k]), (k, d)
    u = end["u"]
    assert u.shape[-3:] == fc.E2E_SHAPE
    high = np.linalg.norm(u[..., 2 * (fc.E2E_SHAPE[1] // 3):, :])
    assert high > 1e-3 * np.linalg.norm(u), high / np.linalg.norm(u)
    for k, v in end.items():
        print(k, v.shape, float(np.abs(v).max()))
    path = os.path.join(ROOT, "tests", "golden", fc.E2E_GOLDEN)
    np.savez_compressed(path, **end)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1000000


if __name__ == "__main__":
    main()
