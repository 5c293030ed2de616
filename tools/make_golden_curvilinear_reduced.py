"""Golden data of the reduced analysis tasks of sphere and shell fields: runs the unmodified reference on the CPU
(oracle.refshim; the spin recombination needs oracle/_ref from `python oracle/build_ref.py`) over the cases of
tests/curvilinear_reduced_cases.py and writes tests/golden/curvilinear_reduced.npz.

    python tools/make_golden_curvilinear_reduced.py

Per case: the input coefficient arrays (`<case>/in/<field>`, float32 values so the file stays small -- the tests load
exactly these numbers) and, per task, the reference's result as 'g' at scales 1 and 3/2 (`<case>/<task>/{g1, g15}`; the
interpolations exist at the dealias scales only: the reference locks them there)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import refshim  # noqa: E402
import curvilinear_reduced_cases as cc  # noqa: E402


def random_input(field, seed, mean):
    """Random coefficients in every valid (m, ell) mode (projected through one grid round trip, which drops the invalid
    ones) plus a mean, so the ell = 0 part is not small; rounded to float32."""
    field.fill_random("c", seed=seed, distribution="standard_normal")
    field.change_scales(1)
    g = np.array(field["g"])
    if not field.tensorsig:
        g = g + mean
    field["g"] = g
    c32 = np.array(field["c"]).astype(np.float32)
    field["c"] = c32.astype(np.float64)
    return c32


def main():
    d3 = refshim.load_reference()
    out = {}
    for ci, case in enumerate(cc.CASES):
        dist, coords, basis, f = cc.build(d3, case)
        for k in cc.input_names(case):
            out["%s/in/%s" % (case, k)] = random_input(f[k], seed=100 * ci + ord(k), mean=1.5)
        for name, expr in cc.tasks(d3, case, coords, f).items():
            # every task starts from the coefficients as stored: the reference evaluates in place (layouts and scales of
            # b and u are whatever the previous task left), and a cubic product formed after that is not the product of
            # the stored fields any more
            for k in cc.input_names(case):
                f[k].change_scales(1)
                f[k]["c"] = out["%s/in/%s" % (case, k)].astype(np.float64)
            rec = cc.record(expr.evaluate())
            assert "g15" in rec, (case, name)
            for key, arr in rec.items():
                out["%s/%s/%s" % (case, name, key)] = arr
            print(case, name, {k: v.shape for k, v in rec.items()})
    path = os.path.join(ROOT, "tests", "golden", "curvilinear_reduced.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
