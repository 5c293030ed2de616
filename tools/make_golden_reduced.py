"""Golden data of the reduced analysis tasks: runs the unmodified reference on the CPU (oracle.refshim) over the cases of
tests/reduced_cases.py and writes tests/golden/reduced_tasks.npz.

    python tools/make_golden_reduced.py

Per case: the input coefficient arrays (`<case>/in/<field>`, float32 values so the file stays small -- the tests load
exactly these numbers) and, per task, the reference's result as 'c' at scale 1 and 'g' at scales 1 and 3/2
(`<case>/<task>/{c, g1, g15}`)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import refshim  # noqa: E402
import reduced_cases as rc  # noqa: E402


def smooth_input(dist, bases, field, seed):
    """Grid data with a decaying spectrum plus a little noise in every mode -> valid coefficients, rounded to float32."""
    rng = np.random.default_rng(seed)
    grids = dist.local_grids(*bases)
    shape = np.broadcast(*grids).shape
    ncomp = int(np.prod([cs.dim for cs in field.tensorsig])) if field.tensorsig else 1
    data = np.zeros((ncomp,) + shape)
    for c in range(ncomp):
        acc = 0.3 * (c + 1) + np.zeros(shape)
        for m in range(1, 4):
            term = np.ones(shape)
            for g, b in zip(grids, bases):
                lo, hi = b.bounds
                s = (g - lo) / (hi - lo)
                ph = rng.uniform(0, 2 * np.pi)
                term = term * (np.cos(2 * np.pi * m * s + ph) if isinstance(b, refshim.load_reference().RealFourier)
                               else (1 + 0.5 * m * s * (1 - s) + 0.2 * np.cos(m * s + ph)))
            acc = acc + term / m ** 2
        data[c] = acc + 1e-3 * rng.standard_normal(shape)
    field.change_scales(1)
    field["g"] = data.reshape(field["g"].shape)
    c32 = np.array(field["c"]).astype(np.float32)
    field["c"] = c32.astype(np.float64)
    return c32


def main():
    d3 = refshim.load_reference()
    out = {}
    for ci, case in enumerate(rc.CASES):
        dist, cd, bases, f = rc.build(d3, case)
        B = tuple(bases[n] for n in rc.CASES[case][0])
        for k in ("b", "u"):
            if k in f:
                out["%s/in/%s" % (case, k)] = smooth_input(dist, B, f[k], seed=100 * ci + len(k) + ord(k))
        for name, expr in rc.tasks(d3, case, cd, f).items():
            if isinstance(expr, (int, float)):
                # the reference folds d/dx of a field without x into the number 0 at construction: recorded as zeros of
                # the shape its operand (the slice) has
                assert expr == 0 and name == "dx_of_b_x"
                rec = {k: np.zeros_like(out["%s/b_x_off/%s" % (case, k)]) for k in ("c", "g1", "g15")}
            else:
                rec = rc.record(expr.evaluate())
            for key, arr in rec.items():
                out["%s/%s/%s" % (case, name, key)] = arr
            print(case, name, {k: v.shape for k, v in rec.items()})
    path = os.path.join(ROOT, "tests", "golden", "reduced_tasks.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
