"""Time curl(u), grad(u) and cross(ez, u) of a shell vector field through the same entry point (operand.eval_c()), and a
step of the shell convection problem with and without the Coriolis force; bytes by formula, not by counter.

    python tools/shell_vector_bench.py [--shape 256 128 128] [--reps 20] [--out profiles/shell_vector_ops.txt]

Bytes counted for the coefficient-space operators: the input and output lines once (8 bytes per coefficient of every
live (m, ell) slot and component) plus the non-zeros of the radial matrices once per ell; the cross product is bound by its
transforms, so its time is given beside a step, not as a rate."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(ex, fn, reps):
    fn()
    ex.sync()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ex.sync()
        ts.append(time.perf_counter() - t0)
    t0 = time.perf_counter()                      # reps calls back to back, one synchronisation: launch latency overlaps
    for _ in range(reps):
        fn()
    ex.sync()
    return float(np.median(ts)), float(np.min(ts)), (time.perf_counter() - t0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=(256, 128, 128))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import dedalus_amd.public as d3
    import shell_vector_cases as sv
    shape = tuple(a.shape)
    coords, dist, shell, u, v = sv.build(d3, shape)
    ex = dist.executor
    u.fill_random("c", seed=1, distribution="standard_normal")
    u.require_coeff_space()
    ez = sv.rotation_axis(d3, coords, dist, shell)
    sb = shell.sphere
    live = sum(2 * min(l + 1, sb.nm) for l in range(sb.nl))              # (m, part) slots with a mode, summed over ell
    lines = []
    for name, op, nci, nco in (("curl(u)", d3.curl(u), 3, 3), ("grad(u)", d3.grad(u), 3, 9)):
        op.eval_c()
        nnz = sum(int(np.count_nonzero(t[2])) for t in op.termlist().terms)
        nbytes = 8.0 * (live * shell.Nr * (nci + nco) + nnz)
        med, best, batch = timed(ex, op.eval_c, a.reps)
        lines.append("%-12s %9.1f us median %9.1f us best   %8.2f MB by formula   %7.1f GB/s (median)   back to back: %7.1f us, %7.1f GB/s"
                     % (name, med * 1e6, best * 1e6, nbytes / 1e6, nbytes / med / 1e9, batch * 1e6, nbytes / batch / 1e9))
    cr = d3.cross(ez, u)
    med, best, batch = timed(ex, cr.eval_c, a.reps)
    lines.append("%-12s %9.1f us median %9.1f us best   back to back: %7.1f us   (two backward transforms, one bilinear kernel, one forward)"
                 % ("cross(ez,u)", med * 1e6, best * 1e6, batch * 1e6))
    for rotate in (False, True):
        solver, f = sv.rotating_convection(d3, shape=shape, rotate=rotate)
        for _ in range(3):
            solver.step(sv.IVP_DT)
        ex.sync()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            solver.step(sv.IVP_DT)
        ex.sync()
        lines.append("step, %-22s %9.2f ms" % ("with Coriolis" if rotate else "without Coriolis", (time.perf_counter() - t0) / a.reps * 1e3))
    text = "# tools/shell_vector_bench.py --shape %d %d %d --reps %d\n" % (shape + (a.reps,)) + "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
