"""Time the rank-2 transpose of a shell tensor through ddh_ell_mix_apply, through the only path that existed before it
(ddh_ell_terms_apply with the scalars as q[ell] * identity matrices), and a one-term ddh_lincomb over the same bytes.

    python tools/shell_mix_bench.py [--shape 256 128 128] [--reps 20] [--out profiles/shell_tensor_ops.txt]

Bytes by formula, not by counter: 8 bytes per coefficient, 9 input components read once on the (m, part, ell) slots that
carry a mode and 9 output components written once on all slots (slots without a mode receive +0); the lincomb reads and
writes all slots of 9 components."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from shell_vector_bench import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=(256, 128, 128))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import dedalus_amd.public as d3
    import shell_tensor_cases as st
    shape = tuple(a.shape)
    coords, dist, shell, u = st.build(d3, shape)
    ex = dist.executor
    u.fill_random("c", seed=1, distribution="standard_normal")
    sb = shell.sphere
    node = d3.trans(d3.grad(u))
    x = node.arg.eval_c()
    terms, slot_map = node._slot_mix()
    nq = len(terms[0][2])
    mix = ex.make_ell_mix(sb.nml, sb.nl, shell.Nr, 9, 9, terms, slot_map)
    eye = np.eye(shell.Nr)
    mats = ex.make_ell_terms(sb.nml, sb.nl, shell.Nr, 9, [(co, ci, q[:, None, None] * eye) for (co, ci, q) in terms], slot_map)
    y = ex.empty(tuple(x.shape))
    y2 = ex.empty(tuple(x.shape))
    mix.apply(x, y)
    mats.apply(x, y2)
    ex.sync()
    ya, yb = np.array(ex.download(y)), np.array(ex.download(y2))
    diff = float(np.abs(ya - yb).max() / np.abs(ya).max())
    live, slots = int(np.count_nonzero(slot_map >= 0)), int(slot_map.size)
    line = 8.0 * shell.Nr
    cases = (("ddh_ell_mix_apply", lambda: mix.apply(x, y), line * 9 * (live + slots)),
             ("ddh_ell_terms_apply", lambda: mats.apply(x, y2), line * 9 * (live + slots) + 8.0 * len(terms) * nq * shell.Nr ** 2),
             ("ddh_lincomb, 1 term", lambda: ex.lincomb(y2, [x], [2.0]), line * 9 * 2 * slots))
    lines = ["trans of a rank-2 tensor, %d terms, %d of %d slots with a mode; mix and matrix path differ by %.1e (relative, max)"
             % (len(terms), live, slots, diff)]
    for name, fn, nbytes in cases:
        med, best, batch = timed(ex, fn, a.reps)
        lines.append("%-20s %9.1f us median %9.1f us best   %8.2f MB by formula   %7.1f GB/s (median)   back to back: %7.1f us, %7.1f GB/s"
                     % (name, med * 1e6, best * 1e6, nbytes / 1e6, nbytes / med / 1e9, batch * 1e6, nbytes / batch / 1e9))
    text = "# tools/shell_mix_bench.py --shape %d %d %d --reps %d\n" % (shape + (a.reps,)) + "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
