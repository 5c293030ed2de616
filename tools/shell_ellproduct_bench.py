"""Time of one SphericalEllProduct evaluation on the device beside the transpose of tools/shell_mix_bench.py.

    python tools/shell_ellproduct_bench.py [Nphi Ntheta Nr]

Prints microseconds per call (wall clock around `reps` queued calls and one synchronisation, after a warm-up) of ddh_ell_mix_apply for the ell product of a
vector and of a rank-2 tensor and for trans(T), with the bytes each call reads and writes once (the formula of
profiles/shell_tensor_ops.txt)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    import dedalus_amd.public as d3
    shape = tuple(int(a) for a in sys.argv[1:4]) if len(sys.argv) >= 4 else (256, 128, 128)
    coords = d3.SphericalCoordinates("phi", "theta", "r")
    dist = d3.Distributor(coords, dtype=np.float64)
    shell = d3.ShellBasis(coords, shape=shape, radii=(0.7, 1.9), dealias=3 / 2, dtype=np.float64)
    u = dist.VectorField(coords, name="u", bases=shell)
    T = dist.TensorField(coords, name="T", bases=shell)
    ex = dist.executor
    sb = shell.sphere
    rng = np.random.default_rng(0)
    cases = [("SphericalEllProduct(u)", d3.SphericalEllProduct(u, coords, lambda l: l + 1), u),
             ("SphericalEllProduct(T)", d3.SphericalEllProduct(T, coords, lambda l: l + 1), T),
             ("trans(T)", d3.trans(T), T)]
    print("shape %s, device %s" % (shape, torch.cuda.get_device_name(0)))
    for name, node, arg in cases:
        x = ex.from_host(rng.standard_normal((arg.ncomp, 2 * sb.nml, sb.nl, shell.Nr)))
        terms, slot_map = node._slot_mix()
        dev = ex.make_ell_mix(sb.nml, sb.nl, shell.Nr, node.ncomp, arg.ncomp, terms, slot_map)
        y = ex.empty((node.ncomp, 2 * sb.nml, sb.nl, shell.Nr))
        for _ in range(20):
            dev.apply(x, y)
        ex.sync()
        reps = 200
        t0 = time.perf_counter()
        for _ in range(reps):
            dev.apply(x, y)
        ex.sync()
        us = (time.perf_counter() - t0) * 1e6 / reps
        # the input lines are read on the slots with a mode, the output lines written on all slots (+0 where there is none)
        live = int((np.asarray(slot_map) >= 0).sum())
        nbytes = 8 * shell.Nr * (arg.ncomp * live + node.ncomp * slot_map.size)
        print("%-24s %8.1f us per call, %6.1f MB moved once, %5.2f TB/s, %d terms" % (name, us, nbytes / 1e6, nbytes / us / 1e6, len(terms)))


if __name__ == "__main__":
    main()
