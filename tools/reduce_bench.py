"""Timing of ddh_axis_contract at the benchmark's shapes (3-D Rayleigh-Benard 512 x 512 x 256, coefficient storage
[kz][kx][ky]) and of the only other way to get such a plane: a full-field 'g' snapshot through a handler.

    python tools/reduce_bench.py [--out profiles/reduced_tasks.txt]

Kernel times are HIP-event times over `--reps` back-to-back launches after a warm-up, median of `--rounds` rounds.  GB/s
from the algorithmic bytes (one read of what the call touches, nw / n of it written) beside the device copy rate the
project records (6.29 TB/s).  The snapshot is wall-clock: evaluate + device-to-host copy + reorder."""
import argparse
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_RATE = 6.29e12


def time_contract(torch, dev, outer, n, inner, nw, N=None, reps=20, rounds=5):
    """N: length of the axis in memory when the call reads its k = 0 slab only (n = 1)."""
    from dedalus_amd import libhip
    from dedalus_amd.device import ptr
    N = n if N is None else N
    x = torch.randn((outer, N, inner), dtype=torch.float64, device=dev.tdev)
    w = torch.randn((nw, n), dtype=torch.float64, device=dev.tdev)
    out = torch.empty((outer, nw, inner), dtype=torch.float64, device=dev.tdev)

    def launch():
        libhip.call("ddh_axis_contract", ptr(x), ptr(out), outer, n, inner, N * inner, ptr(w), nw, dev.stream)
    for _ in range(5):
        launch()
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            launch()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / reps)
    t = float(np.median(ms)) * 1e-3
    nbytes = 8.0 * outer * inner * (n + nw)
    return t, nbytes


def snapshot_seconds(size, rounds=3):
    """One full-field 'g' output of b (scale 1) through a DictionaryHandler, data on the host -> seconds."""
    import dedalus_amd.public as d3
    from dedalus_amd.core.output import DictionaryHandler
    Nx, Ny, Nz = size
    coords = d3.CartesianCoordinates('x', 'y', 'z')
    dist = d3.Distributor(coords, dtype=np.float64)
    B = (d3.RealFourier(coords['x'], size=Nx, bounds=(0, 4), dealias=3 / 2),
         d3.RealFourier(coords['y'], size=Ny, bounds=(0, 4), dealias=3 / 2),
         d3.ChebyshevT(coords['z'], size=Nz, bounds=(0, 1), dealias=3 / 2))
    b = dist.Field(name='b', bases=B)
    b.fill_random('c', seed=1, distribution='normal', scale=1e-3)
    b.require_coeff_space()
    h = DictionaryHandler(types.SimpleNamespace(dist=dist, problem=None), iter=1)
    h.add_task(b, layout='g', name='b')
    plane = DictionaryHandler(types.SimpleNamespace(dist=dist, problem=None), iter=1)
    plane.add_task(b(x=1.0), layout='g', name='plane')
    res = {}
    for name, hd in (("full", h), ("plane", plane)):
        ts = []
        for _ in range(rounds + 1):
            dist.executor.sync()
            t0 = time.perf_counter()
            hd.evaluate()
            hd.process()
            np.asarray(hd[name == "full" and "b" or "plane"]['g'])
            dist.executor.sync()
            ts.append(time.perf_counter() - t0)
        res[name] = float(np.median(ts[1:]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reduced_tasks.txt"))
    ap.add_argument("--size", default="512,512,256")
    ap.add_argument("--no-snapshot", action="store_true")
    args = ap.parse_args()
    Nx, Ny, Nz = (int(v) for v in args.size.split(","))
    from dedalus_amd.device import Device
    dev = Device.get()
    torch = dev.torch
    lines = ["ddh_axis_contract at %d x %d x %d ([kz][kx][ky] coefficient storage), %s" %
             (Nx, Ny, Nz, torch.cuda.get_device_name(0)),
             "bytes = 8 * outer * inner * (n + nw); device copy rate on record: %.2f TB/s" % (COPY_RATE / 1e12), ""]
    shapes = [("x slice            ", Nz, Nx, Ny, None), ("y slice (inner = 1)", Nz * Nx, Ny, 1, None),
              ("mode-0 gather, x   ", Nz, 1, Ny, Nx), ("mode-0 gather, y   ", Nz * Nx, 1, 1, Ny)]
    for label, outer, n, inner, N in shapes:
        for nw in (1, 4):
            t, nb = time_contract(torch, dev, outer, n, inner, nw, N)
            lines.append("%s outer=%-7d n=%-4d inner=%-4d nw=%d  %9.2f us  %8.1f GB/s  (%.1f %% of the copy rate)" %
                         (label, outer, n, inner, nw, t * 1e6, nb / t / 1e9, 100 * nb / t / COPY_RATE))
    if not args.no_snapshot:
        s = snapshot_seconds((Nx, Ny, Nz))
        lines += ["", "one output of the plane b(x=1) at this size, data on the host (wall clock, median of 3):",
                  "  full-field 'g' snapshot of b through a handler (the only way before): %9.2f ms" % (s["full"] * 1e3),
                  "  the reduced task b(x=1) through a handler:                            %9.2f ms" % (s["plane"] * 1e3),
                  "  ratio: %.1f x" % (s["full"] / s["plane"])]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
