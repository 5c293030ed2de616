"""Timing of ddh_grid_map and ddh_grid_broadcast at the dealiased grid of the 3-D Rayleigh-Benard benchmark
(512 x 512 x 256 modes -> 768 x 768 x 384 points), beside a one-term ddh_lincomb of the same size (the copy the project
quotes at 6.29 TB/s), and of flow.max('Re') with Re = sqrt(u@u) / nu as the examples register it.

    python tools/grid_map_bench.py [--out profiles/grid_map.txt] [--parent-tree DIR]

Kernel times are HIP-event times over `--reps` back-to-back launches after a warm-up, median of `--rounds` rounds; GB/s
from the algorithmic bytes (maps and the copy: one read and one write of the grid; broadcast: one write).  flow.max('Re')
is wall-clock with a device synchronisation on both sides, median of 3 after one warm-up, fields at the same size.
--parent-tree: a checkout of the parent commit with its library built; the same flow.max('Re') is timed there in a
child process (`--re-only --root DIR`) and recorded beside this commit's."""
import argparse
import json
import os
import subprocess
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COPY_RATE = 6.29e12


def event_time(torch, launch, reps, rounds):
    for _ in range(3):
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
    return float(np.median(ms)) * 1e-3


def kernel_lines(shape, reps, rounds):
    from dedalus_amd.executor import HipExecutor
    ex = HipExecutor()
    torch = ex.torch
    n = int(np.prod(shape))
    x = torch.rand(n, dtype=torch.float64, device=ex.dev.tdev) + 0.5          # positive: inside every domain used here
    out = torch.empty_like(x)
    lines = []
    t_copy = event_time(torch, lambda: ex.lincomb(out, [x], [1.0]), reps, rounds)
    fmt = "%-28s %9.1f us  %8.1f GB/s  %6.1f %% of the lincomb line"
    lines.append(fmt % ("ddh_lincomb, one term", t_copy * 1e6, 16.0 * n / t_copy / 1e9, 100.0)
                 + "  (%.1f %% of the copy rate on record)" % (100 * 16.0 * n / t_copy / COPY_RATE))
    for op in ("sqrt", "recip", "sin"):
        t = event_time(torch, lambda: ex.grid_map(out, x, op), reps, rounds)
        lines.append(fmt % ("ddh_grid_map " + op, t * 1e6, 16.0 * n / t / 1e9, 100.0 * t_copy / t))
    prof = torch.rand(shape[2], dtype=torch.float64, device=ex.dev.tdev)
    t = event_time(torch, lambda: ex.grid_broadcast(out, prof, 1, shape, (False, False, True)), reps, rounds)
    lines.append("%-28s %9.1f us  %8.1f GB/s  (8 bytes written per point; the copy above moves 16)"
                 % ("ddh_grid_broadcast, z profile", t * 1e6, 8.0 * n / t / 1e9))
    return lines, torch.cuda.get_device_name(0)


def re_seconds(size):
    """wall time of one flow.max('Re'), Re = sqrt(u@u) / nu, for a velocity on RealFourier^2 x Chebyshev of `size` modes"""
    import dedalus_amd.public as d3
    Nx, Ny, Nz = size
    coords = d3.CartesianCoordinates('x', 'y', 'z')
    dist = d3.Distributor(coords, dtype=np.float64)
    B = (d3.RealFourier(coords['x'], size=Nx, bounds=(0, 4), dealias=3 / 2),
         d3.RealFourier(coords['y'], size=Ny, bounds=(0, 4), dealias=3 / 2),
         d3.ChebyshevT(coords['z'], size=Nz, bounds=(0, 1), dealias=3 / 2))
    u = dist.VectorField(coords, name='u', bases=B)
    u.fill_random('c', seed=1, distribution='normal', scale=1e-3)
    u.require_coeff_space()
    nu = 1e-3
    solver = types.SimpleNamespace(ex=dist.executor, dist=dist, iteration=0)
    flow = d3.GlobalFlowProperty(solver, cadence=1)
    flow.add_property(np.sqrt(u @ u) / nu, name='Re')
    ts, val = [], None
    for i in range(4):
        solver.iteration = i                    # (the property is cached per iteration)
        dist.executor.sync()
        t0 = time.perf_counter()
        val = flow.max('Re')
        dist.executor.sync()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts[1:])), float(val)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grid_map.txt"))
    ap.add_argument("--size", default="512,512,256")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--re-only", action="store_true", help="print the flow.max('Re') timing as one JSON line and exit")
    ap.add_argument("--root", default=ROOT, help="the tree to import dedalus_amd from")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    size = tuple(int(v) for v in args.size.split(","))
    if args.re_only:
        t, val = re_seconds(size)
        print(json.dumps(dict(re_seconds=t, re_max=val)))
        return
    shape = tuple(3 * s // 2 for s in size)
    lines, device = kernel_lines(shape, args.reps, args.rounds)
    head = ["pointwise map / broadcast kernels at %d x %d x %d grid points (%.2f GB per array), %s"
            % (shape + (8e-9 * np.prod(shape), device)),
            "HIP-event time per launch; device copy rate on record: %.2f TB/s" % (COPY_RATE / 1e12), ""]
    t_here, val_here = re_seconds(size)
    lines += ["", "flow.max('Re'), Re = sqrt(u@u) / nu at %d x %d x %d modes (wall clock, median of 3):" % size,
              "  this commit (ddh_grid_map on the device):    %10.2f ms   max = %.17g" % (t_here * 1e3, val_here)]
    if args.parent_tree:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--re-only", "--size", args.size, "--root",
                            os.path.abspath(args.parent_tree)], capture_output=True, text=True, cwd=args.parent_tree)
        if r.returncode != 0:
            raise RuntimeError("parent tree run failed:\n" + r.stderr[-3000:])
        p = json.loads(r.stdout.strip().splitlines()[-1])
        lines += ["  parent commit (grid through the host, NumPy): %10.2f ms   max = %.17g" % (p["re_seconds"] * 1e3, p["re_max"]),
                  "  ratio: %.1f x" % (p["re_seconds"] / t_here)]
    text = "\n".join(head + lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
