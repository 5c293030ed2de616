"""Timing of the reduced analysis tasks of shell and sphere fields, and of ddh_axis_contract_rows at their shapes.

    python tools/curvilinear_reduce_bench.py [--out profiles/curvilinear_reduced.txt] [--shell 256,128,128] [--sphere 512,256]

Task times are wall clock from evaluate() to host data at the dealias scales (3/2), median of `--rounds` after one warm-up
(plans, weight rows and transform matrices are built by then).  For f(phi=...) the path this replaces is timed beside
it in the same process: the full dealiased grid to the host and np.fft.rfft there.  Kernel times are HIP-event times over
back-to-back launches; GB/s from the bytes actually read (entries from kmin on, the weights once per line) and written,
beside the device copy rate the project records (6.29 TB/s)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_RATE = 6.29e12


def wall(fn, sync, rounds):
    ts = []
    for _ in range(rounds + 1):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts[1:]))


def host_phi(field, position, scales):
    """the azimuthal interpolation as it was done before: whole grid to the host, trigonometric interpolant there"""
    field.change_scales(scales)
    g = np.asarray(field["g"])
    ax = field.rank
    Np = g.shape[ax]
    c = np.fft.rfft(g, axis=ax) / Np
    k = np.arange(c.shape[ax])
    w = np.where((k == 0) | ((Np % 2 == 0) & (k == Np // 2)), 1.0, 2.0) * np.exp(1j * k * position)
    shape = [1] * g.ndim
    shape[ax] = k.size
    return np.sum((c * w.reshape(shape)).real, axis=ax, keepdims=True)


def task_times(d3, kind, shape, rounds):
    rng = np.random.default_rng(1)
    if kind == "shell":
        coords = d3.SphericalCoordinates("phi", "theta", "r")
        dist = d3.Distributor(coords, dtype=np.float64)
        basis = d3.ShellBasis(coords, shape=shape, radii=(1, 2), dealias=3 / 2, dtype=np.float64)
        s, v = dist.Field(name="b", bases=basis), dist.VectorField(coords, name="u", bases=basis)
    else:
        coords = d3.S2Coordinates("phi", "theta")
        dist = d3.Distributor(coords, dtype=np.float64)
        basis = d3.SphereBasis(coords, shape, radius=1, dealias=3 / 2, dtype=np.float64)
        s, v = dist.Field(name="h", bases=basis), dist.VectorField(coords, name="v", bases=basis)
    for f in (s, v):
        f["g"] = rng.standard_normal(f["g"].shape)
        f.require_coeff_space()
    ex = dist.executor
    tasks = [("%s(phi=1)" % s.name, s(phi=1.0)), ("%s(phi=1)" % v.name, v(phi=1.0)),
             ("%s(theta=0.7)" % s.name, s(theta=0.7)), ("%s(theta=0.7)" % v.name, v(theta=0.7)),
             ("ave(%s, phi)" % s.name, d3.Average(s, coords["phi"])), ("ave(%s, phi)" % v.name, d3.Average(v, coords["phi"]))]
    if kind == "shell":
        tasks.append(("ave(b, S2)", d3.Average(s, coords.S2coordsys)))
        tasks.append(("(u*b)(phi=1)", (v * s)(phi=1.0)))
    out = []
    for name, expr in tasks:
        def run(expr=expr):
            o = expr.evaluate()
            o.change_scales(3 / 2)
            return np.asarray(o["g"])
        t = wall(run, ex.sync, rounds)
        out.append((name, run().shape, t))
    host = []
    for f in (s, v):
        c = f.require_coeff_space()

        def run(f=f, c=c):
            f._set_device_coeff(c)                              # (the grid is formed anew, as for a field that stepped)
            return host_phi(f, 1.0, 3 / 2)
        host.append(("%s(phi=1)" % f.name, wall(run, ex.sync, rounds)))
    return out, host


def kernel_times(torch, dev, label, nc, nm, nl, inner, spins, reps=20, rounds=5):
    from dedalus_amd import libhip
    from dedalus_amd.device import ptr
    import ctypes as C
    outer = nc * 2 * nm
    rows, kmins, index = [], [], {}
    for i in range(nc):
        for m in range(nm):
            key = (abs(spins[i]), m)
            if key not in index:
                index[key] = len(kmins)
                kmins.append(min(max(m, abs(spins[i])), nl))
            rows += [index[key]] * 2
    row = torch.as_tensor(np.array(rows, dtype=np.int32), device=dev.tdev)
    kmin = torch.as_tensor(np.array(kmins, dtype=np.int32), device=dev.tdev)
    x = torch.randn((outer, nl, inner), dtype=torch.float64, device=dev.tdev)
    w = torch.randn((len(kmins), nl), dtype=torch.float64, device=dev.tdev)
    out = torch.empty((outer, inner), dtype=torch.float64, device=dev.tdev)

    def launch():
        libhip.call("ddh_axis_contract_rows", ptr(x), ptr(out), outer, nl, inner, ptr(w), C.c_void_p(row.data_ptr()),
                    C.c_void_p(kmin.data_ptr()), len(kmins), dev.stream)
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
    live = sum(nl - kmins[r] for r in rows)
    nbytes = 8.0 * (live * inner + live + outer * inner)
    return "%s outer=%-5d n=%-4d inner=%-4d  %8.2f us  %7.1f GB/s  (%.1f %% of the copy rate; %.0f %% of the array read)" % (
        label, outer, nl, inner, t * 1e6, nbytes / t / 1e9, 100 * nbytes / t / COPY_RATE, 100.0 * live / (outer * nl))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "curvilinear_reduced.txt"))
    ap.add_argument("--shell", default="256,128,128")
    ap.add_argument("--sphere", default="512,256")
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    shell = tuple(int(v) for v in args.shell.split(","))
    sphere = tuple(int(v) for v in args.sphere.split(","))
    import dedalus_amd.public as d3
    from dedalus_amd.device import Device
    dev = Device.get()
    torch = dev.torch
    lines = ["reduced analysis tasks of curvilinear fields, %s" % torch.cuda.get_device_name(0),
             "wall clock from evaluate() to host data at scales 3/2, median of %d" % args.rounds, ""]
    for kind, shape in (("shell", shell), ("sphere", sphere)):
        tasks, host = task_times(d3, kind, shape, args.rounds)
        lines.append("%sBasis%s, dealias 3/2" % ("Shell" if kind == "shell" else "Sphere", shape))
        for name, shp, t in tasks:
            lines.append("  %-16s -> %-20s %9.3f ms" % (name, shp, t * 1e3))
        for name, t in host:
            new = [x for x in tasks if x[0] == name][0][2]
            lines.append("  %-16s through the host (full grid download + np.fft.rfft%s) %9.3f ms: %.1f x the device path"
                         % (name, ", the path before" if kind == "shell" else "", t * 1e3, t / new))
        lines.append("")
    lines.append("ddh_axis_contract_rows with triangular truncation (kmin = max(m, |s|)); bytes = entries from kmin on + weights + output;")
    lines.append("device copy rate on record: %.2f TB/s; back-to-back launches on one buffer: arrays below the 256 MB last-level" % (COPY_RATE / 1e12))
    lines.append("cache are read from it (the shell shapes), the sphere shapes are launch bound, 'large strided' streams from HBM")
    Ng = int(np.ceil(1.5 * shell[2]))
    lines.append(kernel_times(torch, dev, "shell scalar ", 1, shell[0] // 2, shell[1] - 1, Ng, (0,)))
    lines.append(kernel_times(torch, dev, "shell vector ", 3, shell[0] // 2, shell[1] - 1, Ng, (-1, 1, 0)))
    lines.append(kernel_times(torch, dev, "sphere scalar", 1, sphere[0] // 2, sphere[1] - 1, 1, (0,)))
    lines.append(kernel_times(torch, dev, "sphere vector", 2, sphere[0] // 2, sphere[1] - 1, 1, (-1, 1)))
    lines.append(kernel_times(torch, dev, "large strided", 3, 256, 255, 384, (-1, 1, 0)))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
