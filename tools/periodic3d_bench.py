"""Taylor-Green in a triply periodic box (tests/periodic3d_cases.py) at N^3, RK222: steps/s, the modal solve's time and
achieved GB/s against its algorithmic bytes ((rows read + rows written) * 8 B), the same run on the band LU over the pencil
(DDH_MODAL=0, a fresh process), and the factor memory the modal solve saves.  Writes profiles/periodic3d.txt.

    python tools/periodic3d_bench.py [--n 256] [--steps 10] [--warmup 3]

One run per mode in a child process of its own (the mode is read when the solver is built); every figure is measured."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

COPY_RATE_TBS = 6.29            # the project's measured device copy rate


def child(n, steps, warmup):
    import torch
    import dedalus_amd.public as d3
    import periodic3d_cases as pc
    from dedalus_amd.executor import KernelTimer
    solver, f = pc.taylor_green(d3, (n, n, n), "RK222")
    solver.enable_step_graph(False)
    dt = 1e-3
    for _ in range(warmup):
        solver.step(dt)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        solver.step(dt)
    e1.record()
    torch.cuda.synchronize()
    ms_step = e0.elapsed_time(e1) / steps
    timer = KernelTimer(torch)                      # a second, instrumented pass: HIP events around every kernel family
    solver.ex.timer = timer
    for _ in range(steps):
        solver.step(dt)
    summ = timer.summary()
    solver.ex.timer = None
    # a timestep change: what the next step costs on top of an ordinary one
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    solver.step(0.5 * dt)
    e1.record()
    torch.cuda.synchronize()
    key = "pencil_solve_modal" if solver.modal is not None else "pencil_solve"
    s = summ.get(key, {})
    print("RESULT " + json.dumps(dict(
        modal=solver.modal is not None, n=n, R=solver.R, rc=(solver.modal.plan.rc if solver.modal is not None else None),
        ms_step=ms_step, steps_per_s=1e3 / ms_step, solve_launches_per_step=s.get("launches", 0) / steps,
        solve_ms=s.get("avg_ms"), solve_bytes=s.get("bytes_per_launch"), solve_gbps=s.get("gbps"),
        factor_bytes=solver.factor_bytes(), dt_change_step_ms=e0.elapsed_time(e1),
        u_max=float(abs(f["u"]["g"]).max()),
        families={k: dict(ms_per_step=v["total_ms"] / steps, gbps=v["gbps"]) for k, v in sorted(summ.items())})))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "periodic3d.txt"))
    a = ap.parse_args()
    if a.child:
        return child(a.n, a.steps, a.warmup)
    res = {}
    for mode in ("1", "0"):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--n", str(a.n), "--steps", str(a.steps),
                            "--warmup", str(a.warmup)], capture_output=True, text=True, env=dict(os.environ, DDH_MODAL=mode))
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            raise SystemExit("DDH_MODAL=%s run failed:\n%s" % (mode, r.stderr[-3000:]))
        res[mode] = json.loads(line[-1][7:])
    m, b = res["1"], res["0"]
    lines = ["# tools/periodic3d_bench.py: Taylor-Green, %d^3, RK222, dealias 3/2, %d timed steps (fixed dt, ordinary launches)" % (a.n, a.steps),
             "# modal = matrix-free modal solve (csrc/ddh_modal.hip); band = DDH_MODAL=0, band LU over the Fourier pencil axis",
             "%-34s %14s %14s" % ("", "modal", "band"),
             "%-34s %14.2f %14.2f" % ("steps/s", m["steps_per_s"], b["steps_per_s"]),
             "%-34s %14.3f %14.3f" % ("ms per step", m["ms_step"], b["ms_step"]),
             "%-34s %14.2f %14.2f" % ("solves per step", m["solve_launches_per_step"], b["solve_launches_per_step"]),
             "%-34s %14.3f %14.3f" % ("ms per solve", m["solve_ms"], b["solve_ms"]),
             "%-34s %14.1f %14.1f" % ("solve GB/s (counted bytes)", m["solve_gbps"], b["solve_gbps"]),
             "%-34s %14.1f %14.1f" % ("counted MB per solve", m["solve_bytes"] / 1e6, b["solve_bytes"] / 1e6),
             "%-34s %14.1f %14.1f" % ("factor memory, MB", m["factor_bytes"] / 1e6, b["factor_bytes"] / 1e6),
             "%-34s %14.3f %14.3f" % ("step after a dt change, ms", m["dt_change_step_ms"], b["dt_change_step_ms"]),
             "%-34s %14.6f %14.6f" % ("max |u| after the run", m["u_max"], b["u_max"]),
             "# modal solve: rc = %d component rows, R = %d rows; %.1f %% of the %.2f TB/s copy rate"
             % (m["rc"], m["R"], 100 * m["solve_gbps"] / (1e3 * COPY_RATE_TBS), COPY_RATE_TBS),
             "# factor memory saved: %.1f MB" % ((b["factor_bytes"] - m["factor_bytes"]) / 1e6),
             "# kernel families of the modal run, ms per step (GB/s):"]
    for k, v in m["families"].items():
        lines.append("#   %-28s %9.3f (%8.1f)" % (k, v["ms_per_step"], v["gbps"]))
    text = "\n".join(lines) + "\n"
    print(text)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
