"""Device time of the complex per-ell band LU (a curl on a shell left-hand side) beside the real one, at ShellBasis(256,128,128).

    python tools/shell_curl_lhs_bench.py [NphixNthetaxNr] [--base-lib PATH] [--out profiles/shell_curl_lhs.txt]

One process builds two solvers of the same shape: the shell convection problem of tests/problems.py (real per-ell systems)
and the alpha^2 dynamo of tests/shell_curl_lhs_cases.py (complex ones), and times ddh_ellband_solve (through solver.solve)
and ddh_ellband_factor (through solver.factor on an existing slot) of each with device events: REPEATS windows of a fixed
number of calls after a warm-up, min / median / max of the windows reported (the spread).  The dynamo is timed once more with
dense inverses (DDH_SHELL_DENSE=1), the path the band LU replaces.  Next to every measured time stand the COUNTS of
executor.EllBand (_flops, _bytes) and the expectation they give: per slot 2x the multiply-adds of the LU rows (4x per pair
column), 2x the factor-row bytes, equal right-hand-side and solution bytes.
--base-lib: another build of the library (the parent commit's; DDH_LIB).  The real solve and factor are then timed in fresh
child processes, this build and that one in turn, twice each: their ellband code for real handles is the same, so the times
are expected to agree within the spread of the repeats."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

REPEATS, SOLVES, FACTORS = 7, 20, 5
A0, B0 = 1.0, 0.05 * 2 / 3


def windows(fn, calls):
    import torch
    fn()
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(REPEATS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / calls)
    out.sort()
    return dict(min=out[0], median=out[len(out) // 2], max=out[-1])


def time_solver(s):
    """-> dict(solve, factor: ms windows; plan and counts where the band path is taken)"""
    lu = s.factor(A0, B0)
    s.ex.sync()
    rhs = s.ex.zeros((s.R, s.nx, s.ny))
    rhs.normal_()
    x = s.ex.zeros((s.R, s.nx, s.ny))
    k = [0]

    def refactor():
        k[0] += 1
        s.factor(A0, B0 * (1 + 0.01 * k[0]), reuse=lu)
    res = dict(solve=windows(lambda: s.solve(lu, rhs, x), SOLVES), factor=windows(refactor, FACTORS), band=bool(s._band))
    if s._band:
        pl, dev = s._band["plan"], s._band["dev"]
        res.update(cx=bool(pl.cx), kl=int(pl.kl), ku=int(pl.ku), mp=int(pl.mp), nbc=int(pl.nbc), nmax=int(pl.nmax),
                   banded=len(pl.per), dense_groups=[int(g) for g in pl.dense_groups], info=dev.info(),
                   flops=float(dev._flops), bytes=float(dev._bytes), rows=int(pl.n.sum()), R=int(s.R))
    return res


def real_solver(d3, shape):
    import problems
    return problems.shell_convection(d3, shape=shape)[0]


def dynamo_solver(d3, shape):
    import shell_curl_lhs_cases as sc
    return sc.alpha2_dynamo(d3, "SBDF2", shape=shape)[0]


def fmt(w):
    return "%8.3f ms  (min %.3f, max %.3f of %d windows)" % (w["median"], w["min"], w["max"], REPEATS)


def main():
    args = sys.argv[1:]
    opt = {}
    for key in ("--base-lib", "--out", "--child"):
        if key in args:
            i = args.index(key)
            opt[key] = args[i + 1]
            del args[i:i + 2]
    shape = tuple(int(v) for v in args[0].split("x")) if args else (256, 128, 128)
    import dedalus_amd.public as d3
    if "--child" in opt:                                   # the real problem alone, one JSON line
        print("RESULT " + json.dumps(time_solver(real_solver(d3, shape))))
        return
    lines = []
    say = lambda s="": (lines.append(s), print(s, flush=True))
    say("# tools/shell_curl_lhs_bench.py at ShellBasis(%d,%d,%d); times are MEASURED with device events (median of %d windows of"
        % (shape + (REPEATS,)))
    say("# %d solves / %d factorizations, min and max of the windows = the run-to-run spread); flops and bytes are COUNTS" % (SOLVES, FACTORS))
    say("# (executor.EllBand._flops / _bytes: algorithmic work of one solve), not counter readings.")
    real = time_solver(real_solver(d3, shape))
    cplx = time_solver(dynamo_solver(d3, shape))
    os.environ["DDH_SHELL_DENSE"] = "1"
    dense = time_solver(dynamo_solver(d3, shape))
    del os.environ["DDH_SHELL_DENSE"]
    for name, r in (("real   (shell convection)", real), ("complex (alpha^2 dynamo) ", cplx)):
        say()
        say("%s: %d system components, band LU for %d ell, dense for %s; kl %d ku %d mp %d nbc %d nmax %d, windows nw %d wt %d, cx %s"
            % (name, r["R"], r["banded"], r["dense_groups"], r["kl"], r["ku"], r["mp"], r["nbc"], r["nmax"], r["info"]["nw"],
               r["info"]["wt"], r["cx"]))
        say("  measured  solve  %s" % fmt(r["solve"]))
        say("  measured  factor %s" % fmt(r["factor"]))
        say("  count     solve  %.3f GFLOP, %.1f MB over %d band rows; factor storage %.1f MB"
            % (r["flops"] / 1e9, r["bytes"] / 1e6, r["rows"], r["info"]["factor_bytes"] / 1e6))
        say("  derived   solve  %.1f GFLOP/s, %.1f GB/s of the counted work at the median" % (
            r["flops"] / r["solve"]["median"] / 1e6, r["bytes"] / r["solve"]["median"] / 1e6))
    say()
    say("complex (alpha^2 dynamo), dense inverses (DDH_SHELL_DENSE=1: the path the band LU replaces):")
    say("  measured  solve  %s" % fmt(dense["solve"]))
    say("  measured  factor %s   (device inversion + download of the inverse + a new term list)" % fmt(dense["factor"]))
    say()
    say("expectation from the counts (the two problems differ in size and band, so the ratio is taken per counted unit):")
    say("  per slot column the complex LU rows cost 2x the real multiply-adds (4x per pair column), the real recombination 1x;")
    say("  factor rows 2x the bytes; right-hand side and solution bytes equal.")
    say("  count     flops   complex / real = %.2f      bytes complex / real = %.2f" % (cplx["flops"] / real["flops"], cplx["bytes"] / real["bytes"]))
    say("  measured  solve   complex / real = %.2f      factor complex / real = %.2f" % (
        cplx["solve"]["median"] / real["solve"]["median"], cplx["factor"]["median"] / real["factor"]["median"]))
    say("  measured  solve   band / dense (complex) = %.2f      factor band / dense = %.3f" % (
        cplx["solve"]["median"] / dense["solve"]["median"], cplx["factor"]["median"] / dense["factor"]["median"]))
    if "--base-lib" in opt:
        say()
        say("real solve and factor, this build against the parent commit's library (DDH_LIB), fresh processes in turn (MEASURED):")
        for rnd in (1, 2):
            for name, lib in (("parent", opt["--base-lib"]), ("this  ", None)):
                env = dict(os.environ)
                env.pop("DDH_LIB", None)
                if lib:
                    env["DDH_LIB"] = os.path.abspath(lib)
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "x".join(map(str, shape)), "--child", "1"],
                                   capture_output=True, text=True, env=env, timeout=900)
                got = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
                if r.returncode != 0 or not got:
                    say("  %s run %d failed (exit %d): %s" % (name, rnd, r.returncode, r.stderr[-400:]))
                    return 1
                c = json.loads(got[-1][7:])
                say("  %s run %d  solve %s" % (name, rnd, fmt(c["solve"])))
                say("  %s run %d  factor %s" % (name, rnd, fmt(c["factor"])))
    if "--out" in opt:
        with open(opt["--out"], "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
