"""GPU: M.X written by the backward sweep (solve_backward_kernel<..., EMIT_MX>, ddh_pencil_solve_req::mx_out) against
the parent path, the same solve followed by a DDH_MATVEC_TILED product on the stored solution.

The solution must be bit-identical.  M.X is summed in another order (the band of M P on y instead of M on x = P y), so both
paths are measured against a numpy.longdouble product from the same term list: the sweep's maximum error may be at most
twice the parent's on the same case, or 4 ulp of the row's sum |M_ij x_j|, whichever is larger.  Rows of M without terms
must keep a sentinel.  Each case runs in a process of its own (the sweep switches are read once per process) with the
one-thread-per-(system, block) sweeps forced, so that small problems reach the full-size kernel.

3-D Rayleigh-Benard has n = 5 Nz + 8 band rows in two parity blocks: Nz = 4, 6, 8, 32 give 14, 19, 24 and 84 rows per block
-- below and above the 17-entry window (no Nz of this problem gives exactly 16, 17 or 18).  32 x 32 modes: partner pencils,
16 x 16 cells; 48 x 16: unpaired, 24 x 8 cells (not a multiple of the 64-lane wave).  The kx = ky = 0 pencil is flagged in all.
The 5-step runs use 3-D Rayleigh-Benard 32 x 32 x 128 (the timestepper keeps its M.X and F vectors tile-major only where the
forward z transform writes them so: Chebyshev 192 <- 128 is the smallest such size) and 2-D 64 x 32; they compare end states with the tolerances of tests/test_gpu_ivp.py and count the stand-alone M mat-vecs.
Replaces the reference's sparse M.X products (core/timesteppers.py:588-604)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = {"DDH_PAIR_MIN": "0", "DDH_SWEEP_DEEP": "0", "DDH_X_TILED_MIN": "0", "DDH_RHS_TILING_MIN": "0"}


def _run(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "sweep_emit_mx_worker.py")] + [str(a) for a in args],
                       capture_output=True, text=True, timeout=600, env=dict(os.environ, **ENV), cwd=ROOT)
    assert r.returncode == 0, (args, r.stdout[-1500:], r.stderr[-3000:])
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    print(args, res)
    return res


# (nx, ny, nz, scheme, right-hand-side terms, skip_rows)
CASES = [(32, 32, 4, "RK222", 2, 1), (32, 32, 6, "RK222", 2, 1), (32, 32, 8, "RK222", 4, 0), (48, 16, 8, "RK222", 2, 1),
         (48, 16, 32, "RK443", 4, 1), (32, 32, 32, "RK443", 2, 0)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_sweep_emits_mx_like_the_matvec(case):
    res = _run("kernel", *case)
    assert res["emits"], res
    assert res["nsplit"] == 2 and bool(res["pair"]) == (case[0] == case[1]), res
    assert res["skip_active"] == bool(case[5]), res
    assert res["x_identical"], res
    assert res["finite"] and res["sentinel_kept_new"] and res["sentinel_kept_parent"], res
    assert res["worst_excess"] <= 0.0, res
    assert res["worst_excess_swept"] <= 0.0, res       # (the pencils the sweep computes: without the flagged cell)


@pytest.mark.parametrize("kind,scheme", [("rb3d", "RK222"), ("rb3d", "RK443"), ("rb2d", "RK222"), ("rb2d", "RK443")])
@pytest.mark.parametrize("disturb", [0, 1, 2, 3])
def test_steps_with_emitted_mx_match_the_matvec_path(kind, scheme, disturb):
    res = _run("ivp", kind, scheme, disturb)
    for k, tol in (("p", 1e-10), ("b", 1e-10), ("u", 1e-9)):
        assert res["rel_diff"][k] < tol, res
    assert res["emits"][1] is False
    if kind == "rb3d":
        assert res["emits"][0] is True, res
        # M.X0 is formed by the mat-vec in the first step, in the second (the Hermitian round trip of iteration 0 rewrote
        # the state after the first) and in the step after the state and the timestep changed; nothing else is
        # (disturb 2: a user edit alone, 3: load_state alone -- the timestep and the iteration stay, only the state changed)
        want = [1, 1, 0, 1, 0] if disturb else [1, 1, 0, 0, 0]
        assert res["matvecs_emit"] == want, res
        assert min(res["matvecs_parent"]) >= 2, res
    else:
        # one Fourier axis: the block-inverse / cooperative paths keep the stand-alone mat-vec
        assert res["emits"][0] is False and res["matvecs_emit"] == res["matvecs_parent"], res
