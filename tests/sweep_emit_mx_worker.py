"""Worker of tests/test_gpu_sweep_emit_mx.py (the sweep switches are read once per process): one case per run.

kernel NX NY NZ SCHEME TERMS SKIP   the solve that emits M.x against the parent path (the same solve, then the mat-vec)
ivp PROBLEM SCHEME DISTURB          5 steps with the emitting sweeps against 5 steps with the stand-alone mat-vecs; before the
                                    fourth step: 0 nothing, 1 a user edit and a new timestep, 2 a user edit alone, 3 load_state
                                    alone (a checkpoint of that very iteration, so only the state's authority changes)
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import problems                                  # noqa: E402
import dedalus_amd.public as d3                  # noqa: E402

SENTINEL = -7.25e77


def _solver(kind, scheme, shape):
    if kind == "rb3d":
        solver, f = problems.rayleigh_benard_3d(d3, Nx=shape[0], Ny=shape[1], Nz=shape[2], timestepper=scheme)
    else:
        solver, f = problems.rayleigh_benard_2d(d3, Nx=shape[0], Nz=shape[1], timestepper=scheme)
    solver.pack.set_solve_variant(0)             # one thread per (system, block): the full-size kernels
    if hasattr(solver, "enable_step_graph"):
        solver.enable_step_graph(False)
    return solver, f


def _natural(solver, vec, state):
    if state:
        if getattr(solver, "x_tiled", 0):
            return np.asarray(solver.untile_rows(vec, banded=bool(getattr(solver, "x_banded", 0))).cpu().numpy())
        return np.asarray(vec.cpu().numpy()).reshape(solver.R, solver.nx, solver.ny)
    return np.asarray(solver.untile_rows(vec).cpu().numpy())


def kernel_case(nx, ny, nz, scheme, nterms, use_skip):
    solver, f = _solver("rb3d", scheme, (nx, ny, nz))
    for _ in range(2):
        solver.step(1e-3)
    ts, s, pack, ex = solver.timestepper, solver, solver.pack, solver.ex
    lu = list(ts._lus.values())[0]
    info = pack.lu_info(lu)
    out = dict(emits=bool(s.prepare_mx_emission(lu)), tiled=int(ts._tiled), pair=info["pair"], nsplit=info["nsplit"],
               rows_per_block=info["rows_per_block"], W=info["W"])
    if not out["emits"]:
        return out
    flagged = len(getattr(s, "_flagged_cells", {}).get(lu, ())) if hasattr(s, "_flagged_cells") else -1
    out["flagged"] = flagged
    pool = [ts.MX0, ts.F[0], ts.F[-1], ts.MX[1] if ts.MX[1] is not None else ts.F[0]]
    xs = [pool[i % len(pool)].clone() for i in range(nterms)]
    al = [1.0, 0.37e-3, -0.21e-3, 0.45][:nterms]
    zrows = s.mx_f_zero_rows()
    skip = s.intermediate_skip_rows() if use_skip else None
    out["skip_active"] = skip is not None
    X0 = s.X.clone()
    Xa, Xb = X0.clone(), X0.clone()
    MXa = ex.zeros((s.R, s.nx, s.ny))
    MXb = ex.zeros((s.R, s.nx, s.ny))
    MXa.fill_(SENTINEL)
    MXb.fill_(SENTINEL)
    s.solve_lincomb(lu, xs, al, Xa, zero_rows=zrows, skip_rows=skip, tiled=True)
    pack.matvec(s.M_id, Xa, MXa, owned=True, tiled=True)
    s.solve_lincomb(lu, xs, al, Xb, zero_rows=zrows, skip_rows=skip, tiled=True, mx_out=MXb)
    ex.sync()
    xa, xb = _natural(s, Xa, True), _natural(s, Xb, True)
    out["x_identical"] = bool(np.array_equal(xa.view(np.int64), xb.view(np.int64)))
    ma, mb = _natural(s, MXa, False), _natural(s, MXb, False)
    # longdouble M.x of the stored solution from the same term list (M: real, wavenumber independent)
    tl = s.M_tl
    assert not (np.any(tl.ex) or np.any(tl.ey) or np.any(tl.dx) or np.any(tl.dy) or np.any(tl.coef.imag != 0))
    xl = xa.astype(np.longdouble).reshape(s.R, -1)
    ref = np.zeros_like(xl)
    mag = np.zeros_like(xl)
    for r, c, v in zip(tl.row, tl.col, tl.coef.real):
        ref[r] += np.longdouble(v) * xl[c]
        mag[r] += abs(np.longdouble(v)) * abs(xl[c])
    rows = np.unique(np.asarray(tl.row))
    empty = np.setdiff1d(np.arange(s.R), rows)
    ea = np.abs(ma.reshape(s.R, -1)[rows].astype(np.longdouble) - ref[rows])
    eb = np.abs(mb.reshape(s.R, -1)[rows].astype(np.longdouble) - ref[rows])
    floor = 4 * np.finfo(np.float64).eps * mag[rows]
    # the pencils the sweep itself computes: without the flagged kx = ky = 0 cell (storage rows / columns 0, 1), whose M.X both
    # paths form with the same arithmetic and which holds the largest values
    swept = np.ones((s.nx, s.ny), dtype=bool)
    swept[:2, :2] = False
    swept = swept.reshape(-1)
    eas, ebs = ea[:, swept], eb[:, swept]
    out["err_parent_swept"] = float(eas.max())
    out["err_new_swept"] = float(ebs.max())
    out["worst_excess_swept"] = float((ebs - np.maximum(2 * eas.max(), floor[:, swept])).max())
    out["differs_from_parent"] = int(np.count_nonzero(ma.reshape(s.R, -1)[rows] != mb.reshape(s.R, -1)[rows]))
    out["err_parent"] = float(ea.max())
    out["err_new"] = float(eb.max())
    out["scale"] = float(np.abs(ref[rows]).max())
    out["worst_excess"] = float((eb - np.maximum(2 * ea.max(), floor)).max())
    out["sentinel_kept_new"] = bool(np.all(mb.reshape(s.R, -1)[empty] == SENTINEL))
    out["sentinel_kept_parent"] = bool(np.all(ma.reshape(s.R, -1)[empty] == SENTINEL))
    out["finite"] = bool(np.all(np.isfinite(mb.reshape(s.R, -1)[rows])))
    return out


def ivp_case(kind, scheme, disturb):
    shape = (32, 32, 128) if kind == "rb3d" else (64, 32)
    ends, counts, emits = [], [], []
    chk_path = None
    if disturb == 3:
        import glob
        import tempfile
        tmp = tempfile.mkdtemp()
        solver, f = _solver(kind, scheme, shape)
        chk = solver.evaluator.add_file_handler(os.path.join(tmp, "chk"), iter=3, max_writes=10)
        chk.add_tasks(solver.state, layout="g")
        for _ in range(4):
            solver.step(1e-3)
        chk.close()
        chk_path = sorted(glob.glob(os.path.join(tmp, "chk", "*.h5")))[0]
    for emit in (True, False):
        solver, f = _solver(kind, scheme, shape)
        if not emit:
            solver.pack.emits_mx = lambda *a: False         # the parent path: every M.X by the stand-alone mat-vec
        n = [0]
        real = solver.pack._matvec

        def counted(mat_id, *a, _real=real, _n=n, _s=solver, **kw):
            if mat_id == _s.M_id:
                _n[0] += 1
            return _real(mat_id, *a, **kw)

        solver.pack._matvec = counted
        per = []
        for it in range(5):
            if disturb in (1, 2) and it == 3:
                b = f["b"]
                b["c"] = np.asarray(b["c"]) * 1.25          # a user edit: the host copy becomes the authority
            if disturb == 3 and it == 3:
                solver.load_state(chk_path, index=-1)
                assert solver.iteration == 3
            before = n[0]
            solver.step(1e-3 if not (disturb == 1 and it >= 3) else 0.5e-3)
            per.append(n[0] - before)
        counts.append(per)
        emits.append(bool(getattr(solver.timestepper, "_emit", False)))
        ends.append({k: np.asarray(f[k]["c"]).copy() for k in ("b", "u", "p")})
    out = dict(emits=emits, matvecs_emit=counts[0], matvecs_parent=counts[1])
    out["rel_diff"] = {k: float(np.linalg.norm(ends[0][k] - ends[1][k]) / np.linalg.norm(ends[1][k])) for k in ends[0]}
    return out


if __name__ == "__main__":
    a = sys.argv[1:]
    if a[0] == "kernel":
        res = kernel_case(int(a[1]), int(a[2]), int(a[3]), a[4], int(a[5]), a[6] == "1")
    else:
        res = ivp_case(a[1], a[2], int(a[3]))
    print("RESULT " + json.dumps(res))
