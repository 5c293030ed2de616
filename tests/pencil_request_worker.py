"""Worker of tests/test_gpu_pencil_request.py (the sweep switches are read once per process): every case in one run.

Prints RESULT {"rejections": {name: [raised, message, untouched]}, "agree": {name: bool}, "emits": bool}."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import problems                                  # noqa: E402
import dedalus_amd.public as d3                  # noqa: E402
from dedalus_amd import libhip                   # noqa: E402


class _Null:
    @staticmethod
    def data_ptr():
        return 0


def _solver(make, **kw):
    solver, f = make(d3, timestepper="RK222", **kw)
    solver.pack.set_solve_variant(0)             # one thread per (system, block): the lean forward sweep
    if hasattr(solver, "enable_step_graph"):
        solver.enable_step_graph(False)
    for _ in range(2):
        solver.step(1e-3)
    return solver, list(solver.timestepper._lus.values())[0]


def main():
    out = dict(rejections={}, agree={})
    s, lu = _solver(problems.rayleigh_benard_3d, Nx=8, Ny=8, Nz=8)
    pack, ex, t = s.pack, s.ex, s.ex.torch
    out["emits"] = bool(s.prepare_mx_emission(lu))
    shape = (s.R, s.nx, s.ny)
    rng = np.random.default_rng(11)

    def vec(value=None):
        v = ex.zeros(shape)
        if value is None:
            v.copy_(t.as_tensor(rng.standard_normal(shape) + 3.0, device=v.device))
        else:
            v.fill_(value)
        return v

    def refused(name, call, probe):
        """`call` must raise DdhError without touching `probe` (prefilled with 7.0)"""
        ex.sync()
        try:
            call()
            raised, msg = False, ""
        except libhip.DdhError as e:
            raised, msg = True, str(e)
        ex.sync()
        out["rejections"][name] = [raised, msg, bool(t.all(probe == 7.0).item())]

    def request(name, pk, lu_id, x, **change):
        req = dict(base, x=x)
        req.update(change)
        xs, al, xx = req.pop("xs"), req.pop("alphas"), req.pop("x")
        refused(name, lambda: pk.solve(lu_id, xs, al, xx, **req), x)

    a, b, Y, MX = vec(), vec(), vec(), vec(0.0)
    zeros = t.zeros(s.R, dtype=t.uint8, device=a.device)
    base = dict(xs=[a, b], alphas=[1.0, 0.5], p_mat_id=s.P_id, work=Y, zero_rows=(zeros, 0.0), skip_rows=(zeros, 0.0), tiled=True,
                mx=(s.M_id, MX))
    plain = dict(p_mat_id=None, work=None, zero_rows=None, skip_rows=None, tiled=False, mx=None)
    x = vec(7.0)
    request("lu_id", pack, 99, x)
    request("p_mat_id", pack, lu, x, p_mat_id=99)
    request("m_mat_id", pack, lu, x, mx=(99, MX))
    request("no_terms", pack, lu, x, xs=[], alphas=[])
    request("nine_terms", pack, lu, x, xs=[a] * 9, alphas=[1.0] * 9)
    request("term_is_x", pack, lu, x, xs=[a, x])
    request("term_is_x_without_p", pack, lu, x, xs=[a, x], **plain)
    request("term_is_work", pack, lu, x, xs=[a, Y])
    request("no_work", pack, lu, x, work=None)
    request("work_is_x", pack, lu, x, work=x)
    request("no_mx_out", pack, lu, x, mx=(s.M_id, _Null))
    request("mx_out_is_x", pack, lu, x, mx=(s.M_id, x))
    request("mx_out_is_work", pack, lu, x, mx=(s.M_id, Y))
    request("mx_without_tiled", pack, lu, x, tiled=False)
    request("mx_out_without_m_mat_id", pack, lu, x, mx=(-1, MX))
    request("mx_other_matrix", pack, lu, x, mx=(s.L_id, MX))
    request("masks_without_p", pack, lu, x, **dict(plain, zero_rows=(zeros, 0.0)))
    request("skip_without_p", pack, lu, x, **dict(plain, skip_rows=(zeros, 0.0)))
    request("tiled_without_p", pack, lu, x, **dict(plain, tiled=True))
    request("mx_without_p", pack, lu, x, **dict(plain, mx=(s.M_id, MX)))
    q = libhip.PencilSolveReq()
    q.struct_size, q.nterms, q.p_mat_id, q.m_mat_id = C.sizeof(q) - 8, 1, -1, -1
    q.terms[0], q.alpha[0], q.x = a.data_ptr(), 1.0, x.data_ptr()
    refused("struct_size", lambda: libhip.call("ddh_pencil_solve", pack.handle, lu, C.byref(q), pack.dev.stream), x)
    pack.set_solve_variant(0, 0, 4)              # lean forward sweep, cooperative backward sweep: nothing is fused
    request("mx_not_emitted", pack, lu, x)
    pack.set_state_tiled(2)
    request("band_major_state_unfused", pack, lu, x, tiled=False, mx=None)
    pack.set_state_tiled(0)
    pack.set_solve_variant(2)                    # cooperative forward sweep
    request("tiled_not_lean", pack, lu, x, mx=None)
    pack.set_solve_variant(0)
    y = vec(7.0)
    refused("matvec_tiled_not_window_form", lambda: pack.matvec(s.L_id, a, y, owned=True, tiled=True), y)
    refused("matvec_flags", lambda: libhip.call("ddh_pencil_matvec", pack.handle, s.M_id, C.c_void_p(a.data_ptr()),
                                                C.c_void_p(y.data_ptr()), 4, pack.dev.stream), y)
    refused("matvec_in_place", lambda: pack.matvec(s.M_id, y, y), y)

    # ---- valid requests in each former form, bit for bit ----
    def same(u, v):
        ex.sync()
        return bool(t.equal(u.view(t.int64), v.view(t.int64)))

    x1, x2 = vec(0.0), vec(0.0)
    parts = []
    for k in range(8):                           # rows k, k + 8, ... of `a`, zero elsewhere: the sum is exact
        p = ex.zeros(shape)
        p[k::8] = a[k::8]
        parts.append(p)
    pack.solve(lu, [a], [1.0], x1)
    pack.solve(lu, parts, [1.0] * 8, x2)
    out["agree"]["one_term_and_eight"] = same(x1, x2)
    pack.solve(lu, [a, b], [1.0, 0.5], x1, p_mat_id=s.P_id, work=Y)
    pack.solve(lu, [a, b], [1.0, 0.5], x2, p_mat_id=s.P_id, work=Y, zero_rows=(zeros, 0.0), skip_rows=(zeros, 0.0))
    out["agree"]["null_masks_and_zero_masks"] = same(x1, x2)
    pack.set_solve_variant(0, 0, 4)              # the unfused recombined path: sweeps into `work`, then the P mat-vec
    pack.solve(lu, [a, b], [1.0, 0.5], x1, p_mat_id=s.P_id, work=Y)
    Y2 = vec(0.0)
    pack.solve(lu, [a, b], [1.0, 0.5], Y2)
    pack.matvec(s.P_id, Y2, x2)
    out["agree"]["unfused_p_and_matvec"] = same(x1, x2)
    out["unfused_backward_lanes"] = pack.lu_info(lu)["backward_lanes"]
    pack.set_solve_variant(0)

    # ---- two Fourier axes, ny = 12: not tile-able ----
    s, lu = _solver(problems.rayleigh_benard_3d, Nx=8, Ny=12, Nz=8)
    shape = (s.R, s.nx, s.ny)
    a, Y, x, y = vec(), vec(), vec(7.0), vec(7.0)
    zeros = t.zeros(s.R, dtype=t.uint8, device=a.device)
    base = dict(xs=[a], alphas=[1.0], p_mat_id=s.P_id, work=Y, zero_rows=None, skip_rows=None, tiled=True, mx=None)
    request("tiled_ny_12", s.pack, lu, x)
    refused("matvec_tiled_ny_12", lambda: s.pack.matvec(s.M_id, a, y, owned=True, tiled=True), y)

    # ---- two Fourier axes, nx = 12 ----
    s, lu = _solver(problems.rayleigh_benard_3d, Nx=12, Ny=8, Nz=8)
    shape = (s.R, s.nx, s.ny)
    a, Y, x, y = vec(), vec(), vec(7.0), vec(7.0)
    base = dict(xs=[a], alphas=[1.0], p_mat_id=s.P_id, work=Y, zero_rows=None, skip_rows=None, tiled=True, mx=None)
    request("tiled_nx_12", s.pack, lu, x)
    refused("matvec_tiled_nx_12", lambda: s.pack.matvec(s.M_id, a, y, owned=True, tiled=True), y)

    # ---- one Fourier axis, 8 modes ----
    s, lu = _solver(problems.rayleigh_benard_2d, Nx=16, Nz=16)
    shape = (s.R, s.nx, s.ny)
    a, Y, x, y = vec(), vec(), vec(7.0), vec(7.0)
    base = dict(xs=[a], alphas=[1.0], p_mat_id=s.P_id, work=Y, zero_rows=None, skip_rows=None, tiled=True, mx=None)
    request("tiled_one_axis", s.pack, lu, x)
    request("term_is_work_one_axis", s.pack, lu, x, xs=[Y], tiled=False)
    refused("matvec_tiled_one_axis", lambda: s.pack.matvec(s.M_id, a, y, owned=True, tiled=True), y)
    print("RESULT " + json.dumps(out))


if __name__ == "__main__":
    main()
