"""Reduced analysis tasks of sphere and shell fields on the GPU: the golden tasks of tests/curvilinear_reduced_cases.py
through expr.evaluate(), a DictionaryHandler and a FileHandler (bound: the 1e-11 x max|golden| of the host twin,
tests/test_curvilinear_reduced_host.py); no full-grid download; ddh_axis_contract_rows against NumPy; a stepping shell
solver whose handler holds the new task kinds."""
import os
import types

import numpy as np
import pytest

import curvilinear_reduced_cases as cc
from test_curvilinear_reduced_host import GOLD, TOL, compare

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def d3():
    import dedalus_amd.public as d3
    return d3


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def _setup(d3, gold, case):
    dist, coords, basis, f = cc.build(d3, case)
    assert dist.executor.name == "hip"
    cc.load_inputs(gold, case, f)
    return dist, coords, basis, f


@pytest.mark.parametrize("case", list(cc.CASES))
def test_evaluate_matches_reference(d3, gold, case):
    dist, coords, basis, f = _setup(d3, gold, case)
    for name, expr in cc.tasks(d3, case, coords, f).items():
        compare(gold, case, name, expr.evaluate())


@pytest.mark.parametrize("case", list(cc.CASES))
def test_handlers_match_reference(d3, gold, case, tmp_path):
    from dedalus_amd.core.output import DictionaryHandler, FileHandler
    from dedalus_amd.tools import h5lite
    dist, coords, basis, f = _setup(d3, gold, case)
    tasks = cc.tasks(d3, case, coords, f)
    solver = types.SimpleNamespace(dist=dist, problem=None)
    fh = FileHandler(str(tmp_path / "red"), solver, iter=1)
    dh = DictionaryHandler(solver, iter=1)
    for name, expr in tasks.items():
        fh.add_task(expr, layout="g", scales=cc.DEALIAS, name=name)
        dh.add_task(expr, layout="g", scales=cc.DEALIAS, name=name)
    for h in (fh, dh):
        h.evaluate()
        h.process(iteration=0, wall_time=0.0, sim_time=0.0, timestep=0.1)
    fh.close()
    r = h5lite.read(str(tmp_path / "red" / "red_s1.h5"))
    for name, expr in tasks.items():
        ref = gold["%s/%s/g15" % (case, name)]
        d = r["tasks/" + name]
        assert list(d.attrs["constant"]) == [i in expr.const_axes for i in range(dist.dim)]
        for what, got in (("file", d.read(0)), ("dictionary", np.asarray(dh[name]["g"]))):
            assert got.shape == ref.shape, (what, name)
            err = np.abs(got - ref).max() / np.abs(ref).max()
            print("%s %s/%s: %.3e" % (what, case, name, err))
            assert err <= TOL, (what, case, name, err)


def test_no_full_grid_leaves_the_device(d3, gold, monkeypatch):
    """the shell example's meridional flux slices and the other task kinds download their reduced result only"""
    case = "shell_16_12_8"
    dist, coords, basis, f = _setup(d3, gold, case)
    tasks = cc.tasks(d3, case, coords, f)
    ex = dist.executor
    seen = []
    real = ex.download
    monkeypatch.setattr(ex, "download", lambda t: (seen.append(int(t.numel())), real(t))[1])
    for name in ("flux_phi", "b_phi", "u_theta", "bu_theta", "ave_phi_u", "ave_S2_b"):
        del seen[:]
        out = tasks[name].evaluate()
        out.change_scales(cc.DEALIAS)
        got = np.asarray(out["g"])
        assert seen == [got.size], (name, seen, got.size)


# ---- the kernel ------------------------------------------------------------------------------------------------------

def _rows(x_d, outer, n, inner, w_d, row_d, kmin_d, nrows, out=None):
    import ctypes as C
    import torch
    from dedalus_amd import libhip
    from dedalus_amd.device import Device, ptr
    dev = Device.get()
    if out is None:
        out = torch.empty((outer, inner), dtype=torch.float64, device=dev.tdev)
    libhip.call("ddh_axis_contract_rows", ptr(x_d), ptr(out), outer, n, inner, ptr(w_d), C.c_void_p(row_d.data_ptr()),
                C.c_void_p(kmin_d.data_ptr()), nrows, dev.stream)
    return out


def _problem(rng, outer, n, inner, nrows):
    """random data, rows and kmin; kmin = 0, n - 1 and n are always among the rows in use"""
    x = rng.standard_normal((outer, n, inner))
    w = rng.standard_normal((nrows, n))
    row = rng.integers(0, nrows, size=outer).astype(np.int32)
    kmin = rng.integers(0, n + 1, size=nrows).astype(np.int32)
    edges = (0, n - 1, n)
    if nrows == 1:
        kmin[0] = edges[(outer + n + inner) % 3]
    else:
        kmin[:3] = edges
        row[:3] = np.arange(3)[:min(outer, 3)] if outer >= 3 else (outer + n + inner) % 3
    return x, w, row, kmin


def _ints(a):
    import torch
    from dedalus_amd.device import Device
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32), device=Device.get().tdev)


def _reference(x, w, row, kmin):
    n = x.shape[1]
    live = (np.arange(n)[None, :] >= kmin[row][:, None])[:, :, None]
    xl = np.where(live, x, 0.0).astype(np.longdouble)
    wl = w[row].astype(np.longdouble)[:, :, None]
    return (wl * xl).sum(axis=1), (np.abs(wl) * np.abs(xl)).sum(axis=1).astype(np.float64)


@pytest.mark.parametrize("inner", [1, 2, 3, 12, 64, 65, 200])
def test_axis_contract_rows_against_numpy(inner):
    """|err| <= n 2^-52 sum_k |w_k x_k| per element: the a-priori bound of a fixed-order sum with fused or unfused products.
    Aligned bases and bases offset by one double (the scalar path), which must agree bit for bit."""
    import torch
    from dedalus_amd.device import Device
    dev = Device.get()
    for outer in (1, 5, 64):
        for n in (1, 3, 63, 64, 65, 257):
            for nrows in (1, 7):
                rng = np.random.default_rng(1000 * outer + 10 * n + inner + nrows)
                x, w, row, kmin = _problem(rng, outer, n, inner, nrows)
                ref, mag = _reference(x, w, row, kmin)
                w_d, row_d, kmin_d = dev.from_host(w), _ints(row), _ints(kmin)
                x_d = dev.from_host(x)
                pad = dev.from_host(np.concatenate([[0.0], x.reshape(-1)]))
                outpad = torch.full((outer * inner + 1,), float("nan"), dtype=torch.float64, device=dev.tdev)
                a = _rows(x_d, outer, n, inner, w_d, row_d, kmin_d, nrows)
                b = _rows(x_d, outer, n, inner, w_d, row_d, kmin_d, nrows)
                c = _rows(pad[1:], outer, n, inner, w_d, row_d, kmin_d, nrows, out=outpad[1:].view(outer, inner))
                torch.cuda.synchronize()
                assert torch.equal(a, b), "two calls differ"
                assert torch.equal(a, c), "aligned and offset bases differ"
                assert bool(torch.isnan(outpad[0]))
                got = a.cpu().numpy()
                err = np.abs((got.astype(np.longdouble) - ref).astype(np.float64))
                bound = n * 2.0 ** -52 * mag
                assert np.all(err <= bound), (outer, n, inner, nrows, float((err - bound).max()))
                dead = kmin[row] == n
                assert not got[dead].any() and not np.signbit(got[dead]).any()         # kmin == n: exact +0


@pytest.mark.parametrize("outer,n,inner", [(40, 127, 1), (40, 126, 1), (7, 300, 1), (5, 127, 12), (3, 127, 65), (64, 257, 64),
                                            (2, 40, 200)])
def test_axis_contract_rows_nan_behaviour(outer, n, inner):
    import torch
    from dedalus_amd.device import Device
    dev = Device.get()
    rng = np.random.default_rng(outer + n + inner)
    nrows = 3
    x = rng.standard_normal((outer, n, inner))
    w = rng.standard_normal((nrows, n))
    row = (np.arange(outer) % nrows).astype(np.int32)
    kmin = np.array([n // 3, 5 if n > 5 else 0, n // 2 + 1], dtype=np.int32)
    for o in range(outer):
        x[o, :kmin[row[o]], :] = np.nan                        # never read
    guard = 64
    buf = torch.full((outer * inner + guard,), float("nan"), dtype=torch.float64, device=dev.tdev)
    out = buf[:outer * inner].view(outer, inner)
    w_d, row_d, kmin_d = dev.from_host(w), _ints(row), _ints(kmin)
    _rows(dev.from_host(x), outer, n, inner, w_d, row_d, kmin_d, nrows, out=out)
    torch.cuda.synchronize()
    assert not np.isnan(out.cpu().numpy()).any(), "an entry below kmin reached the output"
    assert bool(torch.isnan(buf[outer * inner:]).all()), "the guard behind the output was written"
    # a NaN at k >= kmin under a zero weight does appear -- in that column alone
    o0, i0 = outer // 2, inner // 3
    k0 = int(kmin[row[o0]])
    w[row[o0], k0] = 0.0
    x[o0, k0, i0] = np.nan
    _rows(dev.from_host(x), outer, n, inner, dev.from_host(w), row_d, kmin_d, nrows, out=out)
    torch.cuda.synchronize()
    bad = np.isnan(out.cpu().numpy())
    expect = np.zeros_like(bad)
    expect[o0, i0] = True
    assert np.array_equal(bad, expect)


def test_axis_contract_rows_split_and_unsplit_agree_bitwise():
    """the same lines through the split-k launch (few columns) and embedded in a large outer (unsplit): identical bits"""
    import torch
    from dedalus_amd.device import Device
    dev = Device.get()
    rng = np.random.default_rng(11)
    outer, n, inner, nrows = 8300, 65, 64, 7                  # two chunks of k
    x = rng.standard_normal((outer, n, inner))
    w = rng.standard_normal((nrows, n))
    row = rng.integers(0, nrows, size=outer).astype(np.int32)
    kmin = np.array([0, 1, 31, 64, 65, 63, 17], dtype=np.int32)
    w_d, row_d, kmin_d = dev.from_host(w), _ints(row), _ints(kmin)
    pad = dev.from_host(np.concatenate([[0.0], x.reshape(-1)]))          # odd base: one column per thread, 8300 * 64 >= 2^19
    big = _rows(pad[1:], outer, n, inner, w_d, row_d, kmin_d, nrows)
    small = _rows(pad[1:], 3, n, inner, w_d, row_d, kmin_d, nrows)        # split over the waves of a workgroup
    vec = _rows(dev.from_host(x[:3]), 3, n, inner, w_d, row_d, kmin_d, nrows)     # 16-byte loads, split
    torch.cuda.synchronize()
    assert torch.equal(big[:3], small) and torch.equal(small, vec)


def test_axis_contract_rows_rejects_bad_arguments():
    import torch
    from dedalus_amd import libhip
    from dedalus_amd.device import Device
    dev = Device.get()
    x_d, w_d = dev.from_host(np.ones((2, 8, 4))), dev.from_host(np.ones((1, 8)))
    row_d, kmin_d = _ints([0, 0]), _ints([0])
    out = torch.full((2, 4), 7.0, dtype=torch.float64, device=dev.tdev)
    with pytest.raises(libhip.DdhError, match="empty shape"):
        _rows(x_d, 2, 0, 4, w_d, row_d, kmin_d, 1, out=out)
    with pytest.raises(libhip.DdhError, match="no weight rows"):
        _rows(x_d, 2, 8, 4, w_d, row_d, kmin_d, 0, out=out)
    with pytest.raises(libhip.DdhError, match="null pointer"):
        libhip.call("ddh_axis_contract_rows", None, None, 2, 8, 4, None, None, None, 1, dev.stream)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()), "a refused call launched"


# ---- a stepping solver with the new task kinds ---------------------------------------------------------------------------

def test_shell_solver_with_reduced_handler_steps_identically(d3):
    import problems

    def run(with_handler):
        solver, f = problems.shell_convection(d3, shape=(16, 12, 8))
        if with_handler:
            b, u = f["b"], f["u"]
            coords = solver.dist.coordsys
            h = solver.evaluator.add_dictionary_handler(iter=1)
            h.add_task(b(phi=1.0), scales=3 / 2, name="meridional")
            h.add_task(u(theta=0.7), scales=3 / 2, name="conical")
            h.add_task(d3.Average(u, coords["phi"]), name="zonal")
            h.add_task(d3.Average(b, coords.S2coordsys), name="profile")
            h.add_task(d3.Average(b * (u @ u), coords.S2coordsys), name="flux profile")
        for _ in range(3):
            solver.step(0.05)
        shapes = {k: np.asarray(h[k]["g"]).shape for k in h.fields} if with_handler else None
        return {k: np.array(f[k]["c"]) for k in ("p", "b", "u")}, shapes

    plain, _ = run(False)
    watched, shapes = run(True)
    for k in plain:
        assert np.array_equal(plain[k], watched[k]), k
    assert shapes == {"meridional": (1, 18, 12), "conical": (3, 24, 1, 12), "zonal": (3, 1, 12, 8), "profile": (1, 1, 8),
                      "flux profile": (1, 1, 8)}
