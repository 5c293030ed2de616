"""Reduced analysis tasks on the GPU: slices, profiles and integrals of Cartesian fields against the unmodified reference
(tests/golden/reduced_tasks.npz, tools/make_golden_reduced.py), through expr.evaluate(), a DictionaryHandler and a
FileHandler; ddh_axis_contract against NumPy; and a stepping solver whose handler holds reduced tasks.

Bounds: rel-L2 <= 1e-12 against the reference (the project's standing bound for transforms, README / DESIGN section 2);
results the reference gives as exactly zero: absolute, 1e-13 x the max-abs of the input field."""
import os
import types

import numpy as np
import pytest

import reduced_cases as rc

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reduced_tasks.npz")
TOL = 1e-12


@pytest.fixture(scope="module")
def d3():
    import dedalus_amd.public as d3
    return d3


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def _all_tasks():
    import dedalus_amd.public as d3
    from oracle.np_executor import NumpyExecutor
    out = []
    for case in rc.CASES:
        dist, cd, bases, f = rc.build(d3, case, dist_kw=dict(executor=NumpyExecutor()))       # (names only: no device)
        out.extend((case, name) for name in rc.tasks(d3, case, cd, f))
    return out


ALL_TASKS = _all_tasks()


def _compare(gold, case, name, key, got, what):
    ref = gold["%s/%s/%s" % (case, name, key)]
    got = np.asarray(got)
    assert got.shape == ref.shape, (what, case, name, key, got.shape, ref.shape)
    nr = np.linalg.norm(ref)
    if nr == 0.0:
        scale = np.abs(gold["%s/in/b" % case]).max()
        err = np.abs(got).max() / scale
        print("%s %s/%s/%s: max-abs / operand max-abs = %.3e (reference: exactly zero)" % (what, case, name, key, err))
        assert err <= 1e-13, (what, case, name, key, err)
    else:
        err = np.linalg.norm(got - ref) / nr
        print("%s %s/%s/%s: rel-L2 = %.3e" % (what, case, name, key, err))
        assert err <= TOL, (what, case, name, key, err)


def _setup(d3, gold, case):
    dist, cd, bases, f = rc.build(d3, case)
    assert dist.executor.name == "hip"
    rc.load_inputs(gold, case, f)
    return dist, rc.tasks(d3, case, cd, f)


def test_task_list_covers_the_issue():
    names3 = {n for c, n in ALL_TASKS if c == "rb3d"}
    assert names3 == {"b_x_on", "b_x_off", "b_x_left", "b_y", "u_x", "b_x_z", "dz_b_x", "dx_of_b_x", "ave_x", "ave_hor",
                      "integ_x", "integ_all", "ave_flux_hor", "ave_x_times_ave_x", "ave_x_z"}
    assert len(ALL_TASKS) == 7 + 14 + 15


@pytest.mark.parametrize("case,name", ALL_TASKS)
def test_evaluate_matches_reference(d3, gold, case, name):
    dist, tasks = _setup(d3, gold, case)
    out = tasks[name].evaluate()
    for key, arr in rc.record(out).items():
        _compare(gold, case, name, key, arr, "evaluate")


@pytest.mark.parametrize("case", list(rc.CASES))
def test_dictionary_handler_matches_reference(d3, gold, case):
    from dedalus_amd.core.output import DictionaryHandler
    dist, tasks = _setup(d3, gold, case)
    h = DictionaryHandler(types.SimpleNamespace(dist=dist, problem=None), iter=1)
    for name, expr in tasks.items():
        for layout, scale in rc.OUTPUTS:
            h.add_task(expr, layout=layout, scales=scale, name="%s:%s" % (name, rc.out_key(layout, scale)))
    h.evaluate()
    h.process(iteration=0, wall_time=0.0, sim_time=0.0, timestep=1.0)
    for name in tasks:
        for layout, scale in rc.OUTPUTS:
            key = rc.out_key(layout, scale)
            _compare(gold, case, name, key, h["%s:%s" % (name, key)][layout], "dictionary")


@pytest.mark.parametrize("case", list(rc.CASES))
def test_file_handler_matches_reference(d3, gold, case, tmp_path):
    from dedalus_amd.core.output import FileHandler
    from dedalus_amd.tools import h5lite
    dist, tasks = _setup(d3, gold, case)
    h = FileHandler(str(tmp_path / "red"), types.SimpleNamespace(dist=dist, problem=None), iter=1)
    outputs = rc.OUTPUTS + (("c", 1.5),)                    # both layouts at both scales
    for name, expr in tasks.items():
        for layout, scale in outputs:
            h.add_task(expr, layout=layout, scales=scale, name="%s:%s:%g" % (name, layout, scale))
    for it in range(2):
        h.evaluate()
        h.process(iteration=it, wall_time=0.0, sim_time=0.1 * it, timestep=0.1)
    h.close()
    r = h5lite.read(str(tmp_path / "red" / "red_s1.h5"))
    assert r.attrs["writes"] == 2
    names = rc.CASES[case][0]
    for name, expr in tasks.items():
        const = [b is None for b in expr.domain.by_axis]
        for layout, scale in outputs:
            d = r["tasks/%s:%s:%g" % (name, layout, scale)]
            assert list(d.attrs["constant"]) == const
            assert list(d.attrs["grid_space"]) == [layout == "g"] * len(names) and np.allclose(d.attrs["scales"], scale)
            labels = d.attrs["DIMENSION_LABELS"][-len(names):]
            assert labels == ["constant" if c else (n if layout == "g" else "k" + n) for c, n in zip(const, names)]
            for write in range(2):
                _compare(gold, case, name, rc.out_key(layout, 1.0 if layout == "c" else scale), d.read(write),
                         "file[%d]" % write)


def test_more_expression_forms(d3, gold):
    """Add / Power / UnaryGridFunction of reduced fields, a sum of two different slices and the gradient of a slice (the
    reductions stay leaves) -- against combinations of the reference's results that are exact in exact arithmetic."""
    case = "rb3d"
    dist, cd, bases, f = rc.build(d3, case)
    rc.load_inputs(gold, case, f)
    p = rc.positions(case)
    b, u, x = f["b"], f["u"], cd["x"]
    g = lambda n: gold["rb3d/%s/g1" % n]

    def G(e):
        o = e.evaluate()
        o.change_scales(1)
        return np.array(o["g"])

    def close(a, ref, what):
        err = np.linalg.norm(a - ref) / np.linalg.norm(ref)
        print("%s: rel-L2 = %.3e" % (what, err))
        assert a.shape == ref.shape and err <= TOL, (what, err)

    close(G(b(x=p["x_on"]) + b(x=p["x_off"])), g("b_x_on") + g("b_x_off"), "sum of two slices")
    close(G(d3.Average(b, x) + d3.Average(b, x)), 2 * g("ave_x"), "sum of equal profiles")
    close(G(b(x=p["x_on"]) - 2 * d3.Average(b, x)), g("b_x_on") - 2 * g("ave_x"), "slice minus profile")
    gr = G(d3.grad(b(x=p["x_off"])))
    assert gr.shape == (3, 1, 32, 16) and not gr[0].any()
    close(gr[2], g("dz_b_x"), "z-gradient of a slice")
    close(G(u(x=p["x_off"]) @ f["ez"]), g("u_x")[2], "component of a slice")
    # grid functions of a profile are formed on its dealiased grid (24 points in z): there they are the function of the
    # reference's profile values point by point
    prof = d3.Average(b, (x, cd["y"]))
    for e, fn in ((prof ** 2, lambda a: a ** 2), (prof ** 3, lambda a: a ** 3), (np.exp(prof), np.exp)):
        o = e.evaluate()
        assert o.layout == "g" and tuple(o.scales) == (1.0, 1.0, 1.5)
        close(np.array(o["g"]), fn(gold["rb3d/ave_hor/g15"]), "grid function of a profile")


# ---- the kernel ------------------------------------------------------------------------------------------------------

def _contract(x_d, outer, n, inner, w_d, nw, ostride=None):
    import torch
    from dedalus_amd import libhip
    from dedalus_amd.device import Device, ptr
    dev = Device.get()
    out = torch.empty((outer, nw, inner), dtype=torch.float64, device=dev.tdev)
    libhip.call("ddh_axis_contract", ptr(x_d), ptr(out), outer, n, inner, n * inner if ostride is None else ostride,
                ptr(w_d), nw, dev.stream)
    return out


# (outer, n, inner): contiguous lines; strided columns, unsplit (outer * inner >= 2^19 or a single chunk of k) and split-k
LINE_SHAPES = [(1000, 64, 1), (777, 768, 1), (513, 1024, 1), (300, 2050, 1), (64, 7, 1)]
STRIDED_SHAPES = [(40, 32, 64), (3, 512, 64), (9000, 512, 64), (5, 32, 512), (2, 512, 512), (1100, 512, 512),
                  (1, 32, 196608), (1, 512, 196608), (3, 512, 196608), (7, 100, 5), (2, 1100, 70)]


@pytest.mark.parametrize("outer,n,inner", LINE_SHAPES + STRIDED_SHAPES)
def test_axis_contract_against_numpy(outer, n, inner):
    import torch
    from dedalus_amd.device import Device
    dev = Device.get()
    rng = np.random.default_rng(outer + 3 * n + 7 * inner)
    x = rng.standard_normal((outer, n, inner))
    w = rng.standard_normal((4, n))
    x_d, w_d = dev.from_host(x), dev.from_host(w)
    ref = np.moveaxis(np.tensordot(w, x, axes=(1, 1)), 0, 1)                    # [outer][4][inner]
    mag = np.moveaxis(np.tensordot(np.abs(w), np.abs(x), axes=(1, 1)), 0, 1)
    assert np.allclose(ref[0, 1, :3], np.einsum("k,ki->i", w[1], x[0])[:3], rtol=1e-9, atol=1e-9)     # (the einsum of the ABI)
    for nw in (1, 4):
        wd = w_d[:nw].contiguous()
        a = _contract(x_d, outer, n, inner, wd, nw)
        b = _contract(x_d, outer, n, inner, wd, nw)
        torch.cuda.synchronize()
        assert torch.equal(a, b), "two calls differ"
        got = a.cpu().numpy()
        excess = np.abs(got - ref[:, :nw]) / (n * 2.0 ** -52 * mag[:, :nw])
        print("outer=%d n=%d inner=%d nw=%d: max error / bound = %.3e" % (outer, n, inner, nw, excess.max()))
        assert excess.max() <= 1.0


def test_axis_contract_unaligned_lines_and_strides():
    """odd line starts take 8-byte loads and must give the bits of the 16-byte path; ostride > n * inner skips padding"""
    import torch
    from dedalus_amd.device import Device
    dev = Device.get()
    rng = np.random.default_rng(5)
    outer, n = 200, 768
    x = rng.standard_normal((outer, n + 1))
    w_d = dev.from_host(rng.standard_normal((4, n)))
    packed = _contract(dev.from_host(np.ascontiguousarray(x[:, :n])), outer, n, 1, w_d, 4)
    padded = _contract(dev.from_host(x), outer, n, 1, w_d, 4, ostride=n + 1)
    torch.cuda.synchronize()
    assert torch.equal(packed, padded)


def test_axis_contract_split_and_unsplit_agree_bitwise():
    """the same columns through the split-k launch (few columns) and the unsplit one (many): identical bits"""
    import torch
    from dedalus_amd.device import Device
    dev = Device.get()
    rng = np.random.default_rng(11)
    outer, n, inner = 1100, 200, 512                        # 4 chunks of k; 1100 * 512 columns >= 2^19: unsplit
    x_d = dev.from_host(rng.standard_normal((outer, n, inner)))
    w_d = dev.from_host(rng.standard_normal((4, n)))
    big = _contract(x_d, outer, n, inner, w_d, 4)
    small = _contract(x_d, 3, n, inner, w_d, 4)             # 3 * 512 columns: split over the waves of a workgroup
    torch.cuda.synchronize()
    assert torch.equal(big[:3], small)


def test_axis_contract_mode0_gather_reads_only_the_slab():
    import torch
    from dedalus_amd.device import Device
    dev = Device.get()
    rng = np.random.default_rng(3)
    for outer, N, inner in ((37, 64, 1), (16, 32, 48), (256, 512, 512)):
        x = rng.standard_normal((outer, N, inner))
        x[:, 1:, :] = np.nan                                # anything but k = 0 would poison the result
        out = _contract(dev.from_host(x), outer, 1, inner, dev.from_host(np.array([[0.25]])), 1, ostride=N * inner)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy()[:, 0, :], 0.25 * x[:, 0, :])


@pytest.mark.parametrize("outer,n,inner", [(50, 768, 1), (10, 2050, 1), (1100, 512, 512), (2, 512, 512), (40, 32, 64)])
def test_axis_contract_propagates_nan(outer, n, inner):
    import torch
    from dedalus_amd.device import Device
    dev = Device.get()
    rng = np.random.default_rng(2)
    x = rng.standard_normal((outer, n, inner))
    w = rng.standard_normal((4, n))
    o0, k0, i0 = outer // 2, n - 3, inner // 3
    w[2, k0] = 0.0                                          # a zero weight does not hide it
    x[o0, k0, i0] = np.nan
    out = _contract(dev.from_host(x), outer, n, inner, dev.from_host(w), 4)
    torch.cuda.synchronize()
    bad = np.isnan(out.cpu().numpy())
    expect = np.zeros_like(bad)
    expect[o0, :, i0] = True
    assert np.array_equal(bad, expect)


def test_axis_contract_rejects_bad_arguments():
    from dedalus_amd import libhip
    from dedalus_amd.device import Device
    dev = Device.get()
    x_d, w_d = dev.from_host(np.zeros((2, 8, 4))), dev.from_host(np.zeros((5, 8)))
    with pytest.raises(libhip.DdhError, match="weight vectors"):
        _contract(x_d, 2, 8, 4, w_d, 5)
    with pytest.raises(libhip.DdhError, match="ostride"):
        _contract(x_d, 2, 8, 4, w_d, 1, ostride=16)


# ---- a stepping solver with reduced tasks ------------------------------------------------------------------------------

def test_solver_with_reduced_handler_steps_identically(d3):
    """3-D Rayleigh-Benard 64 x 64 x 32, RK222: a handler with a slice, a profile and a volume integral at iter=1 reads the
    (tile-major) state between steps; the end state is bit-identical to the run without it, and the profile is the x-y
    mean of the full-field output."""
    import problems

    def run(with_handler):
        solver, f = problems.rayleigh_benard_3d(d3, Nx=64, Ny=64, Nz=32, timestepper="RK222")
        h = None
        if with_handler:
            b = f["b"]
            h = solver.evaluator.add_dictionary_handler(iter=1)
            h.add_task(b(x=1.0), name="slice")
            h.add_task(d3.Average(b, ("x", "y")), name="profile")
            h.add_task(d3.Integrate(b), name="volume")
            h.add_task(b, name="b")
        for _ in range(4):
            solver.step(1e-3)
        seen = None
        if with_handler:                                    # once more on the end state, read at once: the tasks see one state
            solver.evaluator.evaluate_handlers([h], iteration=int(solver.iteration), wall_time=0.0,
                                               sim_time=float(solver.sim_time), timestep=1e-3)
            seen = {k: np.array(h[k]["g"]) for k in ("slice", "profile", "volume", "b")}
        return {k: np.array(f[k]["c"]) for k in ("p", "b", "u")}, seen

    plain, _ = run(False)
    watched, h = run(True)
    for k in plain:
        assert np.array_equal(plain[k], watched[k]), k
    full, prof = h["b"], h["profile"]                       # (scale 1: the Fourier grid means are the k = 0 modes)
    assert full.shape == (64, 64, 32) and prof.shape == (1, 1, 32)
    ref = full.mean(axis=(0, 1))
    err = np.linalg.norm(prof[0, 0] - ref) / np.linalg.norm(ref)
    print("profile vs x-y mean of the full field: rel-L2 = %.3e" % err)
    assert err <= 1e-12
    assert h["slice"].shape == (1, 64, 32) and h["volume"].shape == (1, 1, 1)
