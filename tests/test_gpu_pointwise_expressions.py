"""GPU: grid functions, powers, quotients and products with profile fields reach grid space on the device -- no transfer to
or from the host while the expression is evaluated (HipExecutor.download / from_host raise meanwhile), the map kernels'
launch counter advances, and the values are NumPy's on the operand's own grid data within the bounds of
tests/grid_map_cases.py (bit for bit where the function is one IEEE operation)."""
import ctypes as C

import numpy as np
import pytest

import grid_map_cases as mc

pytestmark = pytest.mark.gpu

DEALIAS = 3 / 2


def launches():
    from dedalus_amd import libhip
    count = C.c_long(-1)
    libhip.call("ddh_grid_map_launches", C.byref(count))
    return count.value


def _host_trip(*a, **k):
    raise AssertionError("grid data crossed to the host while an expression was evaluated")


def on_device(monkeypatch, fn):
    """fn() once to warm every cache (plans, constant operators, the fields' device copies), then again with the host
    transfers of the executor forbidden -> (result of the second call, map / broadcast launches during it)"""
    from dedalus_amd.executor import HipExecutor
    fn()
    with monkeypatch.context() as m:
        m.setattr(HipExecutor, "download", _host_trip)
        m.setattr(HipExecutor, "from_host", _host_trip)
        before = launches()
        out = fn()
        count = launches() - before
    return out, count


def grid(f):
    f.change_scales(DEALIAS)
    return np.array(f["g"])


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


@pytest.fixture(scope="module")
def fields():
    import dedalus_amd.public as d3
    coords = d3.CartesianCoordinates("x", "z")
    dist = d3.Distributor(coords, dtype=np.float64)
    assert dist.executor.name == "hip"
    xb = d3.RealFourier(coords["x"], size=16, bounds=(0, 2 * np.pi), dealias=DEALIAS)
    zb = d3.ChebyshevT(coords["z"], size=12, bounds=(0, 1), dealias=DEALIAS)
    x, z = dist.local_grids(xb, zb)
    b = dist.Field(name="b", bases=(xb, zb))
    b["g"] = 2.0 + 0.5 * np.sin(x) * z + 0.25 * np.cos(2 * x) * (1 - z * z)              # shifted positive
    u = dist.VectorField(coords, name="u", bases=(xb, zb))
    u["g"][0] = np.cos(x) * (1 + z) + 0.3 * np.sin(3 * x) * z * z
    u["g"][1] = 0.7 * np.sin(2 * x) * (z - 0.5) - 0.2 * np.cos(x) + 0.1
    ez = dist.VectorField(coords, name="ez")
    ez["g"][1] = 1
    N2 = dist.Field(name="N2", bases=zb)
    N2["g"] = 1.0 + z ** 2 + 0.5 * z ** 3
    N2full = dist.Field(name="N2full", bases=(xb, zb))
    N2full["g"] = 1.0 + z ** 2 + 0.5 * z ** 3 + 0 * x
    return dict(d3=d3, dist=dist, b=b, u=u, ez=ez, N2=N2, N2full=N2full, bases=(xb, zb))


def _within(got, op, x, p=0.0):
    if op in mc.EXACT or (op == "pow" and p in mc.POW_EXACT):
        assert same_bits(got, mc.numpy_map(op, x, p)), op
        return
    bound = mc.powi_bound(p) if op == "pow" and mc.pow_is_repeated_multiplication(p) else mc.BOUNDS[op]
    r = mc.ulp_ratio(got, mc.reference(op, x, p))
    print("%s p=%g error %.4f U, bound %d U" % (op, p, r, bound))
    assert r <= bound, (op, p, r, bound)


@pytest.mark.parametrize("name", ["sin", "tanh", "pow3", "pow2.5", "pow-1"])
def test_functions_and_powers_of_a_scalar_field(fields, monkeypatch, name):
    b = fields["b"]
    bg = grid(b)
    expr, op, p = {"sin": (np.sin(b), "sin", 0.0), "tanh": (np.tanh(b), "tanh", 0.0), "pow3": (b ** 3, "pow", 3),
                   "pow2.5": (b ** 2.5, "pow", 2.5), "pow-1": (b ** (-1), "pow", -1)}[name]
    out, count = on_device(monkeypatch, expr.evaluate)
    assert count == 1
    _within(grid(out), op, bg, p)


def test_speed_of_a_vector_field(fields, monkeypatch):
    u = fields["u"]
    uu = grid((u @ u).evaluate())
    out, count = on_device(monkeypatch, np.sqrt(u @ u).evaluate)
    assert count == 1
    assert same_bits(grid(out), np.sqrt(uu))


def test_quotients(fields, monkeypatch):
    d3, b, u = fields["d3"], fields["b"], fields["u"]
    bg, ug = grid(b), grid(u)
    # u / b = Multiply(u, Power(b, -1)): one reciprocal and one product per point, both IEEE operations
    out, count = on_device(monkeypatch, (u / b).evaluate)
    assert count == 1
    assert np.array_equal(grid(out), ug * (1 / bg))
    # 1 / b = 1 * Power(b, -1) is linear in the power node: the node's grid data (1 / b bit for bit, above) pass through
    # the coefficients of the domain -- compare with a field holding 1 / b on the dealiased grid, truncated the same way
    out, count = on_device(monkeypatch, (1 / b).evaluate)
    assert count == 1
    r = fields["dist"].Field(bases=fields["bases"])
    r.change_scales(DEALIAS)
    r["g"] = 1 / bg
    r["c"]
    ref, got = grid(r), grid(out)
    assert np.linalg.norm(got - ref) <= 1e-13 * np.linalg.norm(ref)
    out, count = on_device(monkeypatch, np.true_divide(u, b).evaluate)
    assert count == 1 and np.array_equal(grid(out), ug * (1 / bg))


def test_product_with_a_profile_field_is_broadcast_on_the_device(fields, monkeypatch):
    u, ez, N2, N2full = (fields[k] for k in ("u", "ez", "N2", "N2full"))
    out, count = on_device(monkeypatch, (N2 * (u @ ez)).evaluate)
    assert count == 1                                   # the broadcast of N2
    ref, count = on_device(monkeypatch, (N2full * (u @ ez)).evaluate)
    assert count == 0
    assert same_bits(grid(out), grid(ref))
    assert np.abs(grid(out)).max() > 0.1


def test_square_stays_on_the_bilinear_kernel(fields, monkeypatch):
    b = fields["b"]
    bg = grid(b)
    out, count = on_device(monkeypatch, (b ** 2).evaluate)
    assert count == 0
    assert same_bits(grid(out), bg * bg)


def test_unknown_grid_function_raises_its_name(fields):
    with pytest.raises(NotImplementedError, match="cbrt"):
        np.cbrt(fields["b"]).evaluate()


# ---- reaction-diffusion: the map kernels inside F, once per step, and inside a replayed step --------------------------------
def _reaction_diffusion(d3, rhs, graph=None, dist_kw=None):
    xcoord = d3.Coordinate("x")
    dist = d3.Distributor(xcoord, dtype=np.float64, **(dist_kw or {}))
    xbasis = d3.RealFourier(xcoord, size=64, bounds=(0, 2 * np.pi), dealias=DEALIAS)
    u = dist.Field(name="u", bases=xbasis)
    dx = lambda A: d3.Differentiate(A, xcoord)
    problem = d3.IVP([u], namespace=locals())
    problem.add_equation("dt(u) - dx(dx(u)) = " + rhs)
    x = dist.local_grid(xbasis)
    u["g"] = 0.8 * np.sin(x) + 0.5 * np.cos(3 * x) + 0.1 * np.sin(7 * x + 0.3)
    solver = problem.build_solver(d3.SBDF2)
    if graph is not None:
        solver.enable_step_graph(graph)
    for _ in range(20):
        solver.step(2e-3)
    return solver, np.array(u["c"])


@pytest.mark.parametrize("rhs", ["u - u**3", "-np.sin(u)"])
def test_reaction_diffusion_matches_the_oracle_and_replays_from_graphs(rhs):
    import dedalus_amd.public as d3
    from oracle.np_executor import NumpyExecutor
    before = launches()
    plain, c_plain = _reaction_diffusion(d3, rhs, graph=False)
    assert plain.ex.name == "hip"
    assert launches() - before >= 20                   # the map kernel ran in every evaluation of F
    _, c_ref = _reaction_diffusion(d3, rhs, dist_kw=dict(executor=NumpyExecutor()))
    err = np.linalg.norm(c_plain - c_ref) / np.linalg.norm(c_ref)
    print("%s: end state rel-L2 vs oracle %.3e" % (rhs, err))
    assert err <= 1e-10
    replay, c_replay = _reaction_diffusion(d3, rhs, graph=True)
    assert replay._graph["graphs"] and not replay._graph["failed"]
    assert replay.iteration == plain.iteration and abs(replay.sim_time - plain.sim_time) < 1e-15
    assert same_bits(c_replay, c_plain)


# ---- shell ------------------------------------------------------------------------------------------------------------
def test_shell_speed_is_mapped_on_the_device(monkeypatch):
    import dedalus_amd.public as d3
    Ri, Ro = 0.7, 1.9
    coords = d3.SphericalCoordinates("phi", "theta", "r")
    dist = d3.Distributor(coords, dtype=np.float64)
    shell = d3.ShellBasis(coords, shape=(16, 12, 8), radii=(Ri, Ro), dealias=DEALIAS, dtype=np.float64)
    u = dist.VectorField(coords, name="u", bases=shell)
    phi, theta, r = dist.local_grids(shell)
    ug = np.zeros((3,) + np.broadcast(phi, theta, r).shape)
    ug[0] = 0.8 * np.sin(theta) * (r - Ri) * (Ro - r) * (1 + 0.2 * np.sin(2 * phi))
    ug[1] = 0.5 * np.sin(theta) * np.cos(phi) * (r - Ri) * (Ro - r)
    ug[2] = 0.3 * np.cos(theta) * (r - Ri) * (Ro - r) + 0.1 * np.sin(theta) * np.sin(phi)
    u["g"] = ug
    ex = dist.executor
    assert ex.name == "hip"
    uu = ex.download((u @ u).eval_g())
    out, count = on_device(monkeypatch, np.sqrt(u @ u).grid_native)
    assert count == 1
    assert uu.min() >= 0 and uu.max() > 0.01
    assert same_bits(ex.download(out), np.sqrt(uu))
