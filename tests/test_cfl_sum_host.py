"""CPU: the term lists flow_tools.CFL builds for the fused CFL reduction (HipExecutor.cfl_sum_max / ddh_grid_cfl_sum), through
a fake executor that records them and evaluates them with NumPy, and the cases of tests/cfl_sum_cases.py themselves."""
import numpy as np
import pytest

import cfl_sum_cases as cc
import problems
from oracle.np_executor import NumpyExecutor


class FakeSumExecutor(NumpyExecutor):
    """NumpyExecutor plus cfl_sum_max: float64 NumPy over the term descriptors, every call recorded"""

    def __init__(self):
        super().__init__()
        self.sum_calls = []
        self.single_calls = 0

    def cfl_max(self, *a, **kw):
        self.single_calls += 1
        return super().cfl_max(*a, **kw)

    def cfl_sum_max(self, terms, shape):
        self.sum_calls.append((terms, tuple(shape)))
        k = len(shape)
        host = []
        for t in terms:
            own = tuple(1 if b else n for n, b in zip(shape, t["bcast"]))
            d = np.asarray(t["data"], dtype=np.float64)
            assert d.size % int(np.prod(own)) == 0, (d.shape, own)
            h = dict(t, data=d.reshape((-1,) + own))
            if t["kind"] == "velocity":
                assert h["data"].shape[0] == len(t["comp_axis"])
                for ax, inv in zip(t["comp_axis"], t["inv"]):
                    assert (ax is None) == (inv is None) and (ax is None or np.asarray(inv).shape == (shape[ax],))
                h["inv"] = [None if a is None else np.asarray(a) for a in t["inv"]]
            elif t["kind"] == "shell":
                assert all(np.asarray(a).shape == (shape[k - 1],) for a in t["inv"])
            host.append(h)
        f = cc.frequency_field(host, tuple(shape), dtype=np.float64)
        return float(np.max(f)) if not np.isnan(f).any() else float("nan")


def _rb(fake, Nx=16, Nz=8):
    import dedalus_amd.public as d3
    solver, f = problems.rayleigh_benard_2d(d3, Nx=Nx, Nz=Nz, dist_kw=dict(executor=fake))
    u, b = f["u"], f["b"]
    xb, zb = u.domain.bases
    x, z = u.dist.local_grids(xb, zb)
    ug = np.zeros((2,) + np.broadcast(x, z).shape)
    ug[0] = 0.5 * np.sin(2 * np.pi * x / 4) * z * (1 - z) * 4
    ug[1] = 0.3 * np.cos(4 * np.pi * x / 4) * z * (1 - z) * 4
    u["g"] = ug
    return d3, solver, f, (xb, zb)


def test_one_velocity_keeps_the_single_velocity_reduction():
    fake = FakeSumExecutor()
    d3, solver, f, _ = _rb(fake)
    cfl = d3.CFL(solver, initial_dt=0.01, cadence=1, safety=0.5)
    cfl.add_velocity(f["u"])
    for _ in range(3):
        solver.step(cfl.compute_timestep())
    assert fake.single_calls == 3 and not fake.sum_calls


def test_term_list_kinds_order_and_broadcast_flags():
    """u, N(z), B on x only (its z component has no basis), a constant field, sqrt(b b): five terms in the order added, on
    the storage grid of the dealiased domain; storage order is (z, x)"""
    fake = FakeSumExecutor()
    d3, solver, f, (xb, zb) = _rb(fake)
    dist, u, b = f["u"].dist, f["u"], f["b"]
    coords = u.tensorsig[0]
    x, z = dist.local_grids(xb, zb)
    N = dist.Field(name="N", bases=zb)
    N["g"] = 3.0 * (1 + z)
    B = dist.VectorField(coords, name="B", bases=xb)
    B["g"][0] = 1.5 * np.cos(2 * np.pi * x / 4)
    B["g"][1] = 7.0
    c0 = dist.Field(name="c0")
    c0["g"] = 0.75
    cfl = d3.CFL(solver, initial_dt=0.01, cadence=1, safety=0.5)
    cfl.add_velocity(u)
    cfl.add_frequency(N)
    cfl.add_velocity(B)
    cfl.add_frequency(c0)
    cfl.add_frequency(np.sqrt(b * b))
    assert dist.storage_order == (1, 0)
    # the value sampled at the start of the step, against the grid data of the same fields: |u_x|/dx + |u_z|/dz + |N| + |B_x|/dx + |c0| + |b|
    sc = u.domain.dealias
    for fld in (u, N, B, c0, b):
        fld.change_scales(sc if fld is not c0 else 1)
    dx = 1.5 * 4 / 24
    theta = np.pi * (np.arange(12) + 0.5) / 12
    dz = 1.5 * 0.5 * np.sin(theta) * np.pi / 12
    want = (np.abs(u["g"][0]) / dx + np.abs(u["g"][1]) / dz[None, :] + np.abs(N["g"]) + np.abs(B["g"][0]) / dx
            + np.abs(c0["g"]) + np.abs(b["g"]))
    solver.step(cfl.compute_timestep())
    assert fake.single_calls == 0 and len(fake.sum_calls) == 1
    terms, shape = fake.sum_calls[0]
    assert shape == (12, 24)
    assert [t["kind"] for t in terms] == ["velocity", "scalar", "velocity", "scalar", "scalar"]
    assert [list(t["bcast"]) for t in terms] == [[0, 0], [0, 1], [1, 0], [1, 1], [0, 0]]
    assert list(terms[0]["comp_axis"]) == [1, 0] and list(terms[2]["comp_axis"]) == [1, None]
    assert terms[2]["inv"][1] is None and np.asarray(terms[2]["inv"][0]).shape == (24,)
    assert np.asarray(terms[2]["data"]).size == 2 * 24 and np.asarray(terms[1]["data"]).size == 12
    assert abs(cfl._max_freq - want.max()) <= 1e-12 * want.max()
    # the list is built once: the next sample reuses the descriptors and only fetches the data
    built = cfl._terms
    solver.step(cfl.compute_timestep())
    assert cfl._terms is built and len(fake.sum_calls) == 2
    assert abs(cfl.compute_timestep() - 0.5 / cfl._max_freq) < 1e-15


def test_velocity_without_a_vertical_basis_alone_goes_through_the_sum():
    fake = FakeSumExecutor()
    d3, solver, f, (xb, zb) = _rb(fake)
    dist = f["u"].dist
    B = dist.VectorField(f["u"].tensorsig[0], name="B", bases=xb)
    B["g"][0] = 2.0
    B["g"][1] = 9.0
    cfl = d3.CFL(solver, initial_dt=0.01, cadence=1, safety=0.5)
    cfl.add_velocity(B)
    solver.step(cfl.compute_timestep())
    assert fake.single_calls == 0 and len(fake.sum_calls) == 1
    assert abs(cfl._max_freq - 2.0 / (1.5 * 4 / 24)) < 1e-12


def test_incompatible_grids_raise_value_error():
    fake = FakeSumExecutor()
    d3, solver, f, (xb, zb) = _rb(fake)
    dist = f["u"].dist
    other = d3.RealFourier(dist.coords[0], size=20, bounds=(0, 4), dealias=3 / 2)
    g = dist.Field(name="g", bases=other)
    g["g"] = 1.0
    cfl = d3.CFL(solver, initial_dt=0.01, cadence=1, safety=0.5)
    cfl.add_velocity(f["u"])
    cfl.add_frequency(g)
    with pytest.raises(ValueError):
        solver.step(0.01)
    with pytest.raises(ValueError):
        cfl.add_frequency(f["u"])                   # a vector is no frequency
    with pytest.raises(ValueError):
        cfl.add_velocity(f["b"])


def test_an_executor_without_the_fused_reduction_raises():
    import dedalus_amd.public as d3
    solver, f = problems.rayleigh_benard_2d(d3, Nx=16, Nz=8, dist_kw=dict(executor=NumpyExecutor()))
    cfl = d3.CFL(solver, initial_dt=0.01, cadence=1, safety=0.5)
    cfl.add_velocity(f["u"])
    cfl.add_frequency(f["b"])
    with pytest.raises(NotImplementedError):
        solver.step(0.01)


def test_sharded_axis_terms_are_the_ranks_local_block():
    """the term list of rank 1 of 2 (the distributor's rank and size set by hand: nothing is transformed or exchanged while
    the list is built): spacings and shapes are the rank's block of the sharded grid axis z"""
    fake = FakeSumExecutor()
    d3, solver, f, (xb, zb) = _rb(fake)
    dist, u = f["u"].dist, f["u"]
    N = dist.Field(name="N", bases=zb)
    cfl = d3.CFL(solver, initial_dt=0.01, cadence=1, safety=0.5)
    cfl.add_velocity(u)
    cfl.add_frequency(N)
    whole, _, shape1 = cfl._build_terms()
    cfl2 = d3.CFL(solver, initial_dt=0.01, cadence=1, safety=0.5)
    cfl2.add_velocity(u)
    cfl2.add_frequency(N)
    dist.size, dist.rank = 2, 1
    try:
        assert dist.shard_grid_axis == 1
        local, _, shape2 = cfl2._build_terms()
    finally:
        dist.size, dist.rank = 1, 0
    assert shape1 == (12, 24) and shape2 == (6, 24)
    assert [list(t["bcast"]) for t in local] == [[0, 0], [0, 1]]
    assert np.array_equal(np.asarray(local[0]["inv"][1]), np.asarray(whole[0]["inv"][1])[6:])
    assert np.array_equal(np.asarray(local[0]["inv"][0]), np.asarray(whole[0]["inv"][0]))


def test_shell_and_sphere_operands_describe_their_terms():
    import dedalus_amd.public as d3
    fake = FakeSumExecutor()
    solver, f = problems.shell_convection(d3, shape=(16, 12, 8), dist_kw=dict(executor=fake))
    u, b = f["u"], f["b"]
    dist = u.dist
    shell = b.basis
    phi, theta, r = dist.local_grids(shell)
    ug = np.zeros((3,) + np.broadcast(phi, theta, r).shape)
    ug[0] = 8.0 * np.sin(theta) * (r - 14) * (15 - r) * 4
    ug[2] = 3.0 * np.cos(theta) * (r - 14) * (15 - r) * 4 + 0 * phi
    u["g"] = ug
    Nr = dist.Field(name="Nr", bases=shell.radial_basis)
    Nr["g"] = 2.0 + (r - 14) ** 2
    cfl = d3.CFL(solver, initial_dt=0.006, cadence=1, safety=0.5)
    cfl.add_velocity(u)
    cfl.add_frequency(Nr)
    alone = u.cfl_frequency_max()
    solver.step(cfl.compute_timestep())
    (terms, shape), = fake.sum_calls
    assert shape == (24, 18, 12)
    assert [t["kind"] for t in terms] == ["shell", "scalar"] and [list(t["bcast"]) for t in terms] == [[0, 0, 0], [1, 1, 0]]
    prof = np.asarray(terms[1]["data"]).reshape(-1)
    rg = shell.radius_grid(1.5)
    assert prof.shape == (12,) and np.allclose(prof, 2.0 + (rg - 14) ** 2, rtol=1e-12)
    assert alone < cfl._max_freq <= alone + prof.max()
    # the sphere: an S2 vector is a velocity term with the one horizontal spacing R / sqrt(Lmax (Lmax + 1))
    fake2 = FakeSumExecutor()
    solver2, f2, _ = problems.shallow_water(d3, Nphi=16, Ntheta=8, dist_kw=dict(executor=fake2))
    cfl2 = d3.CFL(solver2, initial_dt=0.1, cadence=1, safety=0.5)
    cfl2.add_velocity(f2["u"])
    f2["u"].change_scales(1.5)
    g = np.array(f2["u"]["g"])                       # (the frequency is sampled at the start of the step)
    solver2.step(cfl2.compute_timestep())
    (terms2, shape2), = fake2.sum_calls
    assert shape2 == (24, 12) and [t["kind"] for t in terms2] == ["s2"] and list(terms2[0]["bcast"]) == [0, 0]
    basis = f2["u"].basis
    assert terms2[0]["inv_h"] == np.sqrt(6 * 7) / basis.radius
    want = (np.sqrt(g[0] ** 2 + g[1] ** 2) * terms2[0]["inv_h"]).max()
    assert abs(cfl2._max_freq - want) <= 1e-12 * want


@pytest.mark.parametrize("name", ["rb_sqrt", "rb_no_vertical_basis", "box_two_velocities", "shell_profile", "sphere_velocity"])
def test_host_layer_reproduces_the_reference_dt_sequence(name):
    """the adaptive runs of tests/cfl_terms_cases.py with the fake executor's float64 reduction: operands, spacings,
    scheduling and broadcasting are the reference's (tests/golden/cfl_terms.npz)"""
    import os
    import cfl_terms_cases as tc
    import dedalus_amd.public as d3
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cfl_terms.npz"))
    fake = FakeSumExecutor()
    solver, dts = tc.CASES[name](d3, dist_kw=dict(executor=fake))
    assert len(fake.sum_calls) == tc.STEPS and fake.single_calls == 0
    assert np.allclose(dts, gold[name], rtol=1e-11, atol=0), np.max(np.abs(dts - gold[name]) / gold[name])


@pytest.mark.parametrize("name,n", [c for c in cc.CASES if c[1] < 2000])
def test_expected_values_agree_with_float64(name, n):
    for plant in cc.PLANTS:
        terms, shape = cc.terms_of(name, n, plant)
        ref, at = cc.expected(terms, shape)
        f64 = cc.frequency_field(terms, shape, dtype=np.float64)
        assert abs(float(ref) - f64.max()) <= 8 * 3 * 2.0 ** -52 * f64.max()
        if plant != "none":
            assert at == (0 if plant == "first" else n - 1) and ref >= 500
        # broadcast operands really are small: one point along every flagged axis
        for t in terms:
            own = tuple(1 if b else m for m, b in zip(shape, t["bcast"]))
            assert t["data"].shape[1:] == own


def test_cases_reach_every_launch_shape_edge():
    assert set(cc.SIZES) >= {1, 255, 256, 257, cc.FULL - 1, cc.FULL, cc.FULL + 1, 315}
    assert {len(s) for s in cc.SHAPES.values()} == {1, 2, 3}
    terms, _ = cc.terms_of("eight", 315)
    assert len(terms) == cc.MAX_TERMS and {t["kind"] for t in terms} == {"velocity", "scalar", "shell", "s2"}
    assert any(None in t.get("comp_axis", []) for t in terms) and any(all(t["bcast"]) for t in terms)
