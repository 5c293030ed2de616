"""CPU: the pointwise map / broadcast kernels build and are exported, their op table is the reference's ufunc table, no
instantiation spills, the case tables of tests/grid_map_cases.py are what they claim, and expressions with grid functions
still evaluate on an executor that has no grid_map (the NumPy oracle)."""
import numpy as np

import grid_map_cases as mc
from test_kernel_resources import _usage


def test_library_exports_the_map_entry_points():
    from dedalus_amd import build, libhip
    build.build_library()
    lib = libhip.load()
    for name in ("ddh_grid_map", "ddh_grid_broadcast", "ddh_grid_map_launches"):
        assert hasattr(lib, name) and name in libhip.SIGNATURES, name


def test_op_table_is_the_reference_ufuncs_plus_recip_and_pow():
    from dedalus_amd.executor import HipExecutor
    assert len(mc.UFUNCS) == 21 and all(isinstance(getattr(np, u), np.ufunc) for u in mc.UFUNCS)
    assert set(HipExecutor.MAP_OPS) == set(mc.UFUNCS) | {"recip", "pow"}
    assert sorted(HipExecutor.MAP_OPS.values()) == list(range(23))
    assert all(getattr(np, u).__name__ == u for u in mc.UFUNCS)
    assert np.abs.__name__ == "absolute"


def test_no_map_instantiation_uses_scratch():
    """one instantiation per op (23 and the repeated-multiplication power), none with scratch memory, and the cheap ones
    without the register footprint of the transcendental ones"""
    u = _usage("ddh_gridmap.hip")
    maps = {k: v for k, v in u.items() if "map_kernel" in k}
    assert len(maps) == 24, sorted(maps)
    for k, v in list(maps.items()) + [(k, v) for k, v in u.items() if "broadcast_kernel" in k]:
        print(k, v)
        assert v["scratch"] == 0, (k, v)
    from dedalus_amd.executor import HipExecutor
    inst = lambda name: maps["_ZN3ddh10map_kernelILi%dEEEvPdPKdldii" % HipExecutor.MAP_OPS[name]]
    for cheap in ("absolute", "sqrt", "recip"):
        assert inst(cheap)["vgprs"] < inst("tan")["vgprs"], (cheap, inst(cheap), inst("tan"))


def test_inputs_stay_inside_each_domain_and_bounds_name_every_function():
    for op in mc.OPS:
        for n in (1, 255, 100003):
            x = mc.map_input(op, n)
            assert x.dtype == np.float64 and x.shape == (n,) and np.isfinite(x).all()
            assert np.array_equal(x, mc.map_input(op, n))                   # seeded
            ref = mc.reference(op, x, 2.5)
            assert ref.dtype == mc.LD and np.isfinite(ref).all(), op
    lim = {"exp": 20, "sinh": 20, "cosh": 20, "sin": 100, "cos": 100, "tan": 100, "arcsin": 1, "arccos": 1}
    for op, m in lim.items():
        assert np.abs(mc.map_input(op, 100003)).max() <= m
    for op in ("log", "log2", "log10", "sqrt"):
        x = mc.map_input(op, 100003)
        assert x.min() > 0 and x.max() <= 1e6
    x = mc.map_input("arccosh", 100003)
    assert x.min() >= 1 and x.max() <= 1e6
    assert np.abs(mc.map_input("arctanh", 100003)).max() < 1
    assert (mc.map_input("pow", 100003, "signed", 3) < 0).any() and (mc.map_input("pow", 100003, "positive", 3) > 0).all()
    measured = set(mc.OPS) - set(mc.EXACT)
    assert set(mc.BOUNDS) == measured, set(mc.BOUNDS) ^ measured
    assert all(float(b) == int(b) and b >= 2 for b in mc.BOUNDS.values())
    assert [mc.powi_bound(p) for p in (3, -2, 2, -1)] == [2, 2, 1, 1]
    assert mc.pow_is_repeated_multiplication(3) and mc.pow_is_repeated_multiplication(-2)
    assert not any(mc.pow_is_repeated_multiplication(p) for p in (2.5, -0.5, 0.5, -1, 0, 9))
    assert [mc.stream_tags(n) for n in mc.SIZES] == [mc.gc.LINCOMB_TAGS[n] for n in mc.SIZES]
    first, mid, last = mc.special_positions()
    assert first == 0 and last == mc.SPECIAL_N - 6 and mid // 2 >= 2 * mc.gc.STREAM_PASS and mid + 6 < last
    assert len(mc.BROADCAST_MASKS) == 7 and len(mc.BROADCAST_CASES) == 4 * 7 * 2


def _fields(d3, executor):
    coords = d3.CartesianCoordinates("x", "z")
    dist = d3.Distributor(coords, dtype=np.float64, executor=executor)
    xb = d3.RealFourier(coords["x"], size=16, bounds=(0, 2 * np.pi), dealias=3 / 2)
    zb = d3.ChebyshevT(coords["z"], size=12, bounds=(0, 1), dealias=3 / 2)
    b = dist.Field(name="b", bases=(xb, zb))
    x, z = dist.local_grids(xb, zb)
    b["g"] = 2.0 + 0.5 * np.sin(x) * z + 0.25 * np.cos(2 * x) * (1 - z * z)
    N2 = dist.Field(name="N2", bases=zb)
    N2["g"] = 1.0 + z ** 2
    return b, N2


def test_grid_functions_still_evaluate_on_an_executor_without_grid_map():
    import dedalus_amd.public as d3
    from oracle.np_executor import NumpyExecutor
    ex = NumpyExecutor()
    assert getattr(ex, "grid_map", None) is None and getattr(ex, "grid_broadcast", None) is None
    b, N2 = _fields(d3, ex)
    b.change_scales(3 / 2)
    bg = np.array(b["g"])
    for expr, ref in ((np.sqrt(b), np.sqrt(bg)), (b ** 3, bg ** 3), (b ** (-1), 1 / bg)):
        out = expr.evaluate()
        out.change_scales(3 / 2)
        assert np.allclose(np.array(out["g"]), ref, rtol=1e-13, atol=0)
    N2.change_scales(3 / 2)
    out = (N2 * b).evaluate()
    out.change_scales(3 / 2)
    assert np.allclose(np.array(out["g"]), np.array(N2["g"]) * bg, rtol=1e-13, atol=0)


def test_unknown_grid_function_is_named():
    from dedalus_amd.core.evaluator import Evaluator
    assert Evaluator._map_op(np.abs) == "absolute" and Evaluator._map_op(np.arctanh) == "arctanh"
    for func in (np.cbrt, np.negative, lambda x: x, np.reciprocal):
        try:
            Evaluator._map_op(func)
        except NotImplementedError as e:
            assert getattr(func, "__name__", "lambda") in str(e) or "lambda" in str(e)
        else:
            raise AssertionError("accepted %r" % (func,))
