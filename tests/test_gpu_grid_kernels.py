"""GPU: the streaming grid kernels of dedalus_amd/csrc/ddh_grid.hip against the longdouble references of
tests/grid_cases.py at the edges of their launch shapes (tests/test_grid_cases_host.py proves the tables reach them).

Bounds are derived, not measured: u = 2^-53, sums are sequential with or without FMA contraction.
  lincomb        |got - ref| <= (nterms + 1) u sum_t |alpha_t x_t|
  bilinear       |got - ref| <= (k + 2) u sum |coef a b| over the k terms of that output; an output without terms is 0.0
  cfl_max        relative error <= 4 u (a sum of at most three products; max is exact)
  cfl_spherical  relative error <= 6 u (one sqrt of a two-term sum, one more product, one add)
  scatter, pack / unpack: bit for bit
Every output buffer carries 64 guard doubles past its end, NaN before the call and still NaN after it; the payload is
NaN-filled too and holds no NaN afterwards.  With DDH_GRID_PARITY_OUT=<file> the worst error / bound ratio per kernel
and class is written there (profiles/grid_kernel_parity.txt)."""
import ctypes as C
import math
import os
import time

import numpy as np
import pytest

import cfl_nan_checks
import grid_cases as gc

pytestmark = pytest.mark.gpu

RATIOS = {}            # (kernel, class) -> worst error / bound
T0 = time.time()


def note(kernel, cls, ratio):
    key = (kernel, " ".join(cls) if isinstance(cls, tuple) else str(cls))
    RATIOS[key] = max(RATIOS.get(key, 0.0), float(ratio))


@pytest.fixture(scope="module", autouse=True)
def parity_record():
    yield
    path = os.environ.get("DDH_GRID_PARITY_OUT")
    if path:
        with open(path, "w") as fh:
            fh.write("# worst |error| / bound per kernel and launch-shape class (tests/test_gpu_grid_kernels.py); 0 = bit for bit\n")
            for (kernel, cls), r in sorted(RATIOS.items()):
                fh.write("%-22s %-70s %.4f\n" % (kernel, cls, r))
            fh.write("# wall time of the module: %.1f s\n" % (time.time() - T0))


@pytest.fixture(scope="module")
def ex():
    from dedalus_amd.executor import HipExecutor
    return HipExecutor()


def guarded(ex, n):
    """-> (buffer of n + GUARD doubles, all NaN; view of its first n)"""
    buf = ex.dev.empty(n + gc.GUARD)
    buf.fill_(float("nan"))
    return buf, buf[:n]


def payload(ex, buf, n, nan_ok=False):
    ex.sync()
    host = ex.download(buf)
    assert host.size == n + gc.GUARD and np.isnan(host[n:]).all(), "guard region overwritten"
    assert nan_ok or not np.isnan(host[:n]).any(), "payload entries left unwritten"
    return host[:n]


def ratio(got, ref, bound):
    """worst |got - ref| / bound; entries with a zero bound must be exact"""
    err = np.abs(np.asarray(got, dtype=gc.LD) - ref)
    zero = bound == 0
    assert np.all(err[zero] == 0)
    return float(np.max(err[~zero] / bound[~zero])) if np.any(~zero) else 0.0


# ---- lincomb ----------------------------------------------------------------------------------------------------------
def _lincomb_call(ex, y, ops, al):
    from dedalus_amd import libhip
    from dedalus_amd.device import ptr
    arr = (C.c_void_p * max(len(ops), 1))(*[C.c_void_p(x.data_ptr()) for x in ops])
    a = np.ascontiguousarray(al, dtype=np.float64)
    libhip.call("ddh_lincomb", ptr(y), len(ops), arr, libhip.as_dp(a), y.numel(), ex.dev.stream)


@pytest.mark.parametrize("nterms,n", gc.LINCOMB_CASES)
def test_lincomb(ex, nterms, n):
    xs, al = gc.lincomb_inputs(nterms, n)
    ref, mag = gc.lincomb(xs, al)
    buf, y = guarded(ex, n)
    ex.lincomb(y, [ex.from_host(x) for x in xs], al)
    got = payload(ex, buf, n)
    r = ratio(got, ref, (nterms + 1) * gc.U * mag)
    print("lincomb nterms=%d n=%d error/bound %.4f" % (nterms, n, r))
    note("lincomb", gc.stream_tags(n), r)
    assert r <= 1.0


def test_lincomb_output_is_its_own_first_operand(ex):
    nterms, n = gc.LINCOMB_ALIAS_CASE
    xs, al = gc.lincomb_inputs(nterms, n)
    ref, mag = gc.lincomb(xs, al)
    buf, y = guarded(ex, n)
    ex.upload(y, xs[0])
    ex.lincomb(y, [y] + [ex.from_host(x) for x in xs[1:]], al)
    r = ratio(payload(ex, buf, n), ref, (nterms + 1) * gc.U * mag)
    print("lincomb aliased error/bound %.4f" % r)
    note("lincomb", gc.stream_tags(n) + ("y_is_x0",), r)
    assert r <= 1.0


def test_lincomb_rejections_launch_nothing(ex):
    """0 and 17 terms and an operand 8 bytes off a 16-byte boundary are refused by ddh_lincomb before its launch"""
    from dedalus_amd import libhip
    n = 1000
    buf, y = guarded(ex, n)
    x = ex.from_host(np.ones(n + 2))
    with pytest.raises(libhip.DdhError):
        _lincomb_call(ex, y, [], [])
    with pytest.raises(libhip.DdhError):
        _lincomb_call(ex, y, [x[:n]] * (gc.LINCOMB_MAX_TERMS + 1), np.ones(gc.LINCOMB_MAX_TERMS + 1))
    assert x[1:n + 1].data_ptr() % 16 == 8
    with pytest.raises(libhip.DdhError):
        _lincomb_call(ex, y, [x[:n], x[1:n + 1]], [1.0, 2.0])
    with pytest.raises(libhip.DdhError):
        _lincomb_call(ex, buf[1:n + 1], [x[:n]], [1.0])                  # the output 8 bytes off
    ex.sync()
    assert np.isnan(ex.download(buf)).all()                               # nothing was written
    _lincomb_call(ex, y, [x[:n]] * gc.LINCOMB_MAX_TERMS, np.ones(gc.LINCOMB_MAX_TERMS))
    assert np.array_equal(payload(ex, buf, n), np.full(n, 16.0))


# ---- bilinear ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", gc.BILINEAR_CASES)
def test_bilinear(ex, name, n):
    ncomp_out, na, nb, terms = gc.BILINEAR_TABLES[name]
    a, b = gc.bilinear_inputs(name, n)
    ref, mag, count = gc.bilinear(ncomp_out, a, b, n, terms)
    buf, out = guarded(ex, ncomp_out * n)
    ex.bilinear(out, ncomp_out, ex.from_host(a), ex.from_host(b), n, terms)
    got = payload(ex, buf, ncomp_out * n).reshape(ncomp_out, n)
    worst = 0.0
    for c in range(ncomp_out):
        if count[c] == 0:
            assert np.all(got[c] == 0.0) and not np.signbit(got[c]).any(), "an output without terms must be +0.0"
            continue
        worst = max(worst, ratio(got[c], ref[c], (count[c] + 2) * gc.U * mag[c]))
    print("bilinear %s n=%d error/bound %.4f" % (name, n, worst))
    note("bilinear<%d>" % (1 if ncomp_out <= 1 else 3 if ncomp_out <= 3 else 9), gc.stream_tags(n), worst)
    assert worst <= 1.0


def test_bilinear_rejections_launch_nothing(ex):
    """33 terms, 10 outputs, an output index out of range and an odd point count with two components: each is an error
    returned by ddh_grid_bilinear before its launch"""
    from dedalus_amd import libhip
    n = 512
    buf, out = guarded(ex, 10 * n)
    a, b = ex.from_host(np.ones((3, n))), ex.from_host(np.ones((3, n)))
    ok = [(0, 0, 0, 1.0)]
    with pytest.raises(libhip.DdhError):
        ex.bilinear(out, 1, a, b, n, ok * (gc.BILINEAR_MAX_TERMS + 1))
    with pytest.raises(libhip.DdhError):
        ex.bilinear(out, gc.BILINEAR_MAX_OUT + 1, a, b, n, ok)
    for bad in (3, -1):
        with pytest.raises(libhip.DdhError):
            ex.bilinear(out, 3, a, b, n, [(0, 0, 0, 1.0), (bad, 1, 1, 1.0)])
    with pytest.raises(libhip.DdhError):
        ex.bilinear(out, 2, a, b, n - 1, [(0, 0, 0, 1.0), (1, 0, 0, 1.0)])          # odd n, two outputs
    with pytest.raises(libhip.DdhError):
        ex.bilinear(out, 1, a, b, n - 1, [(0, 1, 0, 1.0)])                          # odd n, second operand component
    ex.sync()
    assert np.isnan(ex.download(buf)).all()


# ---- Cartesian CFL ----------------------------------------------------------------------------------------------------
def _cfl_direct(ex, u_d, ncomp, shape, inv_d, comp_axis):
    """ddh_grid_cfl into a guarded result buffer"""
    from dedalus_amd import libhip
    from dedalus_amd.device import ptr
    buf, res = guarded(ex, 1)
    arr = (C.c_void_p * ncomp)(*[C.c_void_p(a.data_ptr()) for a in inv_d])
    ca = np.ascontiguousarray(comp_axis, dtype=np.int32)
    ln = (C.c_long * len(shape))(*[int(x) for x in shape])
    libhip.call("ddh_grid_cfl", ptr(res), ptr(u_d), ncomp, int(np.prod(shape)), arr, libhip.as_ip(ca), ln, len(shape),
                ex.dev.stream)
    return float(payload(ex, buf, 1, nan_ok=True)[0])


@pytest.mark.parametrize("name", list(gc.CFL_CASES))
def test_cfl_max(ex, name):
    shape, comp_axis, _, tags = gc.CFL_CASES[name]
    ncomp = len(comp_axis)
    for plant in gc.PLANTS:
        u, inv, at = gc.cfl_inputs(name, plant)
        if plant != "none" and at is None:
            continue
        ref = gc.cfl_max(u, ncomp, shape, inv, comp_axis)
        u_d, inv_d = ex.from_host(u), [ex.from_host(a) for a in inv]
        got = ex.cfl_max(u_d, ncomp, shape, inv_d, comp_axis)
        assert _cfl_direct(ex, u_d, ncomp, shape, inv_d, comp_axis) == got
        r = float(abs(gc.LD(got) - ref) / (4 * gc.U * ref))
        print("cfl_max %s plant=%s got %.17g error/bound %.4f" % (name, plant, got, r))
        note("cfl_max", tuple(sorted(tags)) + ("plant_" + plant,), r)
        assert r <= 1.0, (plant, got, float(ref))
    z = ex.zeros((ncomp, int(np.prod(shape))))
    got = ex.cfl_max(z, ncomp, shape, inv_d, comp_axis)
    assert got == 0.0 and not math.copysign(1.0, got) < 0
    z.fill_(-0.0)
    assert ex.cfl_max(z, ncomp, shape, inv_d, comp_axis) == 0.0


@pytest.mark.parametrize("name", list(gc.CFL_CASES))
def test_cfl_max_returns_nan_for_a_nan_velocity(ex, name):
    shape, comp_axis, _, _ = gc.CFL_CASES[name]
    ncomp = len(comp_axis)
    u, inv, _ = gc.cfl_inputs(name)
    u_d, inv_d = ex.from_host(u), [ex.from_host(a) for a in inv]
    finite = ex.cfl_max(u_d, ncomp, shape, inv_d, comp_axis)
    for where in gc.NAN_PLANTS:
        at = gc.nan_index(shape, where)
        for comp in range(ncomp):
            u_d[comp, at] = float("nan")
            assert math.isnan(ex.cfl_max(u_d, ncomp, shape, inv_d, comp_axis)), (where, comp)
            assert math.isnan(_cfl_direct(ex, u_d, ncomp, shape, inv_d, comp_axis))
            u_d[comp, at] = float(u[comp, at])
    assert ex.cfl_max(u_d, ncomp, shape, inv_d, comp_axis) == finite       # restored
    u_d.fill_(float("nan"))
    assert math.isnan(ex.cfl_max(u_d, ncomp, shape, inv_d, comp_axis))    # all NaN: NaN, not 0


# ---- spherical CFL ----------------------------------------------------------------------------------------------------
def _sph_direct(ex, u_d, inv_h_d, inv_dr_d):
    from dedalus_amd import libhip
    from dedalus_amd.device import ptr
    buf, res = guarded(ex, 1)
    libhip.call("ddh_grid_cfl_spherical", ptr(res), ptr(u_d), int(u_d.shape[1]) * int(u_d.shape[2]), int(u_d.shape[3]),
                ptr(inv_h_d), ptr(inv_dr_d), ex.dev.stream)
    return float(payload(ex, buf, 1, nan_ok=True)[0])


@pytest.mark.parametrize("name", list(gc.SPH_CASES))
def test_cfl_max_spherical(ex, name):
    shape, zero_h, tags = gc.SPH_CASES[name]
    for plant in gc.SPH_PLANTS:
        u, inv_h, inv_dr, at = gc.sph_inputs(name, plant)
        if plant != "none" and at is None:
            continue
        ref = gc.cfl_max_spherical(u, inv_h, inv_dr)
        u_d, h_d, dr_d = ex.from_host(u), ex.from_host(inv_h), ex.from_host(inv_dr)
        got = ex.cfl_max_spherical(u_d, h_d, dr_d)
        assert _sph_direct(ex, u_d, h_d, dr_d) == got
        r = float(abs(gc.LD(got) - ref) / (6 * gc.U * ref))
        print("cfl_max_spherical %s plant=%s got %.17g error/bound %.4f" % (name, plant, got, r))
        note("cfl_max_spherical", tuple(sorted(tags)) + ("plant_" + plant,), r)
        assert r <= 1.0, (plant, got, float(ref))
    u_d.zero_()
    assert ex.cfl_max_spherical(u_d, h_d, dr_d) == 0.0


@pytest.mark.parametrize("name", list(gc.SPH_CASES))
def test_cfl_max_spherical_returns_nan_for_a_nan_velocity(ex, name):
    shape = gc.SPH_CASES[name][0]
    u, inv_h, inv_dr, _ = gc.sph_inputs(name)
    u_d, h_d, dr_d = ex.from_host(u), ex.from_host(inv_h), ex.from_host(inv_dr)
    flat = u_d.reshape(3, -1)
    finite = ex.cfl_max_spherical(u_d, h_d, dr_d)
    for where in gc.NAN_PLANTS:
        at = gc.nan_index(shape, where)
        for comp in range(3):
            keep = float(u.reshape(3, -1)[comp, at])
            flat[comp, at] = float("nan")
            assert math.isnan(ex.cfl_max_spherical(u_d, h_d, dr_d)), (where, comp)
            assert math.isnan(_sph_direct(ex, u_d, h_d, dr_d))
            flat[comp, at] = keep
    assert ex.cfl_max_spherical(u_d, h_d, dr_d) == finite
    u_d.fill_(float("nan"))
    assert math.isnan(ex.cfl_max_spherical(u_d, h_d, dr_d))


# ---- the NaN policy at the level of the CFL class ---------------------------------------------------------------------
def test_nan_velocity_leaves_the_timestep_unchanged_on_the_device():
    import dedalus_amd.public as d3
    solver = cfl_nan_checks.nan_velocity_leaves_dt_unchanged(d3)
    assert solver.ex.name == "hip"


def test_nan_shell_velocity_gives_a_nan_frequency_and_an_unchanged_timestep():
    import dedalus_amd.public as d3
    solver = cfl_nan_checks.nan_shell_velocity_leaves_dt_unchanged(d3)
    assert solver.ex.name == "hip"


# ---- scatter ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", gc.SCATTER_SIZES)
@pytest.mark.parametrize("op", ["scatter_add", "scatter_set"])
def test_scatter_with_unique_indices(ex, op, n):
    y, idx, vals = gc.scatter_inputs(n)
    ref = getattr(gc, op)(y, idx, vals)
    buf, y_d = guarded(ex, y.size)
    ex.upload(y_d, y)
    getattr(ex, op)(y_d, ex.make_scatter(idx, vals))
    got = payload(ex, buf, y.size)
    assert np.array_equal(got[idx], ref[idx])
    untouched = np.ones(y.size, bool)
    untouched[idx] = False
    assert np.array_equal(got[untouched].view(np.uint64), y[untouched].view(np.uint64))
    note(op, gc.scatter_tags(n), 0.0)


@pytest.mark.parametrize("op", ["scatter_add", "scatter_set"])
def test_scatter_of_nothing_is_a_no_op(ex, op):
    y = np.random.default_rng(0).standard_normal(100)
    buf, y_d = guarded(ex, y.size)
    ex.upload(y_d, y)
    getattr(ex, op)(y_d, ex.make_scatter(np.zeros(0, np.int64), np.zeros(0)))
    assert np.array_equal(payload(ex, buf, y.size).view(np.uint64), y.view(np.uint64))


# ---- pack / unpack ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(gc.PACK_CASES))
def test_pack_unpack(ex, name):
    from dedalus_amd import libhip
    from dedalus_amd.device import ptr
    kind, dims, tags = gc.PACK_CASES[name]
    src = gc.pack_input(kind, dims)
    n_out = gc.pack_geometry(kind, dims)[4]
    d_src = ex.from_host(src)
    buf, dst = guarded(ex, n_out)
    if kind in ("a2a_pack", "a2a_unpack"):
        getattr(ex, kind)(d_src, dst, *dims)
    else:
        libhip.call("ddh_%s_b" % kind, ptr(d_src), ptr(dst), *dims, ex.dev.stream)
    got = payload(ex, buf, n_out)
    del d_src, buf, dst
    ref = gc.pack_reference(kind, src, dims)
    assert np.array_equal(got, ref)
    note(kind, tags, 0.0)
