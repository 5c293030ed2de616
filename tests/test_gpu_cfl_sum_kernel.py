"""GPU: ddh_grid_cfl_sum (dedalus_amd/csrc/ddh_grid.hip) alone, through ctypes, against the longdouble values of
tests/cfl_sum_cases.py at the edges of its launch shape: n = 1, 255, 256, 257, 256 G - 1, 256 G, 256 G + 1 (G = the grid cap
of stream_grid) and 5 x 7 x 9, for every term list of the cases, with the maximum where the data puts it, in the first and
in the last grid point.

Bound (derived, not measured): every term is a sum of at most ncomp products of non-negative numbers (a square root of two
of them for the spherical kinds), the terms are added in list order, the maximum is exact: relative error <= nterms *
ncomp * u, u = 2^-53, ncomp = the largest component count in the list.  One velocity alone equals ddh_grid_cfl bit for bit.
Every input (operands, spacing arrays) lies between two guard regions of 64 NaNs: a read outside it makes the result NaN.
The result is one double in front of 64 NaNs that stay NaN."""
import ctypes as C
import math

import numpy as np
import pytest

import cfl_sum_cases as cc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ex():
    from dedalus_amd.executor import HipExecutor
    return HipExecutor()


def fenced(ex, a):
    """device copy of host array `a` with cc.GUARD NaNs in front of and behind it (the view keeps the buffer alive)"""
    a = np.ascontiguousarray(a, dtype=np.float64)
    host = np.full(a.size + 2 * cc.GUARD, np.nan)
    host[cc.GUARD:cc.GUARD + a.size] = a.reshape(-1)
    return ex.from_host(host)[cc.GUARD:cc.GUARD + a.size].reshape(a.shape)


def on_device(ex, terms):
    out = []
    for t in terms:
        d = dict(t, data=fenced(ex, t["data"]))
        if t["kind"] == "velocity":
            d["inv"] = [None if a is None else fenced(ex, a) for a in t["inv"]]
        elif t["kind"] == "shell":
            d["inv"] = tuple(fenced(ex, a) for a in t["inv"])
        out.append(d)
    return out


def cfl_sum(ex, terms_d, shape):
    """ex.cfl_sum_max's marshalling, into a guarded result"""
    from dedalus_amd import libhip
    from dedalus_amd.device import ptr
    buf = ex.dev.empty(1 + cc.GUARD)
    buf.fill_(float("nan"))
    arr = _marshal(terms_d)
    ln = (C.c_long * len(shape))(*[int(x) for x in shape])
    libhip.call("ddh_grid_cfl_sum", ptr(buf), len(terms_d), arr, int(np.prod(shape, dtype=np.int64)), ln, len(shape),
                ex.dev.stream)
    ex.sync()
    host = ex.download(buf)
    assert np.isnan(host[1:]).all(), "guard region overwritten"
    return float(host[0])


def _marshal(terms_d):
    from dedalus_amd import libhip
    kinds = dict(velocity=libhip.CFL_VELOCITY, scalar=libhip.CFL_SCALAR, shell=libhip.CFL_SHELL, s2=libhip.CFL_S2)
    arr = (libhip.CflTerm * max(len(terms_d), 1))()
    for t, d in zip(arr, terms_d):
        t.kind, t.data = kinds[d["kind"]], d["data"].data_ptr() if d["data"] is not None else None
        for ax, b in enumerate(d["bcast"]):
            t.bcast[ax] = int(b)
        if d["kind"] == "velocity":
            t.ncomp = len(d["comp_axis"])
            for c, (ax, inv) in enumerate(zip(d["comp_axis"], d["inv"])):
                t.comp_axis[c] = -1 if ax is None else int(ax)
                t.inv[c] = None if inv is None else inv.data_ptr()
        elif d["kind"] == "shell":
            t.inv[0], t.inv[1] = [None if a is None else a.data_ptr() for a in d["inv"]]
        elif d["kind"] == "s2":
            t.inv_h = d["inv_h"]
    return arr


@pytest.mark.parametrize("name,n", cc.CASES)
def test_cfl_sum(ex, name, n):
    for plant in cc.PLANTS:
        terms, shape = cc.terms_of(name, n, plant)
        ref, at = cc.expected(terms, shape)
        if plant != "none":
            assert at == (0 if plant == "first" else n - 1)
        terms_d = on_device(ex, terms)
        got = ex.cfl_sum_max(terms_d, shape)
        assert cfl_sum(ex, terms_d, shape) == got
        bound = len(terms) * cc.ncomp_of(terms) * cc.U
        r = float(abs(cc.LD(got) - ref) / (bound * ref))
        print("cfl_sum %s n=%d plant=%s got %.17g error/bound %.4f" % (name, n, plant, got, r))
        assert r <= 1.0, (plant, got, float(ref))
        if name == "one_velocity":
            t = terms_d[0]
            assert got == ex.cfl_max(t["data"], len(t["comp_axis"]), shape, t["inv"], t["comp_axis"])      # bit for bit


@pytest.mark.parametrize("name,n", cc.CASES)
def test_cfl_sum_nan_and_zero(ex, name, n):
    terms, shape = cc.terms_of(name, n)
    terms_d = on_device(ex, terms)
    last = terms_d[-1]["data"].reshape(-1)
    keep = float(terms[-1]["data"].reshape(-1)[-1])
    last[-1] = float("nan")                       # the last element of the last component of the last term
    assert math.isnan(ex.cfl_sum_max(terms_d, shape))
    last[-1] = keep
    assert not math.isnan(ex.cfl_sum_max(terms_d, shape))
    for t in terms_d:
        t["data"].zero_()
    got = cfl_sum(ex, terms_d, shape)
    assert got == 0.0 and not math.copysign(1.0, got) < 0


def test_cfl_sum_index_past_32_bits(ex):
    """n = 2^32 + 2^12 takes the 64-bit index decomposition; the operands are profiles, so nothing large is allocated:
    a velocity on (1, 1, 4096) whose frequency rises along the last axis, a profile along the first axis that peaks at
    its last point and a constant.  The sum at the last grid point is the maximum only if every index is right."""
    from dedalus_amd import libhip
    shape = (2 ** 8 + 1, 2 ** 12, 2 ** 12)
    n = int(np.prod(shape, dtype=np.int64))
    assert n >= 2 ** 32 and libhip.CFL_MAX_TERMS == cc.MAX_TERMS
    rng = np.random.default_rng(7)
    w = np.sort(rng.uniform(0.1, 1.0, shape[2]))
    p = np.sort(rng.uniform(0.1, 1.0, shape[0]))
    terms = [dict(kind="velocity", data=np.stack([0 * w, 0 * w, w]).reshape(3, 1, 1, -1), bcast=[1, 1, 0],
                  comp_axis=[None, None, 2], inv=[None, None, np.linspace(1.0, 2.0, shape[2])]),
             dict(kind="scalar", data=-p.reshape(1, -1, 1, 1), bcast=[0, 1, 1]),
             dict(kind="scalar", data=np.array([[[[0.25]]]]), bcast=[1, 1, 1])]
    ref = cc.LD(w[-1]) * cc.LD(2.0) + cc.LD(p[-1]) + cc.LD(0.25)
    got = ex.cfl_sum_max(on_device(ex, terms), shape)
    assert abs(cc.LD(got) - ref) <= 3 * 3 * cc.U * ref, (got, float(ref))


def test_cfl_sum_rejections_launch_nothing(ex):
    """9 terms, axis lengths that do not multiply to n, a velocity (each kind) broadcast along every axis and null
    pointers: each is an error returned before the launch"""
    from dedalus_amd import libhip
    from dedalus_amd.device import ptr
    terms, shape = cc.terms_of("two_velocities_scalar", 255)
    terms_d = on_device(ex, terms)
    with pytest.raises(libhip.DdhError):
        ex.cfl_sum_max([terms_d[2]] * (cc.MAX_TERMS + 1), shape)
    with pytest.raises(libhip.DdhError):
        ex.cfl_sum_max([], shape)
    assert ex.cfl_sum_max([terms_d[2]] * cc.MAX_TERMS, shape) > 0
    buf = ex.dev.empty(1 + cc.GUARD)
    buf.fill_(float("nan"))
    ln = (C.c_long * 2)(*shape)

    def call(td, n=255, res=buf, lens=ln, naxes=2):
        libhip.call("ddh_grid_cfl_sum", None if res is None else ptr(res), len(td), _marshal(td), n, lens, naxes, ex.dev.stream)

    with pytest.raises(libhip.DdhError):
        call(terms_d, n=256)
    for kind in ("velocity", "shell", "s2"):
        src = dict(velocity=terms_d[0], shell=on_device(ex, cc.terms_of("shell_profile", 255)[0])[0],
                   s2=on_device(ex, cc.terms_of("s2_scalar", 255)[0])[0])[kind]
        with pytest.raises(libhip.DdhError):
            call([dict(src, bcast=[1, 1])])
    with pytest.raises(libhip.DdhError):
        call(terms_d, res=None)
    with pytest.raises(libhip.DdhError):
        call(terms_d, lens=None)
    with pytest.raises(libhip.DdhError):
        call([dict(terms_d[2], data=None)])
    with pytest.raises(libhip.DdhError):
        call([dict(terms_d[0], inv=[terms_d[0]["inv"][0], None])])
    with pytest.raises(libhip.DdhError):
        call([dict(terms_d[0], comp_axis=[0, 2])])
    with pytest.raises(libhip.DdhError):
        libhip.call("ddh_grid_cfl_sum", ptr(buf), 1, None, 255, ln, 2, ex.dev.stream)
    ex.sync()
    assert np.isnan(ex.download(buf)).all()                               # nothing was written
