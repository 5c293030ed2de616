"""GPU: the size-generic workgroup transform kernel (fft_axis_kernel) at its radix and launch-shape edges, through the C
ABI (cases, shapes and references: tests/transform_edge_cases.py; CPU twin: tests/test_transform_edge_cases_host.py).

Every launch first asserts, through ddh_fft_plan_info, that the library plans the workgroup kernel with the B, block size,
grid and dynamic LDS the Python mirror of the planner gives, and the mirror gives the row what it was put in the table to
hit (host test).  The destination is the interior of a larger device buffer: 64 sentinel doubles on each side, NaN inside.
After the call both guards are untouched, the interior is finite, the source is bit-identical to its upload and
ddh_fft_wave_launches has not moved.  Per-line rel-L2 against the longdouble matrix reference: every line up to 512 points,
the first and the last line above, where every line is also held against oracle/np_transforms.py (itself within a tenth of
the bound of the longdouble reference, host test).  Bounds: 1e-12, 1e-11 for a backward transform through a conversion
solve.  The dual entry points equal the two single launches."""
import ctypes as C

import numpy as np
import pytest

import transform_edge_cases as tc

pytestmark = pytest.mark.gpu

MODE = {("rfft", True): 0, ("rfft", False): 1, ("cheb", True): 2, ("cheb", False): 3, ("cfft", True): 4, ("cfft", False): 5}
INFO_KEYS = ("kernel", "B", "T", "grid", "lds")
WORKGROUP = 3


@pytest.fixture(scope="module")
def dev():
    from dedalus_amd.device import Device
    return Device.get()


def _make_plan(kind, N, M, alpha):
    from dedalus_amd import libhip
    h = C.c_uint64(0)
    if kind == "rfft":
        libhip.call("ddh_plan_rfft", C.byref(h), N, M)
    elif kind == "cfft":
        libhip.call("ddh_plan_cfft", C.byref(h), N, M)
    else:
        _, offs, bands = tc.conversion(M, alpha)
        if offs is None:
            libhip.call("ddh_plan_cheb", C.byref(h), N, M, 0, None, None)
        else:
            libhip.call("ddh_plan_cheb", C.byref(h), N, M, len(offs), libhip.as_ip(offs), libhip.as_dp(bands))
    return h


def _plan_info(plan, kind, op, outer, inner):
    from dedalus_amd import libhip
    info = (C.c_int * 5)(*([-1] * 5))
    dual = op == "backward_dual"
    libhip.call("ddh_fft_plan_info", plan, MODE[(kind, op == "forward")], outer, inner, int(dual),
                int(op == "backward_deriv"), int(dual and kind == "cheb"), info)
    return dict(zip(INFO_KEYS, list(info)))


def _wave_launches():
    from dedalus_amd import libhip
    n = C.c_long(-1)
    libhip.call("ddh_fft_wave_launches", C.byref(n))
    return n.value


class Guarded:
    """a destination of n doubles inside a buffer with GUARD sentinel doubles on each side, NaN inside"""

    def __init__(self, dev, n):
        self.dev, self.n = dev, n
        self.buf = dev.empty(n + 2 * tc.GUARD)
        self.buf.fill_(tc.SENTINEL)
        self.view = self.buf[tc.GUARD:tc.GUARD + n]
        self.view.fill_(float("nan"))

    def ptr(self):
        from dedalus_amd.device import ptr
        return ptr(self.view)

    def fetch(self):
        """(interior, guards intact)"""
        h = self.dev.to_host(self.buf)
        intact = bool((h[:tc.GUARD] == tc.SENTINEL).all() and (h[tc.GUARD + self.n:] == tc.SENTINEL).all())
        return h[tc.GUARD:tc.GUARD + self.n], intact


def _launch(dev, c, plan, op, x, dsts, dvec=None):
    from dedalus_amd import libhip
    from dedalus_amd.device import ptr
    outer, inner = tc.outer_inner(x.shape)
    d_x = dev.from_host(x)
    name = "ddh_%s_%s" % (c.kind, op)
    if op == "backward_deriv":
        libhip.call(name, plan, ptr(d_x), dsts[0].ptr(), outer, inner, tc.DSCALE, dev.stream)
    elif op == "backward_dual" and c.kind == "rfft":
        libhip.call(name, plan, ptr(d_x), dsts[0].ptr(), dsts[1].ptr(), outer, inner, tc.DSCALE, dev.stream)
    elif op == "backward_dual":
        libhip.call(name, plan, ptr(d_x), dsts[0].ptr(), dsts[1].ptr(), ptr(dvec), outer, inner, dev.stream)
    else:
        libhip.call(name, plan, ptr(d_x), dsts[0].ptr(), outer, inner, dev.stream)
    dev.sync()
    assert np.array_equal(dev.to_host(d_x), x), "the source array changed"


def _run(dev, c, plan, op, x, shape, dvec=None):
    """one entry point on one array, all the assertions that need no reference; returns the outputs (host arrays)"""
    outer, inner = tc.outer_inner(shape)
    cx = 2 if c.kind == "cfft" else 1
    n_out = tc.out_axis(c, op)
    out_shape = (shape[0], n_out) + tuple(shape[2:])
    nout = 2 if op == "backward_dual" else 1
    want = tc.plan_mirror(c.kind, c.N, outer, inner)
    info = _plan_info(plan, c.kind, op, outer, inner)
    print("%s %s %s plan_info %s" % (tc.case_id(c), op, shape, info))
    assert info == dict(kernel=WORKGROUP, B=want["B"], T=want["T"], grid=want["grid"], lds=want["lds"]), (info, want)
    dsts = [Guarded(dev, outer * inner * n_out * cx) for _ in range(nout)]
    before = _wave_launches()
    _launch(dev, c, plan, op, x, dsts, dvec)
    assert _wave_launches() == before, "a wave kernel took a size that has none"
    outs = []
    for d in dsts:
        got, intact = d.fetch()
        assert intact, "a store outside the destination array"
        assert np.isfinite(got).all(), "destination elements not written (or not finite)"
        if cx == 2:
            got = got.view(np.complex128)
        outs.append(got.reshape(out_shape))
    return outs


@pytest.mark.parametrize("case", tc.CASES, ids=tc.CASE_IDS)
def test_workgroup_kernel_at_its_edges(dev, case):
    c = case
    plan = _make_plan(c.kind, c.N, c.M, c.alpha)
    plan0 = _make_plan("cheb", c.N, c.M, 0) if c.ops == ("backward_dual",) else None
    dvec = dev.from_host(tc.dual_dvec(c.M)) if plan0 is not None else None
    runs = []
    for shape in tc.shapes_for(c.N):
        for op in c.ops:
            x = tc.make_input(c, op, shape)
            outs = _run(dev, c, plan, op, x, shape, dvec)
            if c.kind == "rfft" and op == "backward_dual":
                # the same coefficients through the two single launches: bit for bit the dual's outputs
                for single, got in zip(("backward", "backward_deriv"), outs):
                    assert np.array_equal(_run(dev, c, plan, single, x, shape)[0], got), (shape, single)
            if c.kind == "cheb" and op == "backward_dual":
                assert np.array_equal(_run(dev, c, plan0, "backward", x, shape)[0], outs[0]), shape
                dc = np.ascontiguousarray(np.moveaxis(tc.derivative_coeffs(np.moveaxis(x, 1, 0)), 0, 1))
                gd1 = _run(dev, c, plan, "backward", dc, shape)[0]
                e = np.linalg.norm(outs[1] - gd1) / np.linalg.norm(gd1)
                print("%s %s dual derivative vs single launch %.3e" % (tc.case_id(c), shape, e))
                assert e < 1e-14, (shape, e)
            xl = tc.lines_of(x, c.N if op == "forward" else c.M)
            runs.append((op, shape, x, outs, tc.compared_lines(c.N, xl.shape[1]), xl))
    refs_all = tc.reference_many(c, [(op, xl[:, pick]) for op, _, _, _, pick, xl in runs])
    worst = {}
    failures = []
    for (op, shape, x, outs, pick, _), refs in zip(runs, refs_all):
        tols = tc.tolerances(c, op)
        for i, (got, ref, tol) in enumerate(zip(outs, refs, tols)):
            err = tc.line_errors(tc.lines_of(got, tc.out_axis(c, op))[:, pick], ref).max()
            worst[(op, i)] = max(worst.get((op, i), 0.0), err)
            if not err < tol:
                failures.append((op, i, shape, "longdouble", err, tol))
        if c.N > tc.BIG:
            for i, (got, ref, tol) in enumerate(zip(outs, tc.oracle(c, op, x), tols)):
                n = tc.out_axis(c, op)
                err = tc.line_errors(tc.lines_of(got, n), tc.lines_of(ref, n).astype(got.dtype)).max()
                worst[(op, i, "oracle")] = max(worst.get((op, i, "oracle"), 0.0), err)
                if not err < tol:
                    failures.append((op, i, shape, "oracle", err, tol))
    for key, err in sorted(worst.items(), key=str):
        print("%s %s worst line rel-L2 %.3e" % (tc.case_id(c), key, err))
    from dedalus_amd import libhip
    for h in (plan, plan0):
        if h is not None:
            libhip.call("ddh_destroy", h)
    assert not failures, failures


@pytest.mark.parametrize("kind,N,M,alpha,text", tc.PLAN_REFUSALS)
def test_plan_refusals(dev, kind, N, M, alpha, text):
    from dedalus_amd import libhip
    before = _wave_launches()
    with pytest.raises(libhip.DdhError, match=text):
        _make_plan(kind, N, M, alpha)
    assert _wave_launches() == before


def _assert_refused(dev, kind, N, M, text):
    """the plan exists; the query and the call raise the library's own message and nothing is written"""
    from dedalus_amd import libhip
    from dedalus_amd.device import ptr
    c = tc.Case(kind, N, M, 0, (), 0, {}, "")
    plan = _make_plan(kind, N, M, 0)
    for shape in tc.shapes_for(N):
        outer, inner = tc.outer_inner(shape)
        for op in ("forward", "backward"):
            with pytest.raises(libhip.DdhError, match=text):
                _plan_info(plan, kind, op, outer, inner)
            x = tc.make_input(c, op, shape)
            d_x = dev.from_host(x)
            dst = Guarded(dev, outer * inner * tc.out_axis(c, op))
            before = _wave_launches()
            with pytest.raises(libhip.DdhError, match=text):
                libhip.call("ddh_%s_%s" % (kind, op), plan, ptr(d_x), dst.ptr(), outer, inner, dev.stream)
            dev.sync()
            got, intact = dst.fetch()
            assert intact and np.isnan(got).all() and _wave_launches() == before, "a refused call launched something"
    libhip.call("ddh_destroy", plan)


@pytest.mark.parametrize("kind,N,M,text", tc.CALL_REFUSALS)
def test_call_refusals(dev, kind, N, M, text):
    _assert_refused(dev, kind, N, M, text)


@pytest.mark.parametrize("kind,N,M", tc.LDS_EDGE)
def test_lines_that_fit_lds_only_without_the_twiddle_table(dev, kind, N, M):
    """Either the transform runs and matches, or the library refuses with its own "axis too long" -- never a bare HIP error.
    transform_plan holds the whole dynamic-LDS request (lines and twiddle table) against 160 KiB, so these are refused."""
    assert tc.plan_mirror(kind, N, 3, 1) == "axis too long"
    _assert_refused(dev, kind, N, M, "axis too long for the LDS kernel")
