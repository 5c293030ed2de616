"""GPU: cross product and curl of shell vector fields on the device.

  * (a), (b) of tests/shell_vector_cases.py through the public d3 names against the reference's results
    (tests/golden/shell_vector_ops.npz), with the bounds of tests/test_shell_vector_ops.py;
  * the banded kernel of ddh_ell_terms_apply pinned at the edges of its launch shape, the instance with rotated terms (the
    flags as generated) and the one without (all flags zero): a longdouble product of the same term list, entry by
    entry within (K + 2) u sum |a| |x| (K: products summed for that entry; the form of tests/test_gpu_swsh_kernels.py),
    behind NaN guards around the output and NaN in every input slot that carries no mode -- the (m, ell) = (0, 0) msin
    slot among them: those slots receive +0, nothing outside the output changes, two calls give identical bits, a call
    on a side stream and the replay of a captured graph give the same bits again;
  * (c) the rotating convection run against the reference's end state (bounds of the shell end-state tests,
    tests/test_shell_fields.py::CONV_TOL), and a curl task that leaves the stepped state bit-identical.

The msin slot of m = 0 carries modes of a VECTOR for ell >= 1 (valid_elements of the reference, core/basis.py:4299-4305,
drops it at ell = 0 only: the azimuthal component of an axisymmetric field lives there), so only (0, 0) is a hole."""
import os

import numpy as np
import pytest

import shell_vector_cases as sv
import test_shell_vector_ops as host

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
GUARD = 4096


@pytest.fixture(scope="module")
def ex():
    from dedalus_amd.executor import HipExecutor
    return HipExecutor()


@pytest.mark.parametrize("shape", sv.CURL_SHAPES, ids=sv.tag)
def test_curl_matches_reference_gpu(shape):
    import dedalus_amd.public as d3
    from dedalus_amd.core.shell import ShLinear
    coords, dist, shell, u, v = sv.build(d3, (8, 4, 6))
    assert isinstance(d3.curl(u), ShLinear) and isinstance(d3.Curl(u), ShLinear)      # not the Cartesian operator
    assert dist.executor.name == "hip"
    host.check_tasks("curl", shape, None)


@pytest.mark.parametrize("shape", sv.CROSS_SHAPES, ids=sv.tag)
def test_cross_matches_reference_gpu(shape):
    import dedalus_amd.public as d3
    from dedalus_amd.core.shell import ShProduct
    coords, dist, shell, u, v = sv.build(d3, (8, 4, 6))
    assert isinstance(d3.cross(u, v), ShProduct) and isinstance(d3.CrossProduct(u, v), ShProduct)
    assert dist.executor.name == "hip"
    host.check_tasks("cross", shape, None)


def guarded(ex, n, fill):
    buf = ex.dev.empty((n + 2 * GUARD,))
    buf.fill_(float("nan"))
    body = buf[GUARD:GUARD + n]
    body.fill_(fill)
    return buf, body


def guards_intact(ex, buf, n):
    h = np.array(ex.download(buf))
    return np.isnan(h[:GUARD]).all() and np.isnan(h[GUARD + n:]).all()


@pytest.mark.parametrize("rot_form", ["as_generated", "all_zero"])
@pytest.mark.parametrize("label", [c[0] for c in sv.KERNEL_CASES])
def test_ell_terms_kernel_pinned(ex, label, rot_form):
    import torch
    nm, nl, nr, nco, terms, rot, slot_map, x = sv.kernel_case(label)
    if rot_form == "all_zero":
        rot = [0] * len(rot)
    assert any(rot) == (rot_form == "as_generated")
    ref, mag, cnt = sv.kernel_reference(nm, nl, nr, nco, terms, rot, slot_map, x)
    dev = ex.make_ell_terms(nm, nl, nr, nco, terms, slot_map, rot=rot)
    n = nco * 2 * nm * nl * nr
    xbuf, xd = guarded(ex, x.size, 0.0)                              # NaN around x as well
    xd.copy_(ex.from_host(np.ascontiguousarray(x)).reshape(-1))
    xd = xd.reshape(x.shape)
    outs = []
    for call in range(2):
        ybuf, yd = guarded(ex, n, 7.0)
        dev.apply(xd, yd.reshape(nco, 2 * nm, nl, nr))
        ex.sync()
        assert guards_intact(ex, ybuf, n), "the kernel wrote outside its output"
        outs.append(np.array(ex.download(yd)).reshape(nco, 2 * nm, nl, nr))
    y = outs[0]
    assert np.array_equal(y.view(np.uint64), outs[1].view(np.uint64)), "two calls differ"
    assert not np.isnan(y).any(), "a slot without a mode was read"
    dead = y[:, slot_map < 0, :]
    assert dead.size and np.all(dead.view(np.uint64) == 0), "slots without a mode must hold +0"
    bound = (cnt + 2) * U * mag
    excess = np.abs(y.astype(np.longdouble) - ref) - bound
    worst = float((np.abs(y.astype(np.longdouble) - ref) / np.maximum(bound, np.finfo(np.float64).tiny)).max())
    print("%s: worst error / bound %.3f, K <= %d" % (label, worst, int(cnt.max())))
    assert np.all(excess <= 0), (label, worst)
    # a caller's stream, then a captured graph replayed: the same bits
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    ybuf, yd = guarded(ex, n, 7.0)
    y4 = yd.reshape(nco, 2 * nm, nl, nr)
    with torch.cuda.stream(side):
        dev.apply(xd, y4)
    side.synchronize()
    assert np.array_equal(np.array(ex.download(y4)).view(np.uint64), y.view(np.uint64))
    yd.fill_(7.0)
    ex.sync()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        dev.apply(xd, y4)
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(np.array(ex.download(y4)).view(np.uint64), y.view(np.uint64))
    assert guards_intact(ex, ybuf, n)


def test_curl_leaves_other_operators_alone_gpu():
    host.check_curl_leaves_other_operators_alone(None)


def test_rotating_convection_end_state_gpu():
    """(c): three SBDF2 steps with the Coriolis force on the right-hand side, ordinary launches; every variable, the
    task curl(u) and the flow property sqrt(curl(u)@curl(u)) against the reference"""
    import dedalus_amd.public as d3
    G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shell_vector_ivp.npz"))
    solver, res = sv.run_rotating_convection(d3)
    assert solver.ex.name == "hip"
    tol = dict(host.CONV_TOL, curl_u=host.CONV_TOL["u"], enstrophy_sqrt=host.CONV_TOL["u"])
    for k, t in tol.items():
        ref = G["end/" + k]
        assert res[k].shape == ref.shape, (k, res[k].shape, ref.shape)
        err = host.rel(res[k], ref)
        print("rotating convection %s: %.3e" % (k, err))
    for k, t in tol.items():
        assert host.rel(res[k], G["end/" + k]) < t, (k, host.rel(res[k], G["end/" + k]))
    assert abs(float(res["tau_p"].reshape(-1)[0])) < 1e-10


def test_curl_task_leaves_the_state_untouched_gpu():
    import dedalus_amd.public as d3
    ends = []
    for task in (False, True):
        solver, f = sv.rotating_convection(d3, shape=(16, 8, 16))
        for _ in range(3):
            solver.step(sv.IVP_DT)
            if task:
                w = np.array(d3.curl(f["u"]).evaluate()["c"])
                assert np.isfinite(w).all()
        ends.append({k: np.array(f[k]["c"]) for k in ("p", "b", "u")})
    for k in ends[0]:
        assert np.array_equal(ends[0][k].view(np.uint64), ends[1][k].view(np.uint64)), k
    assert np.abs(ends[0]["u"]).max() > 0
