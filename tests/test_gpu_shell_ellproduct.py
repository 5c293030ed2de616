"""GPU: SphericalEllProduct and the potential-field walls of tests/test_shell_ellproduct.py on the device (same cases, same
bounds), the IVP steps replayed from a HIP graph bit for bit, and ddh_ell_mix_apply (csrc/ddh_ellmix.hip) on diagonal lists
at the edges of its launch shape (tests/shell_ellproduct_cases.py::DIAG_CASES).

Bound of the kernel cases: a diagonal mix has one product per output element, so every element lies within
2 u |q| |x| of the longdouble product (u = 2^-53: one rounding of the product, one of the sum with the zero the
accumulator starts from, whether or not the two are fused).  Inputs and outputs sit inside NaN guards; slots without a
mode hold NaN on input and +0 on output; a component without a term is +0; two calls give the same bits.
With DDH_ELLPRODUCT_OUT=<file> the measured figures of every case are appended to that file."""
import os

import numpy as np
import pytest

import shell_ellproduct_cases as se
import test_shell_ellproduct as host
from test_gpu_ell_mix_kernel import guarded, guards_intact

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


def record(lines):
    path = os.environ.get("DDH_ELLPRODUCT_OUT")
    if path:
        with open(path, "a") as fh:
            for line in lines:
                fh.write(line + "\n")


@pytest.fixture(scope="module")
def ex():
    from dedalus_amd.executor import HipExecutor
    return HipExecutor()


@pytest.mark.parametrize("shape", se.OP_SHAPES, ids=se.tag)
def test_ell_product_matches_reference_gpu(shape):
    import dedalus_amd.public as d3
    rec = []
    host.check_ops(shape, None, rec)
    assert d3.Distributor(d3.SphericalCoordinates("phi", "theta", "r"), dtype=np.float64).executor.name == "hip"
    record(["op %s %s rel-l2 %.3e" % r for r in rec])


def test_potential_wall_lbvp_gpu():
    rec = []
    solver = host.check_lbvp(None, rec)
    assert solver.ex.name == "hip"
    record(["lbvp %s %s" % (k, " ".join("%s %.2e" % kv for kv in sorted(d.items()))) for (_, errs, own) in rec
            for k, d in (("measured", errs), ("taus-own-norm", {t: own[t] for t in ("tau_A1", "tau_A2")}))])


@pytest.mark.parametrize("ts", ["RK222", "SBDF2"])
def test_potential_wall_induction_end_state_gpu(ts):
    rec = []
    solver = host.check_induction(ts, None, rec)
    assert solver.ex.name == "hip"
    band = solver._band
    path = "dense inverses" if not band else "band LU, dense for ell in %s" % (band["plan"].why_dense,)
    print("LHS path:", path)
    assert band is not None
    record(["ivp %s %s %s" % (ts, k, " ".join("%s %.2e" % kv for kv in sorted(d.items()))) for (_, errs, own) in rec
            for k, d in (("measured", errs), ("taus-own-norm", {t: own[t] for t in ("tau_A1", "tau_A2")}))]
           + ["ivp %s LHS path: %s" % (ts, path)])


def test_induction_step_graphs_reproduce_ordinary_steps():
    """SBDF2 with a fixed timestep replayed from HIP graphs (one per phase of the history rotation) against ordinary launches"""
    import dedalus_amd.public as d3
    GOLD = host.gold("shell_ellproduct_ivp.npz")
    out = []
    for graph in (False, True):
        s, f = se.potential_induction(d3, "SBDF2")
        f["A"]["c"] = GOLD["ivp/in_A"].astype(np.float64)
        if graph:
            s.enable_step_graph(True)
        for _ in range(12):
            s.step(se.IVP_DT)
        if graph:
            assert len(s._graph["graphs"]) == 2 and not s._graph["failed"]       # both phases captured and replayed
        out.append({k: v for k, v in se.end_state(f).items()})
    assert np.abs(out[0]["A"]).max() > 0.1
    for k in out[0]:
        assert np.array_equal(out[0][k].view(np.uint64), out[1][k].view(np.uint64)), k


@pytest.mark.parametrize("label", [c[0] for c in se.DIAG_CASES])
def test_diagonal_mix_kernel_pinned(ex, label):
    nm, nl, nr, nc, terms, slot_map, x = se.diag_case(label)
    assert all(co == ci for (co, ci, q) in terms)
    LD = np.longdouble
    live = slot_map >= 0
    xs = np.where(np.isnan(x), 0.0, x).astype(LD)
    ref, mag = np.zeros(x.shape, LD), np.zeros(x.shape, LD)
    for (c, _, q) in terms:
        qs = np.asarray(q).astype(LD)[np.where(live, slot_map, 0)][:, :, None] * live[:, :, None]
        ref[c] = qs * xs[c]
        mag[c] = np.abs(qs) * np.abs(xs[c])
    dev = ex.make_ell_mix(nm, nl, nr, nc, nc, terms, slot_map)
    n = x.size
    xbuf, xd, xlead = guarded(ex, n, 0.0, False)
    xd.copy_(ex.from_host(np.ascontiguousarray(x)).reshape(-1))
    xd = xd.reshape(x.shape)
    outs = []
    for call in range(2):
        ybuf, yd, ylead = guarded(ex, n, 7.0, False)
        dev.apply(xd, yd.reshape(x.shape))
        ex.sync()
        assert guards_intact(ex, ybuf, ylead, n), "the kernel wrote outside its output"
        outs.append(np.array(ex.download(yd)).reshape(x.shape))
    assert guards_intact(ex, xbuf, xlead, n)
    y = outs[0]
    assert np.array_equal(y.view(np.uint64), outs[1].view(np.uint64)), "two calls differ"
    assert not np.isnan(y).any(), "a slot without a mode was read"
    dead = y[:, ~live, :]
    assert dead.size and np.all(dead.view(np.uint64) == 0), "slots without a mode must hold +0"
    without = [c for c in range(nc) if c not in [t[0] for t in terms]]
    assert all(np.all(y[c].view(np.uint64) == 0) for c in without), "a component without a term must hold +0"
    bound = 2 * U * mag
    err = np.abs(y.astype(LD) - ref)
    worst = float((err / np.maximum(bound, np.finfo(np.float64).tiny)).max())
    print("%s: worst error / (2 u |q||x|) %.3f" % (label, worst))
    record(["kernel %s nm %d nl %d nr %d ncomp %d terms %d: worst error / (2 u |q||x|) %.3f" % (label, nm, nl, nr, nc, len(terms), worst)])
    assert np.abs(ref).max() > 0.5 and np.all(err <= bound), (label, worst)
