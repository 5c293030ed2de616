"""GPU: the curl on a shell left-hand side on HipExecutor -- the Beltrami-like LBVP and the alpha^2 dynamo of
tests/shell_curl_lhs_cases.py against tests/golden/shell_curl_lhs.npz with the bounds of tests/test_shell_curl_lhs.py
(1e-10), through the complex band LU of csrc/ddh_ellband.hip and once more with dense inverses (DDH_SHELL_DENSE=1);
repeated runs and the RK222 steps replayed from a HIP graph are bit-identical."""
import numpy as np
import pytest

import shell_curl_lhs_cases as sc
import test_shell_curl_lhs as host

pytestmark = pytest.mark.gpu


def test_curl_lhs_lbvp_gpu():
    solver = host.check_lbvp(None)
    assert solver.ex.name == "hip" and solver.cx


@pytest.mark.parametrize("ts", ["RK222", "SBDF2"])
def test_alpha2_dynamo_end_state_gpu(ts):
    solver, res = host.check_dynamo(ts, None)
    assert solver.ex.name == "hip"
    band = solver._band
    assert band and band["plan"].cx and band["dev"].cx and len(band["plan"].per) > 0
    print("LHS path: complex band LU for ell in %s, dense for %s" % (sorted(band["plan"].per), band["plan"].why_dense))


@pytest.mark.parametrize("ts", ["RK222", "SBDF2"])
def test_alpha2_dynamo_dense_inverses_gpu(ts, monkeypatch):
    monkeypatch.setenv("DDH_SHELL_DENSE", "1")
    solver, res = host.check_dynamo(ts, None)
    assert solver.ex.name == "hip" and solver._band is False


def test_repeated_runs_and_step_graph_are_bit_identical():
    import dedalus_amd.public as d3
    GOLD = host.gold()
    out = []
    for graph in (False, False, True):
        before = (lambda s: s.enable_step_graph(True)) if graph else None
        solver, f, res = sc.run_alpha2_dynamo(d3, "RK222", GOLD["ivp/in_B"], steps=8, before=before)
        if graph:
            assert solver._graph["graphs"] and not solver._graph["failed"]
        assert solver._band["plan"].cx
        out.append(res)
    assert np.abs(out[0]["B"]).max() > 0.05
    for k in out[0]:
        assert np.array_equal(out[0][k].view(np.uint64), out[1][k].view(np.uint64)), ("repeat", k)
        assert np.array_equal(out[0][k].view(np.uint64), out[2][k].view(np.uint64)), ("graph", k)
