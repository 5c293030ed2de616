"""GPU: adaptive runs under a CFL of several velocities and scalar frequencies (tests/cfl_terms_cases.py) against the dt
sequences of the unmodified reference (tests/golden/cfl_terms.npz, written by tools/make_golden_cfl_terms.py).  Tolerance:
that of the single-velocity comparison in tests/test_gpu_ivp.py (rtol 1e-11 on every timestep)."""
import os

import numpy as np
import pytest

import cfl_terms_cases as tc

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cfl_terms.npz")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


@pytest.mark.parametrize("name", [n for n in tc.CASES if n != "rb_profile_capped"])
def test_dt_sequence_matches_reference(gold, name):
    import dedalus_amd.public as d3
    solver, dts = tc.CASES[name](d3)
    assert solver.ex.name == "hip"
    ref = gold[name]
    print(name, "worst relative deviation %.3e" % np.max(np.abs(dts - ref) / ref))
    assert dts.shape == ref.shape and np.allclose(dts, ref, rtol=1e-11, atol=0), np.max(np.abs(dts - ref) / ref)


def test_dt_sequence_is_identical_when_steps_replay_from_graphs(gold, monkeypatch):
    """cadence 3 and a timestep that sits at max_dt: with DDH_STEP_GRAPH=1 the steps between two samples are replayed from a
    captured graph (a sample reads the velocity on the grid, so that step runs as ordinary launches); the dt sequence is
    the one of ordinary launches, bit for bit, and the reference's."""
    import dedalus_amd.public as d3
    monkeypatch.setenv("DDH_STEP_GRAPH", "0")
    plain, dts0 = tc.rb_profile_capped(d3)
    assert not getattr(plain, "_graph", None)
    monkeypatch.setenv("DDH_STEP_GRAPH", "1")
    solver, dts1 = tc.rb_profile_capped(d3)
    assert solver._graph["graphs"] and not solver._graph["failed"]
    assert np.array_equal(dts0, dts1)
    ref = gold["rb_profile_capped"]
    assert np.allclose(dts1, ref, rtol=1e-11, atol=0), np.max(np.abs(dts1 - ref) / ref)
