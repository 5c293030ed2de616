"""GPU: the fused grid stage (ddh_rfft_bilinear_fused) away from the 3/2 rule, at the sizes where fused_plan changes its
selection (tests/fused_stage_cases.py; CPU twin: tests/test_fused_stage_host.py).

Every case first asserts, through ddh_rfft_fused_plan_info, that the library takes the kernel family, C, NT and lines per
wave its row claims, so that a fallback fails.  Then, rel-L2 <= 1e-12 (the standing bound of tests/test_gpu_transforms.py)
of every output array against the double-precision oracle on all lines, and of every (result, line) against the longdouble
matrix reference on a subset of lines: the first and the last four, every line the last workgroup takes (the wave kernels
are grid-stride: in all its passes), the last line of every wave a ragged count cuts short, and 32 random ones.  Outputs
are NaN-filled before the call, a NaN guard of 64 doubles behind each must come back untouched, and two identical calls
agree bit for bit.  Cases with several lines per wave: seven lines each of the first, the second and the last pass equal
the same lines run alone, bit for bit.  The 16387- and 65541-line cases: a NaN planted in the line operand of line
nlines - 2 (the last line of its wave), and in a second run in lines of other waves that take further lines afterwards,
makes exactly those lines' results NaN and changes no other line.

End to end: a Rayleigh-Benard box with a y basis of 128 modes on 128 points against the reference's end state."""
import os

import numpy as np
import pytest

import fused_stage_cases as fc

pytestmark = pytest.mark.gpu

CASE_IDS = [fc.case_id(c) for c in fc.CASES]


@pytest.fixture(scope="module")
def hex_():
    from dedalus_amd.device import Device
    from dedalus_amd.executor import HipExecutor
    return HipExecutor(Device.get())


def run_stage(hex_, case, a, b):
    """one call on device copies of a, b: (out [nc][nlines][M], guards [nc][GUARD]); outputs and guards NaN before it"""
    na, nb, nc, terms, ads, bds = fc.TABLES[case.table]
    n = case.nlines * case.M
    da, db = hex_.from_host(np.array(a)), hex_.from_host(np.array(b))          # (copies: the shared inputs are read-only)
    buf = hex_.empty((nc, n + fc.GUARD))
    buf.fill_(float("nan"))
    hex_.rfft_bilinear_fused(("rfft", case.N, case.M), None, [da[i] for i in range(na)], [db[i] for i in range(nb)],
                             [buf[i][:n] for i in range(nc)], case.nlines, terms, ads, bds)
    hex_.sync()
    got = hex_.download(buf)
    return got[:, :n].reshape(nc, case.nlines, case.M), got[:, n:]


@pytest.mark.parametrize("case", fc.CASES, ids=CASE_IDS)
def test_fused_stage_at_the_selection_edges(hex_, case):
    sel = fc.assert_selection(case)
    a, b, ora, lines, ref = fc.references(case)
    got, guard = run_stage(hex_, case, a, b)
    again, _ = run_stage(hex_, case, a, b)
    err_oracle = max(fc.rel(got[i], ora[i]) for i in range(got.shape[0])) if np.isfinite(got).all() else float("nan")
    err_line = fc.per_line_error(got[:, lines], ref)
    print("FUSEDROW %-22s internal %4d family %d C %d NT %d twreg %d dma %d lpw %d grid %5d | oracle %.2e per-line %.2e"
          % (fc.case_id(case), sel["internal"], sel["family"], sel["C"], sel["NT"], sel["twreg"], sel["dma"], sel["lpw"],
             sel["grid"], err_oracle, err_line))
    assert np.isnan(guard).all(), "the guard behind an output was written"
    assert np.isfinite(got).all()
    assert np.array_equal(got, again), "two identical calls differ"
    for i in range(got.shape[0]):
        assert fc.rel(got[i], ora[i]) <= fc.TOL, (i, fc.rel(got[i], ora[i]))
    assert err_line <= fc.TOL, err_line
    if case.family == fc.WG or case.lpw == 1:
        return
    # Several lines per wave.  A wave's lines are 4 * grid apart (fused_stage_cases.wave_place), so lines 0..6 are all
    # first lines of their waves: the lines compared with a run of their own also include seven of the second and seven of
    # the last pass, which their waves take after other lines, with the staging, the exchange buffer and the register
    # twiddles those left behind.
    al = fc.alone_lines(case)
    assert al[:7] == list(range(7)) and fc.wave_place(case, al[-1])[2] == case.lpw - 1
    few = case._replace(nlines=len(al), lpw=1)
    fc.assert_selection(few)
    alone, _ = run_stage(hex_, few, a[:, al], b[:, al])
    assert np.array_equal(alone, got[:, al]), "a line depends on the lines its wave took before it"
    if case.nlines not in (16387, 65541):
        return
    # A NaN in the line operand of one line makes that line's result NaN and changes no other line.  Line nlines - 2 is the
    # last line its wave takes: what it leaves behind can reach only an earlier line (an operand prefetched across the line
    # boundary).  The second run plants lines of other waves that take further lines afterwards: a stale staging or
    # exchange buffer would carry the NaN forward into those.
    K = fc.kmax(case.N, case.M)
    last, others = fc.nan_plants(case)
    for bad in ([last], others):
        bp = b.copy()
        bp[0, bad, 2] = np.nan
        planted, guard = run_stage(hex_, case, a, bp)
        assert np.isnan(guard).all()
        assert np.isnan(planted[:, bad, 0]).all() and np.isnan(planted[:, bad, 2:2 * K + 2]).all()
        planted[:, bad] = got[:, bad]
        assert np.array_equal(planted, got), ("a NaN of one line reached another line", bad)


def test_dealias1_box_matches_the_reference(golden_dir):
    """128 modes on 128 points along the fused axis: the products alias on the 128-point grid in the reference, and the
    stage must keep that.  Bounds: those of tests/test_gpu_ivp.py for RK222 end states."""
    import dedalus_amd.public as d3
    import test_gpu_ivp
    from problems import SCHEME_TOL as TOL
    assert TOL == test_gpu_ivp.TOL                       # one set of figures, shared with the CPU twin
    gold = np.load(os.path.join(golden_dir, fc.E2E_GOLDEN))
    solver, fields = fc.rayleigh_benard_dealias1(d3)
    assert solver.ex.name == "hip"
    specs = []
    inner = solver.ex.rfft_bilinear_fused

    def spy(spec, *args, **kw):
        specs.append(tuple(spec))
        return inner(spec, *args, **kw)
    solver.ex.rfft_bilinear_fused = spy
    try:
        for _ in range(fc.E2E_STEPS):
            solver.step(fc.E2E_DT)
    finally:
        del solver.ex.rfft_bilinear_fused
    assert specs and set(specs) == {fc.E2E_SPEC}
    end = {k: np.array(f['c']) for k, f in fields.items()}
    for k, v in end.items():
        print("FUSEDE2E %-7s %.2e" % (k, fc.rel(v, gold[k])))
    for k, v in end.items():
        assert np.isfinite(v).all()
        assert fc.rel(v, gold[k]) < TOL.get(k, 1e-10), (k, fc.rel(v, gold[k]))
    info = fc.plan_info(128, 128, 64)
    assert info["internal"] == 128 and info["family"] == fc.WG
