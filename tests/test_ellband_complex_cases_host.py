"""Host proof of tests/ellband_complex_cases.py (no GPU): the complex synthetic plans are well conditioned and exercise
the interchanges, the table reaches every edge of the four compiled complex windows, pair counts lie on either side of
the sweeps' 16 / 64 pairs per wave, the clongdouble reference and the zgbtrf / zgbtrs baseline agree to the baseline's
rounding, and EllBandPlan.reference_solve (zgbtrf / zgbtrs for a complex plan) is that baseline."""
import numpy as np
import pytest

import ellband_cases as ec
import ellband_complex_cases as cc

U = 2.0 ** -53


def test_table_reaches_every_window_edge_and_pair_count():
    assert {ec.CASES[n][2:4] for n in cc.CX_CASES} == set(cc.CX_VARIANTS)
    for name in cc.CX_WIDEST:
        kl, ku, nw, wt = ec.CASES[name][:4]
        assert name in cc.CX_CASES and ec.variant_for(kl, ku) == (nw, wt) and (kl + 1 == nw or kl + ku == wt)
    for name in cc.CX_REFUSED:
        assert ec.CASES[name][2:4] == (36, 96)
    assert sorted(set(cc.CX_CASES.values())) == [1, 15, 16, 17, 63, 64, 65]
    assert cc.BACKWARD_PAIRS == 16 and cc.FORWARD_PAIRS == 64
    nbcs, mps, lims = set(), set(), set()
    for name in cc.CX_CASES:
        plan, nslots, lim = cc.case(name)
        kl, ku, nw, wt, mp, nbc = ec.CASES[name][:6]
        assert plan.cx and plan.MB.dtype == np.complex128 and nslots % 2 == 0 and np.all(lim % 2 == 0)
        sizes = set(int(v) for v in plan.n)
        assert {0, 1, nw - 1, nw, wt, wt + 1} <= sizes | {v for v in (wt, wt + 1) if v > ec.CASES[name][8]}
        nbcs.add(nbc)
        mps.add(mp)
        lims |= {("zero" if v == 0 else "two" if v == 2 else "full" if v == nslots else "other") for v in lim}
        assert nslots <= 130 and plan.nmax <= 300
    assert {0, 1, 8} <= nbcs and {0, 1, 16} <= mps and {"zero", "two", "full"} <= lims
    assert any(lay == "rows_by_slots" for _, lay in cc.CX_CASE_LAYOUTS)


@pytest.mark.parametrize("name", list(cc.CX_CASES))
def test_inputs_and_references(name):
    plan, nslots, lim = cc.case(name)
    kl = plan.kl
    cols = cc.rhs_columns(name)
    seen_kl = False
    for g in range(plan.nl):
        n = int(plan.n[g])
        assert np.isnan(plan.MB[g, n:]).all() and np.isnan(plan.LB[g, n:]).all()
        if n == 0:
            continue
        band = plan.MB[g, :n]
        assert np.any(band.imag != 0) or n == 1
        for a, b in ec.AB_PAIRS:
            A = plan.dense(g, a, b, np.float64)
            assert A.dtype == np.complex128 and np.linalg.cond(A) <= ec.COND_CAP
            lu, piv, info = cc.band_lu(plan, g, a, b)
            assert info == 0
            off = ec.pivot_offsets(piv)
            assert off.max() <= kl
            seen_kl |= bool(off.max() == kl and kl > 0)
    assert seen_kl or kl == 0 or plan.n.max() <= kl
    a, b = ec.AB_PAIRS[0]
    sol = cc.solved(name, "default", a, b)
    for g, s in sol.items():
        n = int(plan.n[g])
        A = plan.dense(g, a, b)
        r = cc.permuted_rhs(plan, g, cols[g])
        # the reference solves its system to clongdouble rounding, the baseline to complex128 rounding of a stable LU
        assert cc.backward_error(plan, g, a, b, cols[g], s["y"]) <= 1e-3 * U
        assert s["eta_b"] <= 64 * n * U
        cond = np.linalg.cond(A.astype(np.complex128))
        assert s["err_b"] <= 64 * n * U * cond * 10
        # EllBandPlan.reference_solve of a complex plan is the zgbtrf / zgbtrs path
        from dedalus_amd.core.ellband import EllBandPlan
        flat = np.zeros((plan.ncomp * plan.nr, cols[g].shape[1]), dtype=complex)
        flat[plan.row_index[g, :n]] = cols[g]
        out = EllBandPlan.reference_solve(plan, g, a, b, flat)
        assert np.array_equal(out[plan.col_index[g, :n]], s["zb"])


@pytest.mark.parametrize("name", cc.CX_WIDEST)
def test_pivot_cases(name):
    plan, nslots, lim = cc.pivot_case(name)
    for a, b in ec.AB_PAIRS:
        off0 = ec.pivot_offsets(cc.band_lu(plan, 0, a, b)[1])
        off1 = ec.pivot_offsets(cc.band_lu(plan, 1, a, b)[1])
        assert not off0.any()
        assert np.count_nonzero(off1) == 1 and off1.max() == plan.kl


def test_zero_pivot_case_is_singular_where_planted():
    plan, nslots, lim, singular = cc.zero_pivot_case()
    a, b = ec.AB_PAIRS[0]
    for g in range(plan.nl):
        info = cc.band_lu(plan, g, a, b)[2]
        assert (info > 0) == (g in singular)
