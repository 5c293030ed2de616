"""CPU: the references, the case table and the kernel selection that tests/test_gpu_fused_stage.py runs the fused grid
stage against (tests/fused_stage_cases.py).

The double-precision oracle stays within 1e-13 per line of the longdouble matrix restatement on every case, a tenth of the
bound the kernels get.  ddh_rfft_fused_plan_info (host only: no plan, no device) reports for every case exactly the
selection its row claims, and over all 16 <= M <= N <= 1024 an internal grid other than the plan's own only where the
own grid is free of aliasing.  The end-to-end problem with a y basis of 128 modes on 128 points reaches the reference's end
state on the oracle executor."""
import os

import numpy as np
import pytest

import fused_stage_cases as fc

CASE_IDS = [fc.case_id(c) for c in fc.CASES]


def test_longdouble_is_wider_than_double():
    assert np.finfo(fc.LD).eps < 1e-18
    assert abs(float(fc.PI) - np.pi) == 0.0 and fc.PI != fc.LD(np.pi)


def test_case_table_covers_the_selection_edges():
    assert len(set(CASE_IDS)) == len(CASE_IDS)
    seen = {(c.family, c.C, c.NT) for c in fc.CASES}
    assert {(fc.GW, 4, 4), (fc.GW, 8, 8), (fc.GW, 6, 6), (fc.GW, 3, 3), (fc.GW, 2, 2), (fc.GW, 3, 2), (fc.GW, 6, 4),
            (fc.GW, 8, 6), (fc.GW2, 3, 2), (fc.WG, 0, 0)} <= seen
    assert {c.lpw for c in fc.CASES if c.family != fc.WG} == {1, 2, 8}
    for c in fc.CASES:
        K = fc.kmax(c.N, c.M)
        assert c.internal == fc.internal_grid(c.N, c.M), fc.case_id(c)
        assert (c.internal != c.N) <= (c.N > 3 * K)
        if "under-dealiased" in c.what:
            assert c.N <= 3 * K and c.N not in fc.WAVE_SIZES and c.family == fc.WG
        if c.what.startswith("lines per wave") and c.lpw > 1 and c.nlines != 16384:
            # a ragged count: the last workgroup and some waves of others take fewer lines than lines per wave
            assert fc.passes(c) == c.lpw and 0 < len(fc.last_workgroup_lines(c)) < fc.WAVES * c.lpw
            assert 0 < len(fc.short_wave_lines(c)) < fc.WAVES * c.lpw
    ragged = [c for c in fc.CASES if c.nlines == 65541]
    assert len(ragged) == 1 and fc.wave_grid(ragged[0]) == 2049
    # the placement model against the kernels' loop, restated: wave w of workgroup g takes g * 4 + w, + 4 * grid, ...
    for c in fc.CASES:
        if c.family == fc.WG or c.nlines < 8191:
            continue
        grid, seen = fc.wave_grid(c), {}
        for g in (0, 1, grid - 2, grid - 1):
            for w in range(fc.WAVES):
                mine = list(range(g * fc.WAVES + w, c.nlines, grid * fc.WAVES))
                assert len(mine) <= c.lpw
                for p, l in enumerate(mine):
                    assert fc.wave_place(c, l) == (g, w, p)
                seen[(g, w)] = mine
        assert sorted(l for w in range(fc.WAVES) for l in seen[(grid - 1, w)]) == fc.last_workgroup_lines(c)
        short = set(fc.short_wave_lines(c))
        for (g, w), mine in seen.items():
            assert (len(mine) < fc.passes(c) and bool(mine)) == (bool(mine) and mine[-1] in short), (g, w)
        if c.lpw > 1:
            last, others = fc.nan_plants(c)
            assert fc.wave_place(c, last)[2] == fc.passes(c) - 1 and last == c.nlines - 2
            assert all(fc.wave_place(c, l)[2] < fc.passes(c) - 1 for l in others)
            al = fc.alone_lines(c)
            assert {fc.wave_place(c, l)[2] for l in al} == {0, 1, fc.passes(c) - 1} and len(al) == 7 * len({0, 1, fc.passes(c) - 1})
    c16 = next(c for c in fc.CASES if c.nlines == 16387 and c.family == fc.GW)
    assert fc.last_workgroup_lines(c16) == [8192, 8193, 8194, 8195] and fc.wave_place(c16, 16385) == (2047, 1, 1)
    assert fc.short_wave_lines(c16) == [8191, 8192, 8193, 8194, 8195]
    assert fc.wave_place(ragged[0], 65539) == (2041, 3, 7)
    # odd line counts on the workgroup kernel: the last line has no partner
    assert any(c.family == fc.WG and c.nlines & 1 and c.nlines > 1 for c in fc.CASES)
    for name, (na, nb, nc, terms, ads, bds) in fc.TABLES.items():
        assert len(ads) == na and len(bds) == nb and any(bds)
        assert all(0 <= ic < nc and 0 <= ia < na and 0 <= ib < nb for ic, ia, ib, _ in terms)
        assert {t[0] for t in terms} == set(range(nc))
    assert fc.TABLES["grad"][:3] == (3, 12, 4) and fc.TABLES["one"][:3] == (1, 1, 1)


@pytest.mark.parametrize("N,M", [(24, 16), (60, 60), (128, 100), (192, 128)])
def test_longdouble_matrices_restate_the_oracle_transforms(N, M):
    """the synthesis and analysis matrices against oracle/np_transforms.py, and the derivative form against the oracle's
    differentiation at load"""
    from oracle import np_transforms as npt
    from oracle.np_executor import NumpyExecutor
    S, D, A = fc.matrices(N, M)
    F, Bm = npt.real_fourier_mmt_matrices(N, M)
    # (the double matrices take cos / sin of the unreduced k x: two roundings of an argument of up to 2 pi kmax)
    arg = 2 * np.pi * fc.kmax(N, M) * 2 * np.finfo(float).eps + 1e-15
    assert np.abs(S.astype(float) - Bm).max() < arg and np.abs(A.astype(float) - F).max() < arg * 2 / N
    rng = np.random.default_rng(N)
    c = rng.standard_normal((3, M))
    c[:, 1] = 0.0
    g = npt.rfft_backward(c.reshape(3, M, 1), 1, N)[..., 0]
    assert fc.rel(g, (c.astype(fc.LD) @ S.T).astype(float)) < 1e-14
    assert fc.rel(npt.rfft_forward(g.reshape(3, N, 1), 1, M)[..., 0], (g.astype(fc.LD) @ A.T).astype(float)) < 1e-14
    dc = NumpyExecutor._fourier_diff(c, 1.7)
    assert fc.rel((dc.astype(fc.LD) @ S.T).astype(float), (c.astype(fc.LD) @ (fc.LD(1.7) * D).T).astype(float)) < 1e-14
    K = fc.kmax(N, M)
    assert not S[:, 1].any() and not S[:, 2 * K + 2:].any() and not A[1].any() and not A[2 * K + 2:].any()


@pytest.mark.parametrize("case", fc.CASES, ids=CASE_IDS)
def test_oracle_is_within_a_tenth_of_the_kernel_bound_of_the_longdouble_reference(case):
    a, b, ora, lines, ref = fc.references(case)
    assert lines[0] == 0 and lines[-1] == case.nlines - 1 and set(fc.last_workgroup_lines(case)) <= set(lines.tolist())
    assert np.isfinite(ora).all() and ref.shape == (ora.shape[0], len(lines), case.M)
    err = fc.per_line_error(ora[:, lines], ref)
    print("ORACLE %-22s per-line %.2e" % (fc.case_id(case), err))
    assert err <= fc.ORACLE_TOL, err


def test_the_two_references_keep_the_aliasing_of_the_own_grid():
    """an under-dealiased case on a wider grid (what the stage returned before it asked) is far from both references, an
    alias-free one is not: the references can tell the two apart"""
    for N, M, wide, far in ((128, 128, 256, True), (320, 256, 384, True), (192, 128, 256, False)):
        c = fc._case(N, M, 5, "grad", N, fc.WG)
        a, b = fc.inputs(c)
        own = fc.oracle(c, a, b)
        other = fc.oracle(c._replace(N=wide), a, b)
        ref = fc.longdouble_reference(c, a, b, np.arange(5))
        assert fc.per_line_error(own, ref) <= fc.ORACLE_TOL
        if far:
            assert fc.rel(other, own) > 0.3 and fc.per_line_error(other, ref) > 0.3
        else:
            assert fc.rel(other, own) < 1e-14


def test_selection_widens_only_alias_free_plans():
    """over every 16 <= M <= N <= 1024, M even: the internal grid differs from N only if N > 3 kmax(N, M), and is then the
    smallest wave size that is at least N and greater than 3 kmax"""
    import ctypes as C

    from dedalus_amd import libhip
    lib = libhip.load()
    info = (C.c_int * 9)()
    widened = 0
    for N in range(16, 1025):
        for M in range(16, N + 1, 2):
            assert lib.ddh_rfft_fused_plan_info(N, M, 5, info) == 0
            K = fc.kmax(N, M)
            if info[0] != N:
                widened += 1
                assert N > 3 * K, (N, M, info[0])
                assert info[0] == min(s for s in fc.WAVE_SIZES if s >= N and s > 3 * K), (N, M, info[0])
                assert info[1] != fc.WG
            assert info[0] == fc.internal_grid(N, M), (N, M, info[0])
            assert (info[1] == fc.WG) == (info[0] not in fc.WAVE_SIZES)
    assert widened > 1000
    # bad arguments are errors, not a selection
    assert lib.ddh_rfft_fused_plan_info(128, 127, 5, info) != 0 and lib.ddh_rfft_fused_plan_info(128, 128, 0, info) != 0
    assert lib.ddh_rfft_fused_plan_info(128, 128, 5, None) != 0 and lib.ddh_rfft_fused_plan_info(2048, 128, 5, info) != 0


@pytest.mark.parametrize("case", fc.CASES, ids=CASE_IDS)
def test_each_case_reports_the_selection_of_its_row(case):
    got = fc.assert_selection(case)
    if case.family == fc.GW2:
        assert got["dma"] == 1 and got["twreg"] == 1
    if case.family == fc.GW:
        assert got["dma"] == 0 and got["twreg"] == int(case.C == 6 and case.NT == 4)


# ---- end to end -------------------------------------------------------------------------------------------------------
def test_dealias1_box_on_the_oracle_executor_matches_the_reference(golden_dir):
    """the golden end state (the unmodified reference, tools/make_golden_fused_dealias1.py) is reached by this package on
    the oracle executor, through a fused stage of 128 modes on 128 points, under the bounds tests/test_gpu_ivp.py uses for
    RK222 end states (problems.SCHEME_TOL holds the same figures)"""
    import dedalus_amd.public as d3
    from oracle.np_executor import NumpyExecutor
    from problems import SCHEME_TOL as TOL
    gold = np.load(os.path.join(golden_dir, fc.E2E_GOLDEN))
    ex = NumpyExecutor()
    specs = []
    inner = ex.rfft_bilinear_fused

    def spy(spec, *args, **kw):
        specs.append(tuple(spec))
        return inner(spec, *args, **kw)
    ex.rfft_bilinear_fused = spy
    solver, start, end = fc.run_dealias1(d3, dist_kw=dict(executor=ex))
    assert specs and set(specs) == {fc.E2E_SPEC}
    for k, v in end.items():
        assert np.isfinite(v).all()
        assert fc.rel(v, gold[k]) < TOL.get(k, 1e-10), (k, fc.rel(v, gold[k]))
    for k in ("b", "u"):
        assert fc.rel(start[k], gold[k]) > 1e-3          # the run moved the state
