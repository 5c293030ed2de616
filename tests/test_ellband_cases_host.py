"""CPU: the inputs and references of tests/ellband_cases.py that tests/test_gpu_ellband_kernels.py runs the band LU
kernels against.  The synthetic systems are within the condition cap, LAPACK's band LU interchanges rows in most of their
columns and reaches offset kl, the longdouble reference and the LAPACK baseline agree, the baseline is backward stable,
the expected windows follow the selection rule, and the index map of ddh_ellband_gather_complex_inverse is the inverse.

Why the GPU test does not recover the kernel's y by inverting P: with 16 super diagonals of 0.3 normal entries |P^-1| is
~1e3 at n = 300, and that factor multiplies the float64 rounding of z.  LAPACK's own z (kl11_ku14, a = 1, b = 0.37), sent
through the longdouble inverse of P, shows eta = 1.7e-13 against eta = 9.5e-17 of the y it came from.  The last test
here pins that, and that the y of a plan equals the solution of its twin without P, which is what the GPU test uses."""
import numpy as np
import pytest

import ellband_cases as ec


@pytest.mark.parametrize("name,layout", ec.CASE_LAYOUTS)
def test_systems_are_within_the_condition_cap_and_pivot_in_most_columns(name, layout):
    plan, nslots, lim = ec.get_case(name, layout)
    kl = plan.kl
    assert (lim >= 0).all() and (lim <= nslots).all()
    for g in range(plan.nl):
        n = int(plan.n[g])
        assert np.isnan(plan.MB[g, n:]).all() and np.isnan(plan.LB[g, n:]).all() and np.isnan(plan.P[g, n:]).all()
        if n == 0:
            continue
        col = np.arange(n)[:, None] - kl + np.arange(kl + plan.ku + 1)[None, :]
        outside = (col < 0) | (col >= n)
        assert np.all(plan.MB[g, :n][outside] == 0) and np.all(plan.LB[g, :n][outside] == 0)
        reach = np.arange(n)[:, None] + 1 + np.arange(plan.P.shape[2])[None, :] >= n
        assert np.all(plan.P[g, :n][reach] == 0)
        assert sorted(plan.row_index[g, :n]) == sorted(set(plan.row_index[g, :n])) and plan.row_index[g, :n].max() < plan.ncomp * plan.nr
        assert sorted(plan.col_index[g, :n]) == sorted(set(plan.col_index[g, :n])) and (plan.row_index[g, n:] == -1).all()
        k = int(plan.nbc_of[g])
        assert k == min(plan.nbc, n) and np.allclose(plan.T[g, :k, :k] @ plan.T[g, :k, :k].T, np.eye(k), atol=1e-14)
        for a, b in ec.AB_PAIRS:
            assert np.linalg.cond(plan.dense(g, a, b, np.float64)) <= ec.COND_CAP, (g, n, a, b)
            lu, piv, info = ec.band_lu(plan, g, a, b)
            off = ec.pivot_offsets(piv)
            assert info == 0 and off.min() >= 0
            if n >= 2 * kl and kl > 0:
                assert np.mean(off != 0) >= 0.5, (g, n, a, b)
            if n > kl:
                assert off.max() == kl, (g, n, a, b)
                if kl > 0:
                    assert off[plan.planted[g]] == kl


def test_every_edge_of_the_table_is_there():
    used = {}
    for name, (kl, ku, nw, wt, mp, nbc, nslots, ncomp, nmax, zero_n, one_n, layouts) in ec.CASES.items():
        assert ec.variant_for(kl, ku) == (nw, wt), name                     # the literals follow the rule
        used.setdefault((nw, wt), []).append((mp, nbc))
        sizes = ec.group_sizes(nw, wt, nbc, nmax)
        assert 0 in sizes[1:-1] and 1 in sizes and nw in sizes and wt in sizes and wt + 1 in sizes and nmax in sizes
        assert mp <= ec.EB_MP and nbc <= ec.EB_NBC and mp <= kl + ku
    assert sorted(used) == sorted(ec.VARIANTS) and all(len(v) >= 2 for v in used.values())
    for value in (0, 1, 16):
        assert sum(any(mp == value for mp, _ in v) for v in used.values()) >= 2
    for value in (0, 1, 8):
        assert sum(any(nbc == value for _, nbc in v) for v in used.values()) >= 2
    for variant in ((12, 24), (36, 96)):
        assert (16, 8) in used[variant] and (0, 0) in used[variant]
    assert {row[6] for row in ec.CASES.values()} == {1, 15, 17, 64, 65, 130}
    assert sum("rows_by_slots" in row[11] for row in ec.CASES.values()) == 2
    assert ec.variant_for(36, 0) is None and ec.variant_for(35, 62) is None and ec.variant_for(35, 61) == (36, 96)
    for name in ec.WIDEST:
        kl, ku, nw, wt = ec.CASES[name][:4]
        assert all(kl + ku >= r[0] + r[1] for r in ec.CASES.values() if r[2:4] == (nw, wt))
    # slot limits cut a forward wave (64 slots) and a backward wave (16) in the middle, and reach 0 and nslots
    cuts = [(int(l), nslots) for name, lay in ec.CASE_LAYOUTS for l in ec.get_case(name, lay)[2] for nslots in [ec.CASES[name][6]]]
    assert any(l % ec.FORWARD_SLOTS and l % ec.BACKWARD_SLOTS and l < ns for l, ns in cuts)
    assert any(l == 0 for l, ns in cuts) and any(l == ns == 130 for l, ns in cuts)


def test_every_size_edge_is_solved_on_every_window_variant():
    """a group with slot_limit 0 is factored but never solved: per variant, every system size of its cases has live slots
    in at least one of them -- more than one slot where a case has several, except for the one-row system (no pivot, no
    block: the size that gives up its slots where one must), and all slots on the largest system of every case -- and
    every case still has one live-sized group with slot_limit 0"""
    live = {}
    for name, row in ec.CASES.items():
        plan, nslots, lim = ec.case(name)
        variant = row[2:4]
        assert sorted(int(n) for n, l in zip(plan.n, lim) if l == 0) == [0, row[9]]
        assert lim[np.argmax(plan.n)] == nslots
        if row[10] is not None:
            assert lim[list(plan.n).index(row[10])] == 1
        for n, l in zip(plan.n, lim):
            if n:
                best = live.setdefault((variant, int(n)), [0, 0])
                best[0], best[1] = max(best[0], int(l)), max(best[1], nslots)
    for variant in ec.VARIANTS:
        nw, wt = variant
        for n in (1, nw - 1, nw, wt, wt + 1, 2 * wt + 5, 300):
            assert (variant, n) in live, (variant, n)
    for (variant, n), (l, most) in live.items():
        assert l >= (1 if n == 1 else min(2, most)), (variant, n, l)
    for name, lay in ec.CASE_LAYOUTS:
        if lay == "rows_by_slots":
            plan, nslots, lim = ec.single_group_case(name)
            assert lim[0] == nslots and plan.n[0] == 2 * ec.CASES[name][3] + 5


@pytest.mark.parametrize("name,layout", ec.CASE_LAYOUTS)
@pytest.mark.parametrize("a,b", ec.AB_PAIRS)
def test_reference_and_lapack_baseline_agree_and_the_baseline_is_backward_stable(name, layout, a, b):
    from dedalus_amd.core.ellband import EllBandPlan
    plan, nslots, lim = ec.get_case(name, layout)
    cols = ec.rhs_columns(name, layout)
    sol = ec.solved(name, layout, a, b)
    assert sorted(sol) == [g for g in range(plan.nl) if plan.n[g] and lim[g]]
    scale = max(np.abs(s["z"]).max() for s in sol.values())
    for g, s in sol.items():
        n = int(plan.n[g])
        assert np.abs(s["zb"] - s["z"]).max() <= 1e-11 * scale, g
        assert s["eta_b"] <= 1e-15, (g, s["eta_b"])
        assert ec.backward_error(plan, g, a, b, cols[g], s["y"]) <= 1e-18
        # the baseline is the body of EllBandPlan.reference_solve: the same numbers through that method
        flat = np.zeros((plan.ncomp * plan.nr, cols[g].shape[1]))
        flat[plan.row_index[g, :n]] = cols[g]
        x = EllBandPlan.reference_solve(plan, g, a, b, flat)
        assert np.array_equal(x[plan.col_index[g, :n]], s["zb"])
        rest = np.ones(len(x), bool)
        rest[plan.col_index[g, :n]] = False
        assert np.all(x[rest] == 0)


@pytest.mark.parametrize("name", ec.WIDEST)
def test_pivot_cases_have_no_interchange_and_exactly_one(name):
    plan, nslots, lim = ec.pivot_case(name)
    n = int(plan.n[0])
    for a, b in ec.AB_PAIRS:
        off = ec.pivot_offsets(ec.band_lu(plan, 0, a, b)[1])
        assert np.all(off == 0)
        off = ec.pivot_offsets(ec.band_lu(plan, 1, a, b)[1])
        assert off[n - 1 - plan.kl] == plan.kl and np.count_nonzero(off) == 1
        for g in (0, 1):
            assert np.linalg.cond(plan.dense(g, a, b, np.float64)) <= ec.COND_CAP


def test_zero_pivot_case_has_two_singular_groups():
    plan, nslots, lim, singular = ec.zero_pivot_case()
    for g in range(plan.nl):
        A = plan.dense(g, 1.0, 0.37, np.float64)
        assert (np.abs(A).sum(axis=0).min() == 0) == (g in singular)
        if g not in singular:
            assert np.linalg.cond(A) <= ec.COND_CAP


def test_layout_offsets_name_every_element_once():
    for name, layout in ec.CASE_LAYOUTS:
        plan, nslots, lim = ec.get_case(name, layout)
        rowoff, coloff, stride, size = ec.offsets(plan, nslots, layout)
        for off in (rowoff, coloff):
            named = np.concatenate([off[g, :plan.n[g], None] + np.arange(nslots)[None, :] * stride for g in range(plan.nl)], axis=None)
            assert named.min() >= 0 and named.max() < size and len(np.unique(named)) == len(named)
        if layout == "default":
            full = np.arange(size).reshape(plan.ncomp, nslots, plan.nl, plan.nr)
            g, i = plan.nl - 1, 0
            f = plan.row_index[g, i]
            assert full[f // plan.nr, 0, g, f % plan.nr] == rowoff[g, i] and stride == plan.nl * plan.nr


@pytest.mark.parametrize("R,nl,nm", [(1, 5, 5), (3, 7, 4)])
def test_gather_index_map_is_the_inverse(R, nl, nm):
    """slot (nl - 1 - ell) R + c of the unit solves holds A_m^-T e_(c, ell), components 2 cp / 2 cp + 1 its real and
    imaginary parts: gathered, that is A_m^-1"""
    rng = np.random.default_rng(R + nl)
    nslots = R * nl + 2
    x = rng.standard_normal((2 * R, nslots, nm, nl))                       # everything the map does not name: noise
    mats = []
    for m in range(nm):
        ne = nl - m
        A = rng.standard_normal((R * ne, R * ne)) + 1j * rng.standard_normal((R * ne, R * ne)) + 3 * np.eye(R * ne)
        mats.append(A)
        for c in range(R):
            for el in range(ne):
                e = np.zeros(R * ne)
                e[c * ne + el] = 1.0
                v = np.linalg.solve(A.T, e).reshape(R, ne)
                sl = (nl - 1 - (m + el)) * R + c
                x[0::2, sl, m, m:] = v.real
                x[1::2, sl, m, m:] = v.imag
    off, count = ec.gather_offsets(R, nl, nm)
    out = ec.gather_complex_inverse(x, R, nl, nm, nslots, np.full(count, np.nan + 0j))
    assert not np.isnan(out).any()
    for m in range(nm):
        k = R * (nl - m)
        inv = np.linalg.inv(mats[m])
        assert np.abs(out[off[m]:off[m] + k * k].reshape(k, k) - inv).max() <= 1e-13 * np.abs(inv).max()


def test_bordered_reference_is_the_inverse_of_the_bordered_matrix():
    M, L, j0 = ec.bordered_system()
    n = M.shape[0] - 1
    a, b = 1.0, 0.37
    A = a * M + b * L
    assert np.all(A[:n, j0] == 0) and np.linalg.cond(A) <= ec.COND_CAP
    B2 = A[:n, :n].copy()
    B2[:, j0] = A[:n, n]
    i, j = np.nonzero(B2)
    assert (i - j).max() == 5 and (j - i).max() == 6
    X = np.linalg.inv(B2)
    w = A[n, :n].copy()
    d, w[j0] = w[j0], A[n, n]
    row, mag = ec.bordered_row(X, w, 0 * w, d, 0.0, 1.0, 0.0)
    inv = np.zeros((n + 1, n + 1))
    inv[:n, :n] = X
    inv[n, :n] = X[j0]
    inv[j0] = row
    assert np.abs(inv @ A - np.eye(n + 1)).max() <= 1e-9


def test_undoing_P_amplifies_rounding_but_the_twin_plan_gives_y():
    # (on the device the same holds because ellband_backward_kernel forms y = (w + a) * sh.x without P and stores z0 + y,
    # z0 the recombination sum: with P = 0 the store is y itself -- revisit this if that kernel ever folds P into y)
    name, (a, b) = "kl11_ku14", ec.AB_PAIRS[0]
    plan, nslots, lim = ec.case(name)
    cols = ec.rhs_columns(name)
    g = plan.nl - 1
    s = ec.solved(name, "default", a, b)[g]
    eta_undone = ec.backward_error(plan, g, a, b, cols[g], ec.undo_P(plan, g, s["zb"]))
    assert eta_undone > 100 * s["eta_b"]
    assert np.abs(ec.undo_P(plan, g, s["z"]) - s["y"]).max() <= 1e-14 * np.abs(s["y"]).max()     # exact data: it is the inverse
    twin = plan.without_P()
    yt, zt = ec.baseline(twin, g, a, b, cols[g])
    assert np.array_equal(yt, s["yb"]) and np.array_equal(zt, yt) and twin.mp == plan.mp
