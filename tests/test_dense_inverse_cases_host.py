"""CPU: the inputs and references of tests/dense_inverse_cases.py are what tests/test_gpu_dense_inverse_kernels.py takes
them for -- conditioning under the cap, references that solve their systems in longdouble (and, where both exist, the
Woodbury formula and the elimination agree), float64 LAPACK close to them, the kernel instance each case selects, row
interchanges where the kernels' blocked pivoting can go wrong, every listed size and every mask pattern present."""
import numpy as np
import pytest

import dense_inverse_cases as dc


def live(systems):
    return [s for s in systems if s.nv > 0]


@pytest.mark.parametrize("name", list(dc.CASES))
def test_inputs_and_references(name):
    for s in dc.case(name):
        # nothing but the valid block is finite
        inside = np.zeros((s.n, s.n), bool)
        inside[np.ix_(s.rv, s.cv)] = True
        for A in (s.M, s.L):
            assert np.isnan(A[~inside]).all() and np.isfinite(A[inside]).all()
            assert A.dtype == (np.complex128 if s.cx else np.float64)
        assert s.family == ("random" if s.n <= dc.RANDOM_MAX else "structured")
        if s.nv == 0:
            continue
        for a, b in dc.AB_PAIRS:
            cond = np.linalg.cond(s.A64(a, b))
            assert cond <= dc.COND_CAP, (name, s.n, a, b, cond)
            res = dc.residual(s, a, b)
            assert res <= 1e-16, (name, s.n, a, b, res)
            err, scale = dc.lapack_error(s, a, b)
            assert err <= 1e-12, (name, s.n, a, b, err)
            if s.parts is not None:
                perm, d1, _, _, d2, _, _ = s.parts
                assert np.abs(a * d1 + b * d2).min() >= 0.25


@pytest.mark.parametrize("n,cx", [(64, False), (129, False), (64, True), (129, True)])
def test_woodbury_agrees_with_the_elimination(n, cx):
    """The elimination's own forward error is cond * 1e-19 (1.5e-17 of max |X| at n = 64 real, cond 1.7e3): it takes one
    Newton step with an exact residual (the systems are dyadic) before the Woodbury result, as the cases use it, is
    compared with it at 1e-17.  Measured: <= 4.7e-18 on these four systems."""
    s = dc.structured_check_system(n, cx)
    for a, b in dc.AB_PAIRS:
        X = dc.woodbury_inverse(s.parts, a, b)
        A = dc.combine(s.Mv, s.Lv, a, b)
        Y, zero = dc.ld_inverse(A)
        assert zero is None
        Y = dc.ld_refine_dyadic(A, Y)
        assert np.array_equal(dc.ld_refine_dyadic(A, Y), Y)            # a fixed point: nothing left to gain
        assert float(np.abs(X - Y).max()) <= 1e-17 * float(np.abs(Y).max()), (n, cx, a, b)
        assert np.linalg.cond(s.A64(a, b)) <= dc.COND_CAP


def test_kernel_instances_and_their_lds():
    assert dc.expected_bs(768, False) == 12
    assert dc.expected_bs(769, False) == 8 and dc.expected_bs(1024, False) == 8
    assert dc.expected_bs(1, True) == 4 and dc.expected_bs(765, True) == 4 and dc.expected_bs(1024, True) == 4
    assert dc.lds_bytes(768, False) == 153600 + 4296
    assert dc.lds_bytes(1024, False) == 139264 + 4296
    assert dc.lds_bytes(1024, True) == 147456 + 4296
    want = {"real bs12 small": "real bs12", "real bs12 768": "real bs12", "real bs8 769": "real bs8", "real bs8 1024": "real bs8",
            "complex small": "complex", "complex 765": "complex", "complex 1024": "complex", "real multi 1025": "real multi",
            "real multi 1088": "real multi", "complex multi 1040": "complex multi"}
    for name, (cx, systems) in dc.CASES.items():
        assert dc.instance(name)[0] == want[name]
        small = [n for n, _ in systems if n <= dc.DI_NMAX]
        assert dc.lds_bytes(max(small), cx) <= dc.LDS_CU, name
    assert 1040 % dc.BIG_BS == 0 and 1088 % dc.BIG_RW == 0 and 1088 % dc.BIG_BS == 0 and 1025 % dc.BIG_BS == 1


def test_every_listed_size_and_mask_pattern_occurs():
    seen = {k: set() for k in dc.REQUIRED_N}
    for name, (cx, systems) in dc.CASES.items():
        label = dc.instance(name)[0]
        seen[label].update(n for n, pat in systems if pat != "N")
        pats = [pat for n, pat in systems if n > 0]
        assert set(pats) == set("ASFLN") and pats.count("N") == 1, name
        ns = [n for n, _ in systems]
        assert 0 in ns[1:-1], name                                       # an empty system between live ones
        if max(ns) > dc.DI_NMAX:
            k = ns.index(max(ns))
            assert k >= 2 and len(ns) - 1 - k >= 2, name                   # two small systems before and after the large one
        for s in dc.case(name):
            rows, cols = np.flatnonzero(~s.rv), np.flatnonzero(~s.cv)
            if s.pattern == "A":
                assert rows.size == 0 and cols.size == 0
            elif s.pattern == "S":
                assert 0 < rows.size == cols.size < s.n and rows.size == max(1, round(0.15 * s.n))
            elif s.pattern == "F":
                assert list(rows) == [0] and list(cols) == [s.n - 1]
            elif s.pattern == "L":
                assert list(rows) == [s.n - 1] and list(cols) == [0]
            else:
                assert s.nv == 0 and 0 < s.n <= 16
    for label, need in dc.REQUIRED_N.items():
        assert set(need) <= seen[label], (label, set(need) - seen[label])


@pytest.mark.parametrize("name", list(dc.CASES))
def test_pivot_coverage(name):
    """LAPACK's interchanges on the valid blocks: in most columns, from beyond the current block of pending updates, and
    at a step s > 0 inside a block (the kernel then has to exchange the pending u entries of the two rows)"""
    bs = dc.instance(name)[1]
    beyond = inside = False
    for s in live(dc.case(name)):
        for a, b in dc.AB_PAIRS:
            piv = dc.getrf_pivots(s.A64(a, b))
            k = np.arange(s.nv)
            moved = piv != k
            if s.n >= 16:
                assert moved.sum() >= s.nv / 2, (name, s.n, a, b, int(moved.sum()))
            k0 = (k // bs) * bs
            beyond = beyond or bool(np.any(moved & (piv >= k0 + bs)))
            inside = inside or bool(np.any(moved & (k > k0)))
    assert beyond and inside, (name, beyond, inside)


@pytest.mark.parametrize("name", list(dc.SINGULAR_SETS))
def test_singular_sets(name):
    cx, systems, bad, how = dc.SINGULAR_SETS[name]
    sset = dc.singular_set(name)
    (a0, b0), (a1, b1) = dc.SINGULAR_PAIRS
    for i, s in enumerate(sset):
        if i == bad:
            assert s.singular == how
            X, zero = dc.ld_inverse(dc.combine(s.Mv, s.Lv, a0, b0), want_inverse=False)
            assert zero is not None, (name, "no exact zero pivot")
            assert np.linalg.matrix_rank(s.A64(a0, b0)) == s.nv - 1
            pairs = ((a1, b1),)
        else:
            assert s.singular is None
            pairs = dc.SINGULAR_PAIRS
        for a, b in pairs:
            assert np.linalg.cond(s.A64(a, b)) <= dc.COND_CAP, (name, i, a, b)
            assert dc.residual(s, a, b) <= 1e-16
            assert dc.lapack_error(s, a, b)[0] <= 1e-12
    assert max(n for n, _ in systems) > dc.DI_NMAX if "multi" in name else max(n for n, _ in systems) <= dc.DI_NMAX


def test_gemm_chain_inputs():
    for nm, nl, nr, ncomp in dc.GEMM_SHAPES:
        assert nr % dc.EG_K == 0 and (ncomp * nr) % dc.EG_M == 0              # the device-resident GEMM path takes them
        (f0, f1, f2), x, y0 = dc.gemm_inputs(nm, nl, nr, ncomp)
        livem = dc.live_slots(nm, nl)
        assert np.isnan(x[:, ~livem]).all() and np.isfinite(x[:, livem]).all() and np.isfinite(y0).all()
        nz = lambda f: (f.reshape(nl, ncomp, nr, ncomp, nr) != 0).any(axis=(2, 4))          # [ell][co][ci]
        if ncomp > 1:
            assert not nz(f0)[:, 0, 1].any() and nz(f1)[:, 0, 1].all()
            assert not nz(f0)[:-1, 1, 0].any() and nz(f0)[-1, 1, 0]
            assert nz(f0)[:, 0, 0].all() and not nz(f1)[:, 0, 0].any()
            assert not nz(f2)[:, ncomp - 1, :].any() and nz(f2)[:, 0, 0].all()
        ref = dc.gemm_references(nm, nl, nr, ncomp)[0]
        assert np.all(ref[:, ~livem] == 0) and np.isfinite(ref).all()
    tiles = lambda nm: -(-2 * nm // dc.EG_N)
    assert [tiles(s[0]) for s in dc.GEMM_SHAPES] == [2, 1, 1]
    assert 2 * 66 - dc.EG_N == 4                                              # columns of the second tile inside 2 nm
    nm, nl, nr, ncomp = dc.CHAIN_SHAPE
    for l, s in enumerate(dc.chain_systems()):
        assert s.n == ncomp * nr and s.pattern == dc.CHAIN_GROUPS.get(l, "N")
    assert [s.n for s in dc.sphere_systems()] == [21, 18, 15, 12, 9]
    for s in live(dc.chain_systems()) + live(dc.sphere_systems()):
        for a, b in dc.AB_PAIRS:
            assert np.linalg.cond(s.A64(a, b)) <= dc.COND_CAP
            assert dc.residual(s, a, b) <= 1e-16
            assert dc.lapack_error(s, a, b)[0] <= 1e-12
