"""CPU: the tables of the M.X emission of the backward sweep (dedalus_amd/core/solvers.py::mx_band_tables) against a dense
scipy product of the solver's own matrices, 3-D Rayleigh-Benard at Nz = 16 and 24 on the oracle executor.

Checked: every row of M with entries gets exactly one step; the step lies in the block of the row's columns; all columns of
the row lie in [t, t + 18); the coefficients are those of M P = (dense M) (dense P) in the logical ordering; and the
analysis refuses (None) a window that is too narrow, rows that cross blocks, differing grading classes, complex or border
entries, and steps that run out.  The reference forms M.X with one sparse product (core/timesteppers.py:588-604)."""
import numpy as np
import pytest
from scipy import sparse

import problems
from dedalus_amd.core.solvers import mx_band_tables
from oracle.np_executor import NumpyExecutor


def _solver(nz):
    import dedalus_amd.public as d3
    solver, f = problems.rayleigh_benard_3d(d3, Nx=8, Ny=8, Nz=nz, dist_kw=dict(executor=NumpyExecutor()))
    return solver


def _dense(tl, R):
    assert not (np.any(tl.ex) or np.any(tl.ey) or np.any(tl.dx) or np.any(tl.dy))
    return sparse.coo_matrix((np.asarray(tl.coef), (np.asarray(tl.row), np.asarray(tl.col))), shape=(R, R)).toarray()


@pytest.mark.parametrize("nz", [16, 24])
@pytest.mark.parametrize("split", [True, False])
def test_tables_are_the_band_of_m_times_p(nz, split):
    s = _solver(nz)
    R, n = s.R, s.n_interior
    assert s.n_blocks == 2 and len(set(s.block_sizes)) == 1
    nh = s.block_sizes[0] if split else n
    tables = s.mx_band_tables(nh if split else None)
    assert tables is not None
    step_row, band = tables
    assert step_row.shape == (n,) and band.shape == (n, 18)
    MP = (_dense(s.M_tl, R) @ _dense(s.P_tl, R))
    assert np.abs(MP.imag).max() == 0
    MPl = MP.real[np.ix_(s.row_perm, s.col_perm)]              # logical ordering
    assert not MPl[n:].any() and not MPl[:, n:].any()
    scale = np.abs(MPl).max()
    with_entries = np.flatnonzero(np.abs(MPl[:n]).max(axis=1) > 0)
    placed = step_row[step_row >= 0]
    assert sorted(placed.tolist()) == with_entries.tolist()    # every row once, no other row
    assert len(with_entries) == len(np.unique(np.asarray(s.M_tl.row)))
    for t in range(n):
        i = int(step_row[t])
        if i < 0:
            assert not band[t].any()
            continue
        rebuilt = np.zeros(n)
        w = min(18, n - t)
        rebuilt[t:t + w] = band[t, :w]
        assert not band[t, w:].any()
        assert np.abs(rebuilt - MPl[i, :n]).max() <= 4e-16 * scale, (t, i)
        cols = np.flatnonzero(MPl[i, :n])
        assert cols.min() >= t and cols.max() < t + 18
        assert np.all(cols // nh == t // nh)                    # the step's thread sweeps the block of the columns


def test_analysis_refuses_what_the_sweep_cannot_form():
    s = _solver(16)
    n, nh = s.n_interior, s.block_sizes[0]
    tl = s.MP_tl.consolidated()
    rc, cc = s.real_grading["row_code"], s.real_grading["col_code"]
    args = lambda **kw: dict(dict(row=tl.row, col=tl.col, coef=tl.coef, row_perm=s.row_perm, col_perm=s.col_perm, n=n, nh=nh,
                                  row_code=rc, col_code=cc, width=18), **kw)
    assert mx_band_tables(**args()) is not None
    span = max(int(np.ptp(np.flatnonzero(r))) for r in (_dense(s.MP_tl, s.R).real[np.ix_(s.row_perm, s.col_perm)]) if r.any())
    assert mx_band_tables(**args(width=span + 1)) is not None
    assert mx_band_tables(**args(width=span)) is None                       # a row wider than the window
    assert mx_band_tables(**args(nh=7)) is None                             # rows whose columns straddle two blocks
    flipped = np.array(cc).copy()
    flipped[tl.col[0]] ^= 1
    assert mx_band_tables(**args(col_code=flipped)) is None                 # another grading class
    cplx = np.array(tl.coef).copy()
    cplx[0] += 1e-3j
    assert mx_band_tables(**args(coef=cplx)) is None                        # a complex entry
    border = np.array(tl.row).copy()
    border[0] = s.row_perm[-1]
    if s.R > n:
        assert mx_band_tables(**args(row=border)) is None                   # an entry in a border row
    # no free step: two rows with the same single column
    r0, r1 = s.row_perm[0], s.row_perm[1]
    c0 = s.col_perm[0]
    two = mx_band_tables(row=np.array([r0, r1]), col=np.array([c0, c0]), coef=np.array([1.0 + 0j, 2.0 + 0j]), row_perm=s.row_perm,
                         col_perm=s.col_perm, n=n, nh=nh, row_code=np.zeros(s.R, int), col_code=np.zeros(s.R, int), width=18)
    assert two is None
    # ... while a second column lets the wider row move down one step
    c1 = s.col_perm[1]
    ok = mx_band_tables(row=np.array([r0, r1, r1]), col=np.array([c1, c1, c0]), coef=np.array([1.0 + 0j, 2.0 + 0j, 3.0 + 0j]),
                        row_perm=s.row_perm, col_perm=s.col_perm, n=n, nh=nh, row_code=np.zeros(s.R, int),
                        col_code=np.zeros(s.R, int), width=18)
    assert ok is not None and ok[0][1] == 0 and ok[0][0] == 1 and ok[1][0, 0] == 3.0 and ok[1][0, 1] == 2.0 and ok[1][1, 0] == 1.0
