"""GPU: the modal solve kernel of dedalus_amd/csrc/ddh_modal.hip alone, through the C ABI (ddh_modal_create /
ddh_pencil_solve_modal), against numpy.longdouble solves of the same systems assembled on the host from the same symbol
term list (dedalus_amd/core/modal.py::ModalPlan.dense).

Bound per case, not taken from the kernel's output (u = 2^-53): with e(cell) = max |x - x_ld| / max |x_ld| over the
8 rc reals of a cell, max_cells e(kernel) <= max(4 max_cells e(LAPACK), 8 rc u), LAPACK = numpy.linalg.solve in float64 on
the float64 assembly of the same systems, mapped to the real parts like the kernel's.  The factor 4 is a first margin for
the different elimination order; the assembly is common to both.
Right-hand sides are NaN wherever no valid mode lives (msin slots of wavenumber 0, components without a mode in the cell,
guard rows), the solution vector lies between NaN guard regions and is prefilled with 7.0: no NaN may reach a valid
output, slots without a mode are written as +0.0, guard rows keep 7.0 and the guard regions stay NaN.
With DDH_MODAL_PARITY_OUT=<file> the figures per case are written there (profiles/modal_kernel_parity.txt)."""
import ctypes as C
import os

import numpy as np
import pytest

from dedalus_amd.core.modal import ModalPlan

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
RECORD = []
SHAPES = [(4, 4, 2), (16, 16, 8), (12, 20, 6)]
RCS = [1, 2, 5, 8]
CASES = [(rc, shape, tiled) for rc in RCS for shape in SHAPES for tiled in ((False, True) if shape == (16, 16, 8) else (False,))]


@pytest.fixture(scope="module", autouse=True)
def parity_record():
    yield
    path = os.environ.get("DDH_MODAL_PARITY_OUT")
    if path:
        with open(path, "w") as fh:
            fh.write("# tests/test_gpu_modal_kernel.py: max over cells of max |x - x_ld| / max |x_ld| (8 rc reals of a cell) of the\n")
            fh.write("# modal kernel beside numpy.linalg.solve (float64) on the same systems; both against the longdouble solution\n")
            fh.write("%-40s %10s %10s %8s\n" % ("# case", "err", "err_lapack", "ratio"))
            for row in RECORD:
                fh.write("%-40s %10.2e %10.2e %8.2f\n" % row)


@pytest.fixture(scope="module")
def ex():
    from dedalus_amd.executor import HipExecutor
    return HipExecutor()


def make_plan(rc, shape, seed, zero_diagonal=False):
    """Random symbol term list: exponents 0 .. 2 along every axis, mean-mode flags, terms of M and of L; component rows in
    scrambled order with guard rows between them."""
    nx, ny, nz = shape
    rng = np.random.default_rng(seed)
    axes = np.full(rc, 7, dtype=np.uint8)
    if rc >= 2:
        axes[rc - 1] = 0                        # a tau variable: one mode in the whole box
    if rc >= 5:
        axes[rc - 2] = 4                        # a horizontally uniform profile
        axes[rc - 3] = 3                        # no z basis
    order_r, order_x = rng.permutation(rc), rng.permutation(rc)
    lens = np.where(axes & 4, nz, 1)

    def rows(order):
        first = np.zeros(rc, dtype=np.int32)
        r = 1                                   # (row 0: a guard row)
        for k in order:
            first[k] = r
            r += lens[k] + 1                    # (+ a guard row after every component)
        return first, r
    rhs_row, nr = rows(order_r)
    x_row, nxr = rows(order_x)
    ti, tj, coef, exs, eys, ezs, fl = [], [], [], [], [], [], []
    for i in range(rc):
        for j in range(rc):
            if i == j and not (zero_diagonal and i == 0):
                ti.append(i); tj.append(j); coef.append(rc + 2.0); exs.append(0); eys.append(0); ezs.append(0); fl.append(0)
            if i == j and zero_diagonal and i == 0:
                continue
            if rng.random() < 0.7:
                for _ in range(int(rng.integers(1, 3))):
                    ti.append(i); tj.append(j)
                    coef.append(complex(rng.normal(), rng.normal()))
                    exs.append(int(rng.integers(0, 3))); eys.append(int(rng.integers(0, 3))); ezs.append(int(rng.integers(0, 3)))
                    flags = sum(int(rng.random() < 0.15) << b for b in range(3)) | (int(rng.random() < 0.5) << 3)
                    fl.append(flags)
    if zero_diagonal and rc > 1:                # (row 0 and column 0 keep the system regular through their off-diagonals)
        for (i, j) in ((0, 1), (1, 0)):
            ti.append(i); tj.append(j); coef.append(3.0 + 1.0j); exs.append(0); eys.append(0); ezs.append(0); fl.append(0)
    kx, ky, kz = 0.3 * np.arange(nx // 2), 0.25 * np.arange(ny // 2), 0.5 * np.arange(nz // 2)
    return ModalPlan(rc, nx, ny, nz, kx, ky, kz, rhs_row, x_row, axes, ti, tj, coef, exs, eys, ezs, fl, nr, nxr)


def slot_valid(plan):
    """bool [rc][2 ncz][nx][ny] (z slot index 2 mz + part; components without z: slot 0 only): does a mode live there?"""
    nx, ny, nz = plan.nx, plan.ny, plan.nz
    ok = np.zeros((plan.rc, nz, nx, ny), dtype=bool)
    for k in range(plan.rc):
        ax = int(plan.axes[k])
        for zi in range(nz if ax & 4 else 1):
            mz, pz = zi // 2, zi % 2
            for ix in range(nx):
                mx, px = ix // 2, ix % 2
                for iy in range(ny):
                    my, py = iy // 2, iy % 2
                    comp = (mx == 0 or ax & 1) and (my == 0 or ax & 2) and (mz == 0 or ax & 4)
                    ok[k, zi, ix, iy] = comp and not (px and mx == 0) and not (py and my == 0) and not (pz and mz == 0)
    return ok


def to_systems(v, dtype):
    """[rc][nz][nx][ny] reals (zero where no mode lives) -> W [ncz][ncx][ncy][sx][sz][rc]"""
    cc, cs, sc, ss = v[:, :, 0::2, 0::2], v[:, :, 0::2, 1::2], v[:, :, 1::2, 0::2], v[:, :, 1::2, 1::2]
    P = (cc - ss) + 1j * (cs + sc)
    Q = (cc + ss) + 1j * (cs - sc)
    out = np.zeros((P.shape[1] // 2, P.shape[2], P.shape[3], 2, 2, P.shape[0]), dtype=dtype)
    for sx, T in ((0, P), (1, Q)):
        Tc, Ts = T[:, 0::2], T[:, 1::2]
        out[:, :, :, sx, 0, :] = np.moveaxis(Tc + 1j * Ts, 0, -1)
        out[:, :, :, sx, 1, :] = np.moveaxis(Tc - 1j * Ts, 0, -1)
    return out


def from_systems(X):
    """inverse of to_systems: -> [rc][nz][nx][ny] reals"""
    ncz, ncx, ncy, _, _, rc = X.shape
    real = X.real.dtype
    v = np.zeros((rc, 2 * ncz, 2 * ncx, 2 * ncy), dtype=real)
    T = {}
    for sx in (0, 1):
        Xp, Xm = np.moveaxis(X[:, :, :, sx, 0, :], -1, 0), np.moveaxis(X[:, :, :, sx, 1, :], -1, 0)
        Tc, Ts = (Xp + Xm) / 2, (Xp - Xm) / 2j
        full = np.zeros((rc, 2 * ncz, ncx, ncy), dtype=X.dtype)
        full[:, 0::2], full[:, 1::2] = Tc, Ts
        T[sx] = full
    P, Q = T[0], T[1]
    v[:, :, 0::2, 0::2] = (P.real + Q.real) / 2
    v[:, :, 0::2, 1::2] = (P.imag + Q.imag) / 2
    v[:, :, 1::2, 0::2] = (P.imag - Q.imag) / 2
    v[:, :, 1::2, 1::2] = (Q.real - P.real) / 2
    return v


def batched_solve_ld(A, w):
    """Gaussian elimination with partial pivoting in numpy.clongdouble, A [B][n][n], w [B][n]"""
    A, w = A.copy(), w.copy()
    B, n, _ = A.shape
    idx = np.arange(B)
    for k in range(n):
        p = k + np.argmax(np.abs(A[:, k:, k]), axis=1)
        Ak, Ap = A[idx, k].copy(), A[idx, p].copy()
        A[idx, k], A[idx, p] = Ap, Ak
        wk, wp = w[idx, k].copy(), w[idx, p].copy()
        w[idx, k], w[idx, p] = wp, wk
        for i in range(k + 1, n):
            m = A[:, i, k] / A[:, k, k]
            A[:, i, k:] -= m[:, None] * A[:, k, k:]
            w[:, i] -= m * w[:, k]
    x = np.zeros_like(w)
    for k in range(n - 1, -1, -1):
        x[:, k] = (w[:, k] - np.einsum("bj,bj->b", A[:, k, k + 1:], x[:, k + 1:])) / A[:, k, k]
    return x


_REF = {}


def reference(rc, shape, zero_diagonal=False):
    """(plan, rhs values [rc][nz][nx][ny] float64 (zero where no mode lives), valid mask, longdouble and LAPACK real parts)"""
    key = (rc, shape, zero_diagonal)
    if key in _REF:
        return _REF[key]
    plan = make_plan(rc, shape, seed=100 * rc + shape[1] + (7 if zero_diagonal else 0), zero_diagonal=zero_diagonal)
    a, b = 1.0, 0.37
    ok = slot_valid(plan)
    rng = np.random.default_rng(5 + rc)
    vals = np.where(ok, rng.normal(size=ok.shape), 0.0)
    ncz, ncx, ncy = plan.nz // 2, plan.nx // 2, plan.ny // 2
    Ald = np.zeros((ncz, ncx, ncy, 2, 2, rc, rc), dtype=np.clongdouble)
    A64 = np.zeros(Ald.shape, dtype=np.complex128)
    for mz in range(ncz):
        for mx in range(ncx):
            for my in range(ncy):
                for sx in (0, 1):
                    for sz in (0, 1):
                        sg = (1 - 2 * sx, 1 - 2 * sz)
                        Ald[mz, mx, my, sx, sz] = plan.dense(a, b, mx, my, mz, sg[0], sg[1], dtype=np.clongdouble)
                        A64[mz, mx, my, sx, sz] = plan.dense(a, b, mx, my, mz, sg[0], sg[1])
    Wld = to_systems(vals.astype(np.longdouble), np.clongdouble)
    W64 = to_systems(vals, np.complex128)
    valid = np.zeros(Wld.shape, dtype=bool)
    for mz in range(ncz):
        for mx in range(ncx):
            for my in range(ncy):
                valid[mz, mx, my] = plan.valid(mx, my, mz)
    Wld[~valid] = 0
    W64[~valid] = 0
    Xld = batched_solve_ld(Ald.reshape(-1, rc, rc), Wld.reshape(-1, rc)).reshape(Wld.shape)
    X64 = np.linalg.solve(A64.reshape(-1, rc, rc), W64.reshape(-1, rc)[..., None])[..., 0].reshape(W64.shape)
    xld = np.where(ok, from_systems(Xld), 0)
    x64 = np.where(ok, from_systems(X64), 0.0)
    _REF[key] = (plan, a, b, vals, ok, xld, x64)
    return _REF[key]


def tile(row):
    nx, ny = row.shape
    return np.ascontiguousarray(row.reshape(nx // 8, 8, ny // 8, 8).transpose(0, 2, 1, 3)).reshape(nx, ny)


def untile(row):
    nx, ny = row.shape
    return np.ascontiguousarray(row.reshape(nx // 8, ny // 8, 8, 8).transpose(0, 2, 1, 3)).reshape(nx, ny)


def pack_rows(plan, first, nrows, vals, ok, fill, tiled):
    """vector [nrows][nx][ny]: `fill` everywhere, the components' values where a mode lives (NaN-poisoned elsewhere)"""
    v = np.full((nrows, plan.nx, plan.ny), fill)
    for k in range(plan.rc):
        n = plan.nz if plan.axes[k] & 4 else 1
        v[first[k]:first[k] + n] = np.where(ok[k, :n], vals[k, :n], fill)
    if tiled:
        v = np.stack([tile(r) for r in v])
    return v


def run_kernel(ex, plan, a, b, rhs_list, alphas, tiled, pad=6):
    from dedalus_amd import libhip
    modal = ex.make_modal(plan)
    n = plan.nrows_x * plan.nx * plan.ny
    buf = ex.dev.empty(n + 2 * pad)
    buf.fill_(float("nan"))
    x = buf[pad:pad + n]
    x.fill_(7.0)
    count0, count1 = C.c_long(0), C.c_long(0)
    libhip.call("ddh_modal_launches", C.byref(count0))
    modal.solve(a, b, [ex.from_host(r) for r in rhs_list], alphas, x, rhs_tiled=tiled, x_tiled=tiled)
    ex.sync()
    libhip.call("ddh_modal_launches", C.byref(count1))
    assert count1.value == count0.value + 1
    out = np.array(ex.download(buf)).reshape(-1)
    assert np.isnan(out[:pad]).all() and np.isnan(out[pad + n:]).all(), "the guard regions around x were written"
    xs = out[pad:pad + n].reshape(plan.nrows_x, plan.nx, plan.ny)
    if tiled:
        xs = np.stack([untile(r) for r in xs])
    return xs


def unpack(plan, xs):
    """-> ([rc][nz][nx][ny] component values, bool mask of the rows no component names)"""
    v = np.zeros((plan.rc, plan.nz, plan.nx, plan.ny))
    named = np.zeros(plan.nrows_x, dtype=bool)
    for k in range(plan.rc):
        n = plan.nz if plan.axes[k] & 4 else 1
        v[k, :n] = xs[plan.x_row[k]:plan.x_row[k] + n]
        named[plan.x_row[k]:plan.x_row[k] + n] = True
    return v, ~named


def cell_error(x, xld, rc):
    """max over cells of max |x - x_ld| / max |x_ld| (the 8 rc reals of a cell)"""
    d = np.abs(x.astype(np.longdouble) - xld)
    r, nz, nx, ny = d.shape
    cells = lambda q: q.reshape(r, nz // 2, 2, nx // 2, 2, ny // 2, 2).transpose(1, 3, 5, 0, 2, 4, 6).reshape(nz // 2, nx // 2, ny // 2, -1)
    num, den = cells(d).max(axis=-1), cells(np.abs(xld)).max(axis=-1)
    return float((num / np.maximum(den, np.longdouble(1e-300))).max())


def check(label, ex, rc, shape, tiled, zero_diagonal=False):
    plan, a, b, vals, ok, xld, x64 = reference(rc, shape, zero_diagonal)
    rhs = pack_rows(plan, plan.rhs_row, plan.nrows_rhs, vals, ok, float("nan"), tiled)
    xs = run_kernel(ex, plan, a, b, [rhs], [1.0], tiled)
    x, guard = unpack(plan, xs)
    assert not np.isnan(x).any(), "NaN in x: a slot without a mode was read"
    assert (xs[guard] == 7.0).all(), "a row no component names was written"
    dead = ~ok
    for k in range(rc):
        if not plan.axes[k] & 4:
            dead[k, 1:] = False                 # (rows that do not exist)
    assert (x[dead] == 0.0).all() and not np.signbit(x[dead]).any(), "slots without a mode must hold +0.0"
    err, err_l = cell_error(x, xld, rc), cell_error(x64, xld, rc)
    RECORD.append((label, err, err_l, err / max(err_l, 1e-300)))
    print("%s: err %.2e lapack %.2e" % (label, err, err_l))
    assert err <= max(4 * err_l, 8 * rc * U), (label, err, err_l)


@pytest.mark.parametrize("rc,shape,tiled", CASES)
def test_modal_kernel_against_longdouble(ex, rc, shape, tiled):
    check("rc%d %dx%dx%d %s" % ((rc,) + shape + ("tiled" if tiled else "natural",)), ex, rc, shape, tiled)


@pytest.mark.parametrize("rc", [5, 8])
def test_zero_leading_diagonal_needs_the_pivoting(ex, rc):
    plan = reference(rc, (12, 20, 6), True)[0]
    assert not ((plan.ti == 0) & (plan.tj == 0)).any()
    check("rc%d 12x20x6 zero diagonal" % rc, ex, rc, (12, 20, 6), False, zero_diagonal=True)


def test_right_hand_side_terms_are_combined_in_the_load(ex):
    """two terms with weights 1 and 0.5 (every product exact): bit for bit the solve of the combined vector"""
    plan, a, b, vals, ok, xld, x64 = reference(5, (12, 20, 6))
    rng = np.random.default_rng(3)
    v2 = np.where(ok, rng.normal(size=ok.shape), 0.0)
    r1 = pack_rows(plan, plan.rhs_row, plan.nrows_rhs, vals, ok, float("nan"), False)
    r2 = pack_rows(plan, plan.rhs_row, plan.nrows_rhs, v2, ok, float("nan"), False)
    both = pack_rows(plan, plan.rhs_row, plan.nrows_rhs, vals + 0.5 * v2, ok, float("nan"), False)
    x2 = run_kernel(ex, plan, a, b, [r1, r2], [1.0, 0.5], False)
    x1 = run_kernel(ex, plan, a, b, [both], [1.0], False)
    again = run_kernel(ex, plan, a, b, [r1, r2], [1.0, 0.5], False)
    assert np.array_equal(x1, x2) and np.array_equal(x2, again)


def test_refusals_launch_nothing(ex):
    from dedalus_amd import libhip
    plan = reference(2, (12, 20, 6))[0]
    rhs = pack_rows(plan, plan.rhs_row, plan.nrows_rhs, np.zeros((2, 6, 12, 20)), np.zeros((2, 6, 12, 20), bool), 0.0, False)
    n0, n1 = C.c_long(0), C.c_long(0)
    libhip.call("ddh_modal_launches", C.byref(n0))
    modal = ex.make_modal(plan)
    x = ex.dev.empty(plan.nrows_x * 12 * 20)
    with pytest.raises(libhip.DdhError, match="multiples of 8"):
        modal.solve(1.0, 1.0, [ex.from_host(rhs)], [1.0], x, rhs_tiled=True)
    with pytest.raises(libhip.DdhError, match="right-hand-side terms"):
        modal.solve(1.0, 1.0, [ex.from_host(rhs)] * 9, [1.0] * 9, x)
    bad = ModalPlan(9, 12, 20, 6, plan.kx, plan.ky, plan.kz, [0] * 9, [0] * 9, [0] * 9, [], [], [], [], [], [], [], 9, 9)
    with pytest.raises(libhip.DdhError, match="component rows"):
        ex.make_modal(bad)
    libhip.call("ddh_modal_launches", C.byref(n1))
    assert n1.value == n0.value
