"""CPU: the inputs, references and case tables of tests/swsh_cases.py that tests/test_gpu_swsh_kernels.py runs the
kernels of dedalus_amd/csrc/ddh_swsh.hip against.  The plain references agree with the float64 oracle
(oracle/np_swsh.py, NumpyExecutor.regularity_recombine) to the bound the GPU test uses, the mode-2 construction is the
spin identity of the real SWSH matrices, the random matrices have none of the symmetries that hide index errors, and the
tables reach every launch-shape edge of every path in both directions (derived from the constants restated in the case
module, path selection from ncols and n3 only)."""
import numpy as np
import pytest

import swsh_cases as sc

U = 2.0 ** -53
UNPAIRED = [n for n, row in sc.CASES.items() if row[4] == "none"]
PAIRED = [n for n, row in sc.CASES.items() if row[4] != "none"]


def test_reference_precision_is_beyond_float64():
    """a cancellation float64 loses: extended longdouble, or the math.fsum fallback, keeps it"""
    assert sc.LD_OK == (np.finfo(np.longdouble).eps <= 2.0 ** -63)
    r, s = sc.product_and_scale(np.array([[1.0, 2.0 ** -60, -1.0]]), np.ones((3, 1)))
    assert float(r[0, 0]) == 2.0 ** -60 and r.dtype == sc.LD and 2.0 <= float(s[0, 0]) <= 2.0 + 2.0 ** -50
    saved, sc.LD_OK = sc.LD_OK, False
    try:
        rng = np.random.default_rng(1)
        A, X = rng.standard_normal((3, 70)), rng.standard_normal((2, 70, 4))
        r = sc.product_and_scale(A, X)[0]
    finally:
        sc.LD_OK = saved
    if saved:
        want, S = sc.product_and_scale(A, X)
        assert r.shape == want.shape and np.all(np.abs(r - want) <= U * S)


@pytest.mark.parametrize("name", UNPAIRED)
def test_plain_references_agree_with_the_oracle(name):
    from oracle import np_swsh
    p = sc.plan(name)
    g, c = sc.inputs(name)
    fw, bw = dict(zip(p.keys, p.fwd)), dict(zip(p.keys, p.bwd))
    f, b = sc.forward_reference(name), sc.backward_reference(name)
    cout = np.full(p.cshape, 7.0)
    np_swsh.forward_reduced(g, cout, p.groups, fw)
    assert not np.isnan(cout).any() and np.all(cout[~f["named"]] == 7.0)
    assert np.all(np.abs(cout - f["ref"])[f["named"]] <= ((f["K"] + 2) * U * f["S"])[f["named"]])
    gout = np.full(p.gshape, 7.0)
    np_swsh.backward_reduced(c, gout, p.groups, bw)
    assert not np.isnan(gout).any() and np.all(gout[~(b["named"] | b["zero"])] == 7.0) and np.all(gout[b["zero"]] == 0.0)
    assert np.all(np.abs(gout - b["ref"])[b["named"]] <= ((b["K"] + 2) * U * b["S"])[b["named"]])
    assert f["named"].any() and b["named"].any() and b["zero"].any() and (f["S"][f["named"]] > 0).all()


@pytest.mark.parametrize("name", PAIRED)
def test_paired_references_are_plain_products_of_explicit_matrices(name):
    """every pair expanded: the partner's slices hold the product of its own matrices (float64 einsum, same bound)"""
    p = sc.plan(name)
    g, c = sc.inputs(name)
    f, b = sc.forward_reference(name), sc.backward_reference(name)
    seen = 0
    for r in p.rows:
        F, B = p.matrices(r["key"])
        if r["mode"] == 0 or F is None:
            continue
        ells = r["ell_start"] + np.arange(r["n_ell"])
        if r["mode"] == 2:
            sign = (-1.0) ** (ells + r["parity"])
            F, B = sign[:, None] * F[:, ::-1], sign[None, :] * B[::-1]
        sl_g, sl_c = slice(r["gq"], r["gq"] + r["count"]), slice(r["cq"], r["cq"] + r["count"])
        want = np.einsum("lt,ajtx->ajlx", F, g[:, sl_g])
        assert np.all(np.abs(want - f["ref"][:, sl_c][:, :, ells]) <= (p.n_grid + 2) * U * f["S"][:, sl_c][:, :, ells])
        want = np.einsum("tl,ajlx->ajtx", B, c[:, sl_c][:, :, ells])
        assert np.all(np.abs(want - b["ref"][:, sl_g]) <= (r["n_ell"] + 2) * U * b["S"][:, sl_g])
        seen += 1
    assert seen >= 6


def test_inputs_are_poisoned_where_the_operation_names_nothing():
    for name in sc.CASES:
        p = sc.plan(name)
        g, c = sc.inputs(name)
        f, b = sc.forward_reference(name), sc.backward_reference(name)
        assert np.array_equal(~np.isnan(g), b["named"]) and np.array_equal(~np.isnan(c), f["named"])
        used_g, used_c = b["named"] | b["zero"], np.zeros(p.n1c, bool)
        for F, B, g0, c0, cnt, ells in p.products():
            used_c[c0:c0 + cnt] = True
        assert (~used_g.any(axis=(0, 2, 3))).sum() >= 2 and (~used_c).sum() >= 2         # slices of no group
        assert not used_g[:, 0].any() and not used_c[0]
        starts = p.groups[:, 1]
        free_g = np.flatnonzero(~used_g.any(axis=(0, 2, 3)))
        assert np.any(np.diff(starts) < 0) and np.any((free_g > 0) & (free_g < p.n1g - 1))         # unordered, with gaps
        rows = f["named"].any(axis=(0, 3))
        assert np.any(rows.any(axis=1) & ~rows.all(axis=1))                             # rows outside a group's ell range


@pytest.mark.parametrize("s", [1, 2])
def test_mode2_construction_is_the_spin_identity(s):
    """a (+s, -s) plan laid out as core/sphere.py::colatitude_plan does (group per m: ell_start = m, parity = m & 1,
    the matrices of +s): the mirrored matrices of the case module are the -s matrices"""
    from dedalus_amd.tools import sphere as sph
    N, Lmax = 36, 22
    for m in (0, 1, 2, 5, 11, 22):
        fp, bp = sph.swsh_matrices(N, Lmax, m, s)
        fm, bm = sph.swsh_matrices(N, Lmax, m, -s)
        f2, b2 = sc.mirrored(fp, bp, m, m & 1)
        assert np.abs(f2 - fm).max() < 1e-14 and np.abs(b2 - bm).max() < 1e-14
        assert np.abs(fp).max() > 0.01


def test_random_matrices_have_no_symmetry_to_hide_behind():
    def rd(a, b):
        return np.linalg.norm(a - b) / np.linalg.norm(b)
    for name in sc.CASES:
        p = sc.plan(name)
        for F, B in zip(p.fwd, p.bwd):
            if p.n_grid > 1 and F.shape[0] > 1:
                assert rd(F[:, ::-1], F) > 0.1 and rd(-F[:, ::-1], F) > 0.1 and rd(B[::-1], B) > 0.1 and rd(-B[::-1], B) > 0.1
            if F.size >= 4:
                assert rd(B.T, F) > 0.1
            if F.shape[0] > 1:
                assert rd(F[::-1], F) > 0.1 and rd(B[:, ::-1], B) > 0.1
        assert all(rd(p.fwd[i][:1, :], p.fwd[i + 1][:1, :]) > 0.1 for i in range(len(p.fwd) - 1) if p.n_grid > 3)


# ---- coverage, derived from the tables ---------------------------------------------------------------------------------
def _shapes(path):
    """per direction the (rows, K, case) of every product with a matrix on the path"""
    fwd, bwd = [], []
    for name in sc.CASES:
        p = sc.plan(name)
        if sc.path_of(p.n0 * p.max_count * p.n3, p.n3) != path:
            continue
        for r in p.rows:
            if r["n_ell"]:
                fwd.append((r["n_ell"], p.n_grid, name))
                bwd.append((p.n_grid, r["n_ell"], name))
    return {"forward": fwd, "backward": bwd}


def test_path_selection_and_required_values():
    by_path = {}
    for name, (n_grid, n0, mc, n3, pairing) in sc.CASES.items():
        path = sc.path_of(n0 * mc * n3, n3)
        assert name.startswith(path) and sc.plan(name).path == path
        by_path.setdefault(path, []).append(dict(n_grid=n_grid, n0=n0, n3=n3, ncols=n0 * mc * n3, pairing=pairing, mc=mc))
        p = sc.plan(name)
        # every case: the whole n_ell set one group each, a folded group sharing a key, a group without a matrix
        ne = sorted(r["n_ell"] for r in p.rows if r["ell_step"] == 1 and r["n_ell"])
        assert ne == sorted(sc.NELL)
        folded = [r for r in p.rows if r["ell_step"] == -1]
        assert len(folded) == 1 and sum(r["key"] == folded[0]["key"] for r in p.rows) == 2
        assert sum(r["key"] not in p.keys for r in p.rows) == 1
        assert p.n1g * p.n_grid * p.n0 * p.n3 * 8 < 8e6 and p.n1c * p.n2c * p.n0 * p.n3 * 8 < 8e6
    assert set(sc.NELL) == {1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 67}
    assert sorted(by_path) == ["gemv", "lds", "mfma"]
    for path, need in sc.REQUIRED.items():
        for key, values in need.items():
            assert values <= {row[key] for row in by_path[path]}, (path, key)
        assert any(row["mc"] == 3 for row in by_path[path]), (path, "counts 1, 2, 3 in one plan")
    assert sc.REQUIRED["gemv"]["n_grid"] == {5, 63, 64, 65, 130} and sc.REQUIRED["gemv"]["ncols"] == {1, 2, 3, 4, 5, 8}
    assert sc.REQUIRED["lds"]["ncols"] == {9, 63, 64, 65, 130} and sc.REQUIRED["lds"]["n3"] == {1, 3, 13, 15}
    assert sc.REQUIRED["lds"]["n_grid"] == {15, 16, 17, 65} and sc.REQUIRED["mfma"]["n0"] == {1, 2}
    assert sc.REQUIRED["mfma"]["n3"] == {16, 17, 63, 64, 65, 130} and sc.REQUIRED["mfma"]["n_grid"] == {3, 31, 32, 33, 65, 130}
    # the switches between the paths: ncols 8 | 9 and n3 15 | 16
    assert sc.path_of(8, 1) == "gemv" and sc.path_of(9, 1) == "lds" and sc.path_of(9, 9) == "lds"
    assert sc.path_of(45, 15) == "lds" and sc.path_of(16, 16) == "mfma" and sc.path_of(8, 8) == "gemv"
    assert any(r["ncols"] == 8 for r in by_path["gemv"]) and any(r["ncols"] == 9 for r in by_path["lds"])
    assert any(r["n3"] == 15 for r in by_path["lds"]) and any(r["n3"] == 16 for r in by_path["mfma"])
    for name in sc.ALIAS_CASES:
        assert name in sc.CASES
    assert {sc.case_path(n) for n in sc.ALIAS_CASES} == {"gemv", "lds", "mfma"}
    assert any(sc.CASES[n][4] != "none" for n in sc.ALIAS_CASES)


def test_gemv_edges():
    # every compiled width, paired and unpaired; both directions run on every case
    inst = {(sc.gemv_width(n0 * mc * n3), pairing != "none") for n_grid, n0, mc, n3, pairing in sc.CASES.values()
            if sc.path_of(n0 * mc * n3, n3) == "gemv"}
    assert inst == {(w, pr) for w in sc.GV_WIDTHS for pr in (False, True)}
    block_rows = sc.GV_ROWS * sc.GV_WAVES
    for direction, shapes in _shapes("gemv").items():
        rows, K = {s[0] for s in shapes}, {s[1] for s in shapes}
        assert {r % sc.GV_ROWS for r in rows} == set(range(sc.GV_ROWS)), direction           # ragged last wave
        assert any(r > block_rows and r % block_rows for r in rows) and any(r % block_rows == 0 for r in rows)
        assert any(r < block_rows for r in rows), direction
        assert any(k > sc.LANES and k % sc.LANES for k in K), direction                      # lanes stride K, ragged
        assert {sc.LANES - 1, sc.LANES, sc.LANES + 1} <= K and any(k < sc.LANES for k in K), direction
    # pair modes: isolated and mixed, both parities, both parities of ell_start under mode 2, a paired group without matrix
    for pairing in ("mode1", "mode2", "mixed"):
        plans = [sc.plan(n) for n in sc.CASES if sc.CASES[n][4] == pairing]
        modes = {r["mode"] for p in plans for r in p.rows if r["ell_step"] == 1}
        assert modes == {"mode1": {1}, "mode2": {2}, "mixed": {0, 1, 2}}[pairing]
        assert all(any(r["mode"] and r["key"] not in p.keys for r in p.rows) for p in plans)
        if pairing != "mode1":
            for p in plans:
                combos = {(r["parity"], r["ell_start"] % 2) for r in p.rows if r["mode"] == 2 and r["n_ell"]}
                assert {c[0] for c in combos} == {0, 1} and len(combos) >= 3, (p.name, combos)


def test_lds_gemm_edges():
    cols = {n0 * mc * n3 for n_grid, n0, mc, n3, pairing in sc.CASES.values() if sc.path_of(n0 * mc * n3, n3) == "lds"}
    assert {sc.GT_X - 1, sc.GT_X, sc.GT_X + 1} <= cols and any(c > 2 * sc.GT_X for c in cols) and min(cols) == sc.GV_COLS + 1
    for direction, shapes in _shapes("lds").items():
        rows, K = {s[0] for s in shapes}, {s[1] for s in shapes}
        assert any(r > sc.GT_I and r % sc.GT_I for r in rows) and any(r < sc.GT_I for r in rows), direction
        assert {sc.GT_J - 1, sc.GT_J, sc.GT_J + 1} <= K and any(k > 2 * sc.GT_J and k % sc.GT_J for k in K), direction
        assert {r % 8 for r in rows} >= {0, 1, 7}, direction                                 # 8 rows per thread


def test_mfma_gemm_edges():
    n3s = {n3 for n_grid, n0, mc, n3, pairing in sc.CASES.values() if sc.path_of(n0 * mc * n3, n3) == "mfma"}
    assert {sc.GM_N - 1, sc.GM_N, sc.GM_N + 1} <= n3s and any(x > 2 * sc.GM_N for x in n3s) and min(n3s) == sc.MFMA_MIN_N3
    for direction, shapes in _shapes("mfma").items():
        rows, K = {s[0] for s in shapes}, {s[1] for s in shapes}
        assert any(r > sc.GM_M for r in rows), direction                                     # blockIdx.y > 0
        # a last row tile with whole 16-row strips past nrows (the wave-uniform continue), and a ragged strip
        assert any(-(-(r % sc.GM_M) // sc.GM_STRIP) in (1, 2, 3) for r in rows if r % sc.GM_M), direction
        assert any(r % sc.GM_STRIP for r in rows) and any(r % sc.GM_STRIP == 0 for r in rows), direction
        assert {k % sc.GM_KSTEP for k in K} == set(range(sc.GM_KSTEP)), direction
        assert any(k > sc.GM_K and k % sc.GM_K for k in K) and any(k % sc.GM_K == 0 for k in K), direction
        assert any(k > 2 * sc.GM_K for k in K), direction                                    # several chunks
    fwd, bwd = _shapes("mfma")["forward"], _shapes("mfma")["backward"]
    assert {1, 3, 31} <= {k % sc.GM_K for _, k, _ in fwd}                                    # K tails forward
    assert any(-(-r // sc.GM_M) == 3 for r, _, _ in bwd)                                     # three row tiles backward
    assert {k % sc.GM_K for _, k, _ in bwd} >= {0, 1, 31}


# ---- regularity -------------------------------------------------------------------------------------------------------
def test_regularity_table_reaches_every_thread_count_edge():
    assert set(sc.REG_N3) == {1, 63, 64, 65, 128, 129, 255, 256, 257, 600} and set(sc.REG_NCOMP) == {1, 3, 9}
    T = {n3: sc.regularity_threads(n3) for n3 in sc.REG_N3}
    assert set(T.values()) == set(sc.REG_T)
    assert T[64] == 64 and T[65] == 128 and T[255] == 128 and T[256] == 256 and T[1] == 64
    for t in sc.REG_T:
        assert any(n3 == t for n3 in T if T[n3] == t) or t == 128          # a full block
    assert T[128] == 128 and any(n3 > T[n3] and n3 % T[n3] for n3 in T) and any(n3 > 2 * T[n3] for n3 in T)   # the loop
    assert any(n3 > T[n3] for n3 in T if T[n3] == 128) and any(n3 < T[n3] for n3 in T)


@pytest.mark.parametrize("ncomp", sc.REG_NCOMP)
@pytest.mark.parametrize("with_fac", [False, True])
def test_regularity_reference_agrees_with_the_oracle(ncomp, with_fac):
    from oracle.np_executor import NumpyExecutor
    ex = NumpyExecutor()
    for n3 in (1, 65, 257):
        data, slot_map, mats, fac = sc.regularity_inputs(ncomp, n3)
        assert (slot_map == -1).sum() == 4 and slot_map.max() == sc.REG_NMATS - 2 and np.isnan(mats[-1]).all()
        assert not np.isnan(fac).any() and np.all(fac != 1.0) and np.all(fac != 0.0)
        ref, S = sc.regularity_reference(data, slot_map, mats, fac if with_fac else None)
        got = data.copy()
        with np.errstate(invalid="ignore"):
            ex.regularity_recombine(got, ex.make_recombination(slot_map, mats), fac if with_fac else None)
        assert not np.isnan(got).any() and np.all(np.abs(got - ref) <= (ncomp + 2) * U * S)
        dead = slot_map == -1
        if not with_fac:
            assert np.array_equal(got[:, dead], data[:, dead]) and np.array_equal(ref[:, dead], data[:, dead].astype(sc.LD))
            if ncomp > 1:
                assert not np.array_equal(got[:, ~dead], data[:, ~dead])
