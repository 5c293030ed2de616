"""CPU: the case table of tests/transform_edge_cases.py that tests/test_gpu_transform_edges.py runs the size-generic
transform kernel against.

The double-precision oracle (oracle/np_transforms.py) stays within a tenth of the kernel's bound of the longdouble matrix
reference on every row -- per line, on the GPU test's own inputs -- which is what lets the GPU test hold all lines of the
rows above 512 points against the oracle.  The Python mirror of transform_plan gives every row the (B, T, lds) it was put
in the table to hit, and the table holds every launch shape and every path of the conversion solve the kernel has."""
import ctypes as C

import numpy as np
import pytest

import transform_edge_cases as tc


def _host_shapes(c):
    # the GPU test's contiguous three-line input (lines 0 and 2 above 512 points); below, a strided one as well
    return [(3, c.N)] if c.N > tc.BIG else [(3, c.N), (2, c.N, 19)]


@pytest.mark.parametrize("case", tc.CASES, ids=tc.CASE_IDS)
def test_oracle_is_within_a_tenth_of_the_bound_of_the_longdouble_reference(case):
    c = case
    runs = []
    for op in c.ops:
        for shape in _host_shapes(c):
            x = tc.make_input(c, op, shape)
            xl = tc.lines_of(x, c.N if op == "forward" else c.M)
            runs.append((op, shape, x, tc.compared_lines(c.N, xl.shape[1]), xl))
    refs_all = tc.reference_many(c, [(op, xl[:, pick]) for op, _, _, pick, xl in runs])
    for (op, shape, x, pick, _), refs in zip(runs, refs_all):
        for got, ref, tol in zip(tc.oracle(c, op, x), refs, tc.tolerances(c, op)):
            err = tc.line_errors(tc.lines_of(got, tc.out_axis(c, op))[:, pick], ref)
            print("%s %s %s oracle-vs-longdouble worst line %.3e (bound %.1e)" % (tc.case_id(c), op, shape, err.max(),
                                                                                 tc.ORACLE_MARGIN * tol))
            assert np.isfinite(err).all() and err.max() <= tc.ORACLE_MARGIN * tol, (op, shape, err.max())


@pytest.mark.parametrize("case", tc.CASES, ids=tc.CASE_IDS)
def test_mirror_gives_every_row_the_launch_shape_it_pins(case):
    c = case
    assert tc.factorize_mirror(c.N) is not None
    for shape in tc.shapes_for(c.N):
        outer, inner = tc.outer_inner(shape)
        p = tc.plan_mirror(c.kind, c.N, outer, inner)
        assert isinstance(p, dict), (shape, p)
        for key, want in c.expect.items():
            if key == "lds_le":
                assert p["lds"] <= want, (shape, p)
            elif key == "lds_gt":
                assert p["lds"] > want, (shape, p)
            else:
                assert p[key] == want, (shape, key, p)
        assert p["lds"] <= tc.LDS_LIMIT and c.N * p["B"] <= 12 * p["T"]
        assert p["T"] == 256 or c.N * p["B"] > 6 * p["T"]            # the smallest block that holds 12 values per thread


def test_no_row_is_a_wave_kernel_size():
    from dedalus_amd import libhip
    lib = libhip.load()
    covered = C.c_int(-1)
    for c in tc.CASES:
        if c.kind == "cfft":
            continue
        assert lib.ddh_fft_wave_size(0 if c.kind == "rfft" else 1, c.N, c.M, C.byref(covered)) == 0
        assert covered.value == 0, tc.case_id(c)


def test_pass_schedules():
    f = tc.factorize_mirror
    assert f(1) == [] and f(2) == [2] and f(3) == [3] and f(4) == [4] and f(6) == [6] and f(9) == [3, 3]
    assert f(36) == [6, 6] and f(144) == [16, 3, 3]                  # the 4 3 3 rewrite, and a 16 that must not take it
    assert f(25) == [5, 5] and f(49) == [7, 7] and f(125) == [5, 5, 5] and f(343) == [7, 7, 7]
    assert f(96) == [16, 6] and f(1536) == [16, 16, 6] and f(210) == [5, 7, 6] and f(1000) == [8, 5, 5, 5]
    assert f(11) is None and f(22) is None and f(208) is None
    sched = {tuple(f(c.N)) for c in tc.CASES}
    for r in (2, 3, 4, 5, 6, 7, 8, 16):
        assert any(r in s for s in sched), r
    for r in (3, 5, 6, 7, 16):
        assert any(s.count(r) >= 2 for s in sched), r
    for kind, N, M, alpha, text in tc.PLAN_REFUSALS[:3]:
        assert f(N) is None


def test_every_edge_of_the_table_is_there():
    plans = [(c, shape, tc.plan_mirror(c.kind, c.N, *tc.outer_inner(shape))) for c in tc.CASES for shape in tc.shapes_for(c.N)]
    assert {p["T"] for _, _, p in plans} == {256, 512, 1024}
    assert any(p["lds"] <= 64 * 1024 for _, _, p in plans) and any(p["lds"] > 64 * 1024 for _, _, p in plans)
    assert max(p["lds"] for _, _, p in plans) == 161824              # nothing larger fits: see below
    # B = 1 because the line is long; B clamped to the pair count; a ragged second block with a half-empty last pair
    assert any(p["B"] == 1 and p["npairs"] > 1 for _, _, p in plans)
    assert any(p["B"] == p["npairs"] and p["B"] not in (1, 4, 8, 16) for _, _, p in plans)
    for c in tc.CASES:
        if c.N <= tc.BIG and c.kind != "cfft":
            p = tc.plan_mirror(c.kind, c.N, 2, 19)
            assert p["npairs"] == 10 and p["B"] == 8 and p["grid"] == 4, tc.case_id(c)
            p = tc.plan_mirror(c.kind, c.N, 35, 1)
            assert p["npairs"] == 18 and p["npairs"] % p["B"] != 0 and p["grid"] >= 2, tc.case_id(c)
    # the conversion solve: every path, every scan size edge
    solves = {}
    for c in tc.CASES:
        if c.kind == "cheb" and c.alpha > 0:
            offs = tc.conversion(c.M, c.alpha)[1]
            assert len(offs) <= 4
            solves[(c.N, c.M, c.alpha)] = tc.solve_mirror(c.N, c.M, list(offs))
    assert solves[(210, 140, 1)] == dict(g=2, order=1, E=2, L=70, path="scan")            # ragged: 70 of 128 lane slots
    assert solves[(1536, 1024, 1)]["E"] == 8 and solves[(1536, 1024, 1)]["path"] == "scan"
    assert solves[(1728, 1152, 1)]["E"] == 9 and solves[(1728, 1152, 1)]["path"] == "serial"
    assert any(s["E"] == 1 and s["path"] == "scan" for s in solves.values())
    assert {s["order"] for s in solves.values()} == {0, 1, 2}
    assert solves[(210, 140, 2)]["path"] == "serial" and solves[(210, 140, 3)]["path"] == "general"
    assert list(tc.conversion(140, 3)[1]) == [0, 2, 4, 6] and len(tc.conversion(32, 4)[1]) == 5
    # complex Fourier: even M with the Nyquist slot, odd M, M > N
    cf = [(c.N, c.M) for c in tc.CASES if c.kind == "cfft"]
    assert sum(M % 2 == 0 for _, M in cf) >= 4 and sum(M % 2 == 1 for _, M in cf) >= 2 and any(M > N for N, M in cf)
    # real Fourier on odd grids, and every entry point on every row
    assert sum(c.N % 2 for c in tc.CASES if c.kind == "rfft") >= 8
    assert all(c.ops == tc.RFFT_OPS for c in tc.CASES if c.kind == "rfft")


def test_lds_bound_is_the_whole_request():
    """9216 points is the longest 2,3,5,7-smooth line whose lines AND twiddle table fit 160 KiB; 9408 and 9600 fit with
    their lines alone (159952 B, 163216 B) and not with the table (165184 B, 168544 B): the planner refuses them."""
    assert tc.plan_mirror("rfft", 9216, 3, 1)["lds"] == 161824
    for kind, N, M in tc.LDS_EDGE:
        assert tc.factorize_mirror(N) is not None
        assert (N + (N >> 4) + 1) * 16 <= tc.LDS_LIMIT < (N + (N >> 4) + 1) * 16 + tc.tw_bytes(N)
        assert tc.plan_mirror(kind, N, 3, 1) == "axis too long"
    for N in range(9217, 9408):
        assert tc.factorize_mirror(N) is None or tc.plan_mirror("rfft", N, 3, 1) == "axis too long" or \
            tc.plan_mirror("rfft", N, 3, 1)["lds"] <= tc.LDS_LIMIT
    for kind, N, M, text in tc.CALL_REFUSALS:
        assert tc.factorize_mirror(N) is not None and tc.plan_mirror(kind, N, 3, 1) == text


def test_reference_is_the_matrix_definition_at_a_hand_checked_size():
    """N = 4, M = 4 real Fourier: a0 = mean, a1 = (g0 - g2) / 2, b1 = -(g1 - g3) / 2 (msin); Chebyshev f = 1 -> c0 = sqrt(pi);
    complex M = 4, N = 6 slots [0, 1, (Nyquist: zero), -1]."""
    g = np.array([[1.0], [2.0], [4.0], [8.0]])
    c = tc.rfft_forward_ref(g, 4)
    assert np.allclose(c[:, 0].astype(float), [3.75, 0.0, -1.5, 3.0], atol=1e-18)
    assert np.abs(tc.rfft_backward_ref(c.astype(float), 4)[:, 0].astype(float) - [2.25, 0.75, 5.25, 6.75]).max() < 1e-15
    ones = np.ones((5, 1))
    c = tc.cheb_forward_ref(ones, 3, 0)
    assert abs(float(c[0, 0]) - np.sqrt(np.pi)) < 1e-15 and np.abs(c[1:]).max() < 1e-18
    assert np.abs(tc.cheb_backward_ref(c.astype(float), 5, 0).astype(float) - 1.0).max() < 1e-15
    j = np.arange(6)
    for k, slot in ((1, 1), (-1, 3)):
        c = tc.cfft_forward_ref(np.exp(2j * np.pi * k * j / 6)[:, None], 4)
        want = np.zeros(4)
        want[slot] = 1.0
        assert np.abs(c[:, 0] - want).max() < 1e-15
    c = tc.cfft_forward_ref(np.exp(2j * np.pi * 2 * j / 6)[:, None], 4)          # k = 2 = M / 2: the zeroed slot
    assert np.abs(c).max() < 1e-15
    cin = np.array([1.0, 2.0, 50.0, 3.0])[:, None] + 0j
    g = tc.cfft_backward_ref(cin, 6)[:, 0]
    assert np.abs(g - (1.0 + 2.0 * np.exp(2j * np.pi * j / 6) + 3.0 * np.exp(-2j * np.pi * j / 6))).max() < 1e-14
