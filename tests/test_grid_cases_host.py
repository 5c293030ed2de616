"""CPU: the references and case tables of tests/grid_cases.py that tests/test_gpu_grid_kernels.py runs the streaming grid
kernels against.  Each reference agrees with the NumpyExecutor method of the same operation, every launch-shape class is
populated, and the class of every case, recomputed from its shape and the restated launch constants, equals the declared
one.  Also the host side of the CFL NaN policy: a NaN frequency survives the host reductions and leaves the timestep
unchanged, as in the reference (extras/flow_tools.py:191-214)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import cfl_nan_checks
import grid_cases as gc
from oracle.np_executor import NumpyExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NP = NumpyExecutor()


def nrel(a, b):
    a, b = np.asarray(a, dtype=gc.LD), np.asarray(b, dtype=gc.LD)
    return float(np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-300))


# ---- references against the oracle executor ---------------------------------------------------------------------------
@pytest.mark.parametrize("nterms,n", [c for c in gc.LINCOMB_CASES if c[0] * c[1] <= gc.HOST_LIMIT])
def test_lincomb_reference_matches_oracle(nterms, n):
    xs, al = gc.lincomb_inputs(nterms, n)
    ref, mag = gc.lincomb(xs, al)
    y = np.full(n, np.nan)
    NP.lincomb(y, xs, al)
    assert nrel(y, ref) <= 1e-15
    assert np.all(np.abs(y - ref) <= (nterms + 1) * gc.U * mag)           # the bound of the GPU test holds for NumPy too
    assert np.all(mag >= np.abs(ref))


@pytest.mark.parametrize("name,n", [c for c in gc.BILINEAR_CASES if c[1] <= 100003])
def test_bilinear_reference_matches_oracle(name, n):
    ncomp_out, na, nb, terms = gc.BILINEAR_TABLES[name]
    a, b = gc.bilinear_inputs(name, n)
    ref, mag, count = gc.bilinear(ncomp_out, a, b, n, terms)
    out = np.full((ncomp_out, n), np.nan)
    NP.bilinear(out, ncomp_out, a, b, n, terms)
    for c in range(ncomp_out):
        if count[c] == 0:
            assert np.all(out[c] == 0.0) and np.all(ref[c] == 0.0)
        else:
            assert nrel(out[c], ref[c]) <= 1e-15, c
            assert np.all(np.abs(out[c] - ref[c]) <= (count[c] + 2) * gc.U * mag[c])


@pytest.mark.parametrize("name", list(gc.CFL_CASES))
@pytest.mark.parametrize("plant", gc.PLANTS)
def test_cfl_reference_matches_oracle_and_the_plant_is_the_maximum(name, plant):
    shape, comp_axis, _, _ = gc.CFL_CASES[name]
    u, inv, at = gc.cfl_inputs(name, plant)
    if plant != "none" and at is None:
        return                                                            # the shape has no such point
    ref = gc.cfl_max(u, len(comp_axis), shape, inv, comp_axis)
    got = NP.cfl_max(u, len(comp_axis), shape, inv, comp_axis)
    assert abs(got - ref) <= 1e-15 * ref and ref > 0
    f = gc.cfl_field(u, len(comp_axis), shape, inv, comp_axis).ravel()
    if at is not None:
        assert int(np.argmax(f)) == at
        assert f[at] > 100 * np.max(np.delete(f, at))                     # well above the rest
        if plant == "final_pass":
            assert at >= (f.size - 1) // gc.STREAM_PASS * gc.STREAM_PASS > 0
        if plant == "distinct_indices":
            idx = [i for i, s in zip(np.unravel_index(at, shape), shape) if s > 1]
            assert len(set(idx)) == len(idx) >= 2


def test_cfl_distinct_index_plant_sees_every_wrong_decomposition():
    """non-uniform spacings on every axis: reading any other axis order, or the reversed digit order, for the planted
    point changes the frequency there by far more than the test's bound"""
    import itertools
    for name in ("box7x12x5", "box7x12x5_rotated", "box192x96x48", "box192x96x48_rotated"):
        shape, comp_axis, kinds, _ = gc.CFL_CASES[name]
        assert "uniform" not in kinds
        u, inv, at = gc.cfl_inputs(name, "distinct_indices")
        idx = np.unravel_index(at, shape)
        right = sum(abs(u[c, at]) * inv[c][idx[comp_axis[c]]] for c in range(3))
        for perm in itertools.permutations(range(3)):
            if perm == (0, 1, 2):
                continue
            wrong_idx = [idx[p] for p in perm]
            if any(wrong_idx[comp_axis[c]] >= len(inv[c]) for c in range(3)):
                continue
            wrong = sum(abs(u[c, at]) * inv[c][wrong_idx[comp_axis[c]]] for c in range(3))
            assert abs(wrong - right) > 1e-3 * right, (name, perm)


@pytest.mark.parametrize("name", list(gc.SPH_CASES))
@pytest.mark.parametrize("plant", gc.SPH_PLANTS)
def test_spherical_cfl_reference_matches_oracle(name, plant):
    shape = gc.SPH_CASES[name][0]
    u, inv_h, inv_dr, at = gc.sph_inputs(name, plant)
    if plant != "none" and at is None:
        return
    ref = gc.cfl_max_spherical(u, inv_h, inv_dr)
    got = NP.cfl_max_spherical(u, inv_h, inv_dr)
    assert abs(got - ref) <= 1e-15 * ref and ref > 0
    if at is not None:
        f = gc.cfl_field_spherical(u, inv_h, inv_dr).ravel()
        assert int(np.argmax(f)) == at and f[at] > 100 * np.max(np.delete(f, at))


def test_cfl_references_and_oracle_return_nan_for_nan_input():
    shape, comp_axis, _, _ = gc.CFL_CASES["box7x12x5_rotated"]
    for where in gc.NAN_PLANTS:
        for comp in range(3):
            u, inv, _ = gc.cfl_inputs("box7x12x5_rotated")
            u[comp, gc.nan_index(shape, where)] = np.nan
            assert math.isnan(gc.cfl_max(u, 3, shape, inv, comp_axis)) and math.isnan(NP.cfl_max(u, 3, shape, inv, comp_axis))
            us, inv_h, inv_dr, _ = gc.sph_inputs("shell8x4x5")
            us.reshape(3, -1)[comp, gc.nan_index(us.shape[1:], where)] = np.nan
            assert math.isnan(gc.cfl_max_spherical(us, inv_h, inv_dr)) and math.isnan(NP.cfl_max_spherical(us, inv_h, inv_dr))
    u, inv, _ = gc.cfl_inputs("box7x12x5")
    assert math.isnan(NP.cfl_max(np.full_like(u, np.nan), 3, shape, inv, (0, 1, 2)))
    assert gc.cfl_max(np.zeros_like(u), 3, shape, inv, (0, 1, 2)) == 0.0


@pytest.mark.parametrize("n", gc.SCATTER_SIZES)
def test_scatter_references_match_oracle_bit_for_bit(n):
    y, idx, vals = gc.scatter_inputs(n)
    assert len(np.unique(idx)) == n and idx.max() < y.size
    for ref_fn, method in ((gc.scatter_add, NP.scatter_add), (gc.scatter_set, NP.scatter_set)):
        got = y.copy()
        method(got, NP.make_scatter(idx, vals))
        ref = ref_fn(y, idx, vals)
        assert np.array_equal(got, ref)
        untouched = np.ones(y.size, bool)
        untouched[idx] = False
        assert np.array_equal(ref[untouched], y[untouched]) and not np.array_equal(ref[idx], y[idx])


def _small(name):
    kind, dims, _ = gc.PACK_CASES[name]
    return gc.pack_geometry(kind, dims)[3] <= gc.HOST_LIMIT


@pytest.mark.parametrize("name", [k for k in gc.PACK_CASES if _small(k)])
def test_pack_references_match_oracle_bit_for_bit(name):
    kind, dims, _ = gc.PACK_CASES[name]
    src = gc.pack_input(kind, dims)
    ref = gc.pack_reference(kind, src, dims)
    assert ref.size == gc.pack_geometry(kind, dims)[4]
    assert np.array_equal(np.sort(ref), src)                              # a permutation of the distinct inputs
    if kind in ("a2a_pack", "a2a_unpack"):
        dst = np.full(ref.size, np.nan)
        getattr(NP, kind)(src, dst, *dims)
        assert np.array_equal(dst, ref)
        return
    # uneven blocks: the slicing definition, element by element from the offsets of the header's description
    outer, n, row, P, block = dims
    lo = gc.block_bounds(n, P, block)
    packed = np.full(src.size, np.nan)
    natural = src if kind == "a2av_pack" else np.full(src.size, np.nan)
    off = 0
    for p in range(P):
        w = lo[p + 1] - lo[p]
        for o in range(outer):
            for k in range(w):
                a, b = slice(off, off + row), slice((o * n + lo[p] + k) * row, (o * n + lo[p] + k + 1) * row)
                if kind == "a2av_pack":
                    packed[a] = natural[b]
                else:
                    natural[b] = src[a]
                off += row
    assert np.array_equal(packed if kind == "a2av_pack" else natural, ref)


def test_uneven_references_reduce_to_the_even_ones_and_invert_each_other():
    rng = np.random.default_rng(4)
    for outer, na, nb, inner, P in [(3, 8, 5, 7, 4), (2, 6, 1, 9, 3), (1, 4, 3, 2, 1)]:
        src = rng.standard_normal(outer * na * nb * inner)
        assert np.array_equal(gc.a2av_pack(src, outer, na, nb * inner, P), gc.a2a_pack(src, outer, na, nb, inner, P))
    for outer, na, nb, inner, P in [(3, 5, 8, 7, 4), (2, 1, 6, 9, 3)]:
        src = rng.standard_normal(outer * na * nb * inner)
        assert np.array_equal(gc.a2av_unpack(src, outer * na, nb, inner, P), gc.a2a_unpack(src, outer, na, nb, inner, P))
    for outer, n, row, P, block in [(4, 7, 5, 3, 4), (3, 5, 3, 4, 0), (2, 9, 4, 4, 0)]:
        src = rng.standard_normal(outer * n * row)
        assert np.array_equal(gc.a2av_unpack(gc.a2av_pack(src, outer, n, row, P, block), outer, n, row, P, block), src)


# ---- classes ----------------------------------------------------------------------------------------------------------
def test_launch_constants_match_the_kernel_source():
    """the restated constants are the literals of dedalus_amd/csrc/ddh_grid.hip

    The match is on exact source lines, so a reformat of one of them fails here without any change of behaviour: update
    the string below (and, if a value moved, the constant of grid_cases.py and the cases that depend on it)."""
    src = open(os.path.join(ROOT, "dedalus_amd", "csrc", "ddh_grid.hip")).read()
    for text in ("constexpr int MAX_TERMS = %d;" % gc.LINCOMB_MAX_TERMS, "constexpr int MAX_BIL = %d;" % gc.BILINEAR_MAX_TERMS,
                 "if (blocks > 256 * 8) blocks = 256 * 8;", "if (ncomp_out > %d)" % gc.BILINEAR_MAX_OUT,
                 "long cx = (seg_doubles / 2 + 1023) / 1024;", "while (cx > 1 && cx * nseg > %d)" % gc.SEG_WORKGROUP_TARGET,
                 "if (cx > %d) cx = %d;" % (gc.SEG_CX_CAP, gc.SEG_CX_CAP), "nseg < %d ? nseg : %d" % (gc.SEG_GRID_Y_CAP, gc.SEG_GRID_Y_CAP),
                 "for (; i + 3 * nth < n2; i += 4 * nth)"):
        assert text in src, text
    assert gc.STREAM_MAX_BLOCKS == 256 * 8 and gc.SEG_WORDS_PER_CHUNK == 1024 and gc.SEG_UNROLL == 4
    assert gc.STREAM_PASS == 524288


def test_streaming_cases_are_classified_and_cover_every_class():
    assert set(gc.LINCOMB_NTERMS) == {1, 2, 5, gc.LINCOMB_MAX_TERMS}
    for n in gc.LINCOMB_SIZES:
        assert gc.stream_tags(n) == tuple(sorted(gc.LINCOMB_TAGS[n])), n
    assert {gc.stream_tags(n) for n in gc.LINCOMB_SIZES} == {tuple(sorted(c)) for c in gc.LINCOMB_CLASSES}
    assert gc.stream_tags(gc.LINCOMB_ALIAS_CASE[1]) == ("odd", "one_pass")
    for _, n in gc.BILINEAR_CASES:
        assert gc.stream_tags(n) == tuple(sorted(gc.BILINEAR_TAGS[n])), n
    assert {gc.stream_tags(n) for _, n in gc.BILINEAR_CASES} == {tuple(sorted(c)) for c in gc.BILINEAR_CLASSES}
    for n in gc.SCATTER_SIZES:
        assert gc.scatter_tags(n) == gc.SCATTER_TAGS[n]
    assert {gc.scatter_tags(n) for n in gc.SCATTER_SIZES} == {("one_block",), ("two_blocks",), ("many_blocks",)}


def test_bilinear_tables_cover_the_instantiations_and_the_term_shapes():
    tabs = gc.BILINEAR_TABLES
    assert {t[0] for t in tabs.values()} == {1, 2, 3, 4, 9}               # <= 1 -> <1>, 2..3 -> <3>, 4..9 -> <9>
    assert max(len(t[3]) for t in tabs.values()) == gc.BILINEAR_MAX_TERMS
    for name, (nout, na, nb, terms) in tabs.items():
        assert all(0 <= ic < nout and 0 <= ia < na and 0 <= ib < nb for ic, ia, ib, _ in terms), name
        key = [(t[1], t[2]) for t in terms]
        if len(set(key)) > 1:
            assert key != sorted(key), name                               # reaches the host-side sort unsorted
    nout, _, _, terms = tabs["shared_pairs_gap"]
    by_pair = {}
    for ic, ia, ib, _ in terms:
        by_pair.setdefault((ia, ib), set()).add(ic)
    assert max(len(v) for v in by_pair.values()) >= 3                     # one pair feeds three outputs
    assert set(range(nout)) - {t[0] for t in terms} == {2}                # output 2 receives no term
    assert len({(t[1], t[2]) for t in tabs["terms32"][3]}) < 32           # repeated pairs among the 32 terms
    name, n = gc.BILINEAR_ODD_CASE
    assert n & 1 and tabs[name][:3] == (1, 1, 1)


def test_cfl_cases_are_classified_and_cover_every_class():
    seen = set()
    for name, (shape, comp_axis, kinds, tags) in gc.CFL_CASES.items():
        assert gc.cfl_tags(shape, comp_axis) == tuple(sorted(tags)), name
        assert sorted(comp_axis) == list(range(len(shape))) and len(kinds) == len(comp_axis)
        seen |= set(tags)
    assert seen >= set(gc.CFL_CLASSES)
    assert {c[0] for c in gc.CFL_CASES.values()} >= {(7, 12, 5), (96, 1, 48), (64, 96), (192, 96, 48)}
    assert any("cheb" in c[2] for c in gc.CFL_CASES.values())
    assert all(gc.plant_index((192, 96, 48), w) is not None for w in gc.PLANTS[1:])
    seen = set()
    for name, (shape, zero_h, tags) in gc.SPH_CASES.items():
        assert gc.sph_tags(shape, zero_h) == tuple(sorted(tags)), name
        seen |= set(tags)
    assert seen >= set(gc.SPH_CLASSES)
    assert {c[0] for c in gc.SPH_CASES.values()} == {(8, 4, 5), (64, 32, 48), (128, 96, 72)}
    u, _, _ = gc.cfl_inputs("box7x12x5")
    assert np.any(np.signbit(u) & (u == 0)) and np.any(~np.signbit(u) & (u == 0)) and np.any(u > 0) and np.any(u < 0)


def test_pack_cases_are_classified_and_cover_every_class():
    for name, (kind, dims, tags) in gc.PACK_CASES.items():
        assert gc.pack_tags(kind, dims) == tags, (name, gc.pack_tags(kind, dims))
        _, _, _, n_in, n_out = gc.pack_geometry(kind, dims)
        if name not in gc.CX_HALVED_EXCEPTION:
            assert 8 * (max(n_in, n_out) + gc.GUARD) <= gc.MAX_BUFFER_BYTES, name
    for cls, pred in gc.PACK_CLASSES.items():
        for kind in gc.PACK_CLASS_KINDS[cls]:
            hits = [n for n, (k, d, t) in gc.PACK_CASES.items() if k == kind and pred(t)]
            assert hits, (cls, kind)
    # the shapes the classes are named after
    geo = lambda n: gc.pack_geometry(*gc.PACK_CASES[n][:2])
    for pre in ("pack", "unpack"):
        assert geo(pre + "_seg2000")[1] == 2000 and geo(pre + "_seg1800")[1] == 1800 and geo(pre + "_scalar4097")[1] == 4097
        assert geo(pre + "_halved")[:2] == (64, 1 << 20) and geo(pre + "_capped")[:2] == (8, 3276800)
        assert geo(pre + "_ycap")[:2] == (131072, 6) and gc.PACK_CASES[pre + "_ycap"][1][4] == 8
    assert gc.seg_grid(64, 1 << 20)[:3] == (256, 64, True) and gc.seg_grid(8, 3276800) == (1024, 8, False, True)
    assert gc.seg_grid(131072, 6)[:2] == (1, 65535) and gc.seg_grid(12, 2000)[0] == 1
    # halving needs more than 2^25 doubles in an even pack: why the two exceptions exist
    assert all(gc.seg_grid(nseg, (1 << 25) // nseg)[2] is False for nseg in (8, 16, 64, 512, 4096))
    for name in ("packv_mixed", "unpackv_mixed"):
        kind, dims, _ = gc.PACK_CASES[name]
        assert dims[2] & 1 and dims[3] == 3
        segs = gc.pack_geometry(kind, dims)[2]
        assert {v for c, v in segs if c} == {True, False} and min(c for c, v in segs if c) > 2048 and (0, True) in segs


# ---- the NaN policy on the host ---------------------------------------------------------------------------------------
def test_nan_frequency_survives_the_host_maximum():
    from dedalus_amd.extras.flow_tools import _nan_max
    nan = float("nan")
    assert math.isnan(_nan_max(0.0, nan)) and math.isnan(_nan_max(nan, 3.0)) and math.isnan(_nan_max(nan, nan))
    assert _nan_max(0.0, 2.0) == 2.0 and _nan_max(2.0, 0.5) == 2.0 and _nan_max(0.0, 0.0) == 0.0
    assert _nan_max(1.0, float("inf")) == float("inf")


def test_nan_velocity_leaves_the_timestep_unchanged_on_the_oracle_executor():
    import dedalus_amd.public as d3
    cfl_nan_checks.nan_velocity_leaves_dt_unchanged(d3, dist_kw=dict(executor=NumpyExecutor()))


def test_nan_shell_velocity_leaves_the_timestep_unchanged_on_the_oracle_executor():
    import dedalus_amd.public as d3
    cfl_nan_checks.nan_shell_velocity_leaves_dt_unchanged(d3, dist_kw=dict(executor=NumpyExecutor()))


def test_curvilinear_cfl_sample_keeps_a_nan_frequency():
    """the `cfl_frequency_max` branch of CFL._sample (shell velocities) folded with max(): max(0.0, nan) is 0.0"""
    from dedalus_amd.extras.flow_tools import CFL

    class _Solver:
        iteration, initial_iteration, dist, ex = 4, 0, None, None
        _step_hooks = []

    class _U:
        tensorsig = (None,)

        def __init__(self, v):
            self.v = v

        def cfl_frequency_max(self):
            return self.v

    for v in (float("nan"), 2.5):
        cfl = CFL(_Solver(), initial_dt=0.01, cadence=1, safety=0.5)
        cfl.add_velocity(_U(v))
        cfl._sample(cfl.solver)
        if v != v:
            assert math.isnan(cfl._max_freq)
            cfl.solver.iteration = 5
            assert cfl.compute_timestep() == 0.01
        else:
            assert cfl._max_freq == 2.5
            cfl.solver.iteration = 5
            assert cfl.compute_timestep() == 0.5 / 2.5


_ALLREDUCE_WORKER = r'''
import math, os, sys
sys.path.insert(0, %r)
from dedalus_amd.parallel import Comm
c = Comm(2)
nan = float("nan")
for holder in (0, 1):                       # the NaN on either rank, the larger finite value on the other
    got = c.allreduce_max(nan if c.rank == holder else 7.0 + c.rank)
    assert math.isnan(got), (holder, got)
assert c.allreduce_max(1.0 + c.rank) == 2.0 and c.allreduce_max(-3.0 - c.rank) == -3.0
assert c.allreduce_max(float("inf") if c.rank == 0 else 0.0) == float("inf")
assert math.isnan(c.allreduce_max(nan))
print("OK", c.rank)
'''


def test_allreduce_max_over_two_ranks_keeps_a_nan(tmp_path):
    script = tmp_path / "allreduce_worker.py"
    script.write_text(_ALLREDUCE_WORKER % ROOT)
    port = 31500 + (os.getpid() % 2000)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), str(script)]
    env = dict(os.environ, OMP_NUM_THREADS="1", DDH_DIST_BACKEND="gloo")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and r.stdout.count("OK") == 2, r.stderr[-3000:]
