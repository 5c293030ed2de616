"""CPU: the one backend contract of the implicit solves (dedalus_amd/core/packbase.py) -- the oracle pack's request
against the reference's steps called directly, its refusals, the declarations of the three packs, the wrapper of a pack
older than the contract, the modal solve's bookkeeping without a device, and the paths SolverBase.solve_lincomb takes --
at the smallest problems that reach each branch: a 1-D Chebyshev LBVP without P, a 2-D (8 x 16) IVP with P and tau
rows, the 12 x 20 x 8 periodic box on the band fallback."""
import numpy as np
import pytest

import periodic3d_cases as pc
import problems
from oracle import np_pencil as npp
from oracle.np_executor import NumpyExecutor, _NpPack

import dedalus_amd.public as d3
from dedalus_amd.core.packbase import PackBase, PreContractPack

KW = dict(dist_kw=dict(executor=NumpyExecutor()))
MATERIALISED = "ddh_pencil_solve_recombined (one materialised right-hand side)"


def _lbvp_1d():
    """2 u = f on one Chebyshev axis: no boundary rows, so no recombination P"""
    zc = d3.Coordinate("z")
    dist = d3.Distributor(zc, dtype=np.float64, executor=NumpyExecutor())
    zb = d3.ChebyshevT(zc, size=12, bounds=(0, 1))
    u, f = dist.Field(name="u", bases=zb), dist.Field(name="f", bases=zb)
    z, = dist.local_grids(zb)
    f["g"] = np.exp(z) * np.sin(3 * z)
    problem = d3.LBVP([u], namespace=dict(u=u, f=f))
    problem.add_equation("2*u = f")
    return problem.build_solver()


_SOLVERS = {}


def solver_of(name):
    """(solver, lu id, a, b), built once and left unchanged"""
    if name not in _SOLVERS:
        if name == "lbvp1d":
            s, a, b = _lbvp_1d(), 0.0, 1.0
        elif name == "rb2d":
            s, a, b = problems.rayleigh_benard_2d(d3, Nx=8, Nz=16, **KW)[0], 1.0, 3e-4
        else:
            s, a, b = pc.taylor_green(d3, (12, 20, 8), "RK222", **KW)[0], 1.0, 0.5 * pc.DT
        _SOLVERS[name] = (s, s.factor(a, b), a, b)
    return _SOLVERS[name]


def test_the_three_problems_reach_the_three_branches():
    assert solver_of("lbvp1d")[0].P_id is None and solver_of("lbvp1d")[0].nf == 0
    s = solver_of("rb2d")[0]
    assert s.P_id is not None and (s.nx, s.R) == (8, 16 * 4 + 7) and len(s._boundary_rows()) == 6
    assert type(s.pack) is _NpPack and s.pack.posts == [] and s.pack.pairing is None
    s = solver_of("box")[0]
    assert s.modal is None and s.P_id is None and s.dist._pencil_fourier and (s.nx, s.ny) == (12, 20)


def reference_steps(s, a, b, xs, alphas, with_p):
    """The reference's steps, called directly on the oracle's building blocks: axpy chain into a zeroed buffer in term
    order, PencilLU.solve per pencil, mat-vec with P."""
    pk = s.pack
    lu = npp.PencilLU(pk.mats[s.MP_id], pk.mats[s.LP_id], a, b, pk.nf, pk.nx, pk.ny, pk.kx, pk.ky,
                      np.asarray(s.row_axes), np.asarray(s.col_axes), pk.mx_offset)
    rhs = np.zeros((s.R, s.nx, s.ny))
    for v, al in zip(xs, alphas):
        rhs += al * v
    y = lu.solve(rhs).reshape(rhs.shape)
    if not with_p:
        return y
    P = pk.mats[s.P_id]
    return npp.matvec(P, y.reshape(P.ncols, pk.nx, pk.ny), pk.nf, pk.kx, pk.ky, pk.mx_offset).reshape(rhs.shape)


@pytest.mark.parametrize("name,with_p", [("lbvp1d", False), ("rb2d", False), ("rb2d", True), ("box", False)])
@pytest.mark.parametrize("nterms", [1, 8])
def test_request_agrees_bit_for_bit_with_the_steps_called_directly(name, with_p, nterms):
    s, lu, a, b = solver_of(name)
    rng = np.random.default_rng(7 * nterms + len(name))
    shape = (s.R, s.nx, s.ny)
    xs = [rng.normal(size=shape) for _ in range(nterms)]
    alphas = [1.0] if nterms == 1 else list(rng.normal(size=nterms))
    want = reference_steps(s, a, b, xs, alphas, with_p)
    x = np.full(shape, np.nan)
    if with_p:
        s.pack.solve(lu, xs, alphas, x, p_mat_id=s.P_id, work=np.full(shape, np.nan))
    else:
        s.pack.solve(lu, xs, alphas, x)
    assert np.isfinite(want).all() and np.abs(want).max() > 0
    assert x.tobytes() == want.tobytes()


@pytest.mark.parametrize("with_p", [False, True])
def test_request_with_x_aliasing_a_term(with_p):
    s, lu, a, b = solver_of("rb2d")
    rng = np.random.default_rng(5)
    shape = (s.R, s.nx, s.ny)
    xs = [rng.normal(size=shape) for _ in range(3)]
    alphas = [0.5, -2.0, 0.3]
    want = reference_steps(s, a, b, [v.copy() for v in xs], alphas, with_p)
    if with_p:
        s.pack.solve(lu, xs, alphas, xs[1], p_mat_id=s.P_id, work=np.zeros(shape))
    else:
        s.pack.solve(lu, xs, alphas, xs[1])
    assert xs[1].tobytes() == want.tobytes()


REFUSALS = [
    (dict(tiled=True), "the oracle pack takes no tile-major terms"),
    (dict(mx=(0, None)), "the oracle pack does not write M.x"),
    (dict(zero_rows=(None, 0.0)), "the oracle pack takes no zero_rows mask"),
    (dict(skip_rows=(None, 0.0)), "the oracle pack takes no skip_rows mask"),
    (dict(p_mat_id=0), "the oracle pack applies P through a work vector"),
]


@pytest.mark.parametrize("kw,message", REFUSALS)
def test_refusals_have_their_own_message_and_write_nothing(kw, message):
    s, lu, a, b = solver_of("rb2d")
    shape = (s.R, s.nx, s.ny)
    x = np.full(shape, 7.0)
    with pytest.raises(ValueError, match=message):
        s.pack.solve(lu, [np.ones(shape)], [1.0], x, **kw)
    assert (x == 7.0).all()
    assert len({m for _, m in REFUSALS}) == 5


CONTRACT = ["MAX_RHS_TERMS", "supports_tiled_rhs", "supports_zero_rows", "supports_mx_emission", "supports_pairing",
            "supports_row_blocks", "supports_state_tiling", "supports_block_inverse", "variant_epoch",
            "flagged", "lu_bytes"]


def test_every_pack_declares_the_contract_on_its_class():
    from dedalus_amd.core.curviproblem import MatvecPack
    from dedalus_amd.pencilpack import PencilPack
    capabilities = [n for n in CONTRACT if n.startswith("supports_")]
    for cls in (PencilPack, _NpPack, MatvecPack):
        assert issubclass(cls, PackBase)
        for name in CONTRACT:
            assert hasattr(cls, name), (cls.__name__, name)
        assert cls.MAX_RHS_TERMS == 8 and cls.variant_epoch == 0 and len(cls.flagged) == 0 and callable(cls.lu_bytes)
    assert all(getattr(PackBase, n) is False for n in capabilities)
    assert all(getattr(PencilPack, n) is True for n in capabilities)
    assert [n for n in capabilities if getattr(_NpPack, n)] == ["supports_pairing"]
    assert not any(getattr(MatvecPack, n) for n in capabilities)
    # every capability names methods the declaring pack has
    for flag, method in (("supports_pairing", "set_pairing"), ("supports_row_blocks", "set_row_blocks"),
                         ("supports_state_tiling", "set_state_tiled"), ("supports_block_inverse", "set_block_inverse"),
                         ("supports_mx_emission", "set_mx_band")):
        for cls in (PencilPack, _NpPack, MatvecPack):
            assert not getattr(cls, flag) or callable(getattr(cls, method)), (cls.__name__, flag)
    with pytest.raises(TypeError):
        PackBase.flagged[0] = []                        # (the shared default cannot be written through)


def test_a_pack_older_than_the_contract_is_wrapped_once():
    """SolverBase gives a pack that does not inherit PackBase the contract at construction: the request becomes the pack's
    own solve_lincomb and mat-vec, attribute reads and writes reach the pack, anything beyond terms and P is refused."""
    calls = []

    class Old:
        MAX_RHS_TERMS = 8
        mats = "the pack's own"

        def solve_lincomb(self, lu, xs, alphas, x):
            calls.append(("solve_lincomb", lu, xs, alphas, x))

        def matvec(self, mid, x, y):
            calls.append(("matvec", mid, x, y))

        def lu_bytes(self, lu):
            return 5

    old = Old()
    pk = PreContractPack(old)
    pk.solve(3, ["a"], [1.0], "x")
    pk.solve(3, ["a"], [1.0], "x", p_mat_id=2, work="w", zero_rows=None, skip_rows=None, tiled=False, mx=None)
    assert calls == [("solve_lincomb", 3, ["a"], [1.0], "x"), ("solve_lincomb", 3, ["a"], [1.0], "w"), ("matvec", 2, "w", "x")]
    for kw in (dict(tiled=True), dict(mx=(0, None)), dict(zero_rows=(None, 0.0)), dict(skip_rows=(None, 0.0))):
        with pytest.raises(ValueError, match="terms and P only"):
            pk.solve(3, ["a"], [1.0], "x", p_mat_id=2, work="w", **kw)
    assert len(calls) == 3
    pk.matrices = [1]
    assert old.matrices == [1] and pk.mats == "the pack's own" and pk.lu_bytes(0) == 5 and pk.inner is old
    assert pk.supports_pairing and not pk.supports_zero_rows and not pk.supports_row_blocks and pk.variant_epoch == 0


def test_modal_solve_keeps_its_pairs_without_a_device_call():
    from dedalus_amd.executor import ModalSolve

    class Ex:
        timer = None

    m = object.__new__(ModalSolve)                      # (no ddh_modal_create: the bookkeeping alone)
    m.ex, m._ab, calls = Ex(), [], []
    m._solve = lambda *args: calls.append(args)
    assert (m.factor(1.0, 0.25), m.factor(1, 0.5)) == (0, 1)
    assert m.factor(2.0, 0.125, reuse=0) == 0 and m.factor(3.0, 4.0) == 2
    xs, al, x = [object()], [1.0], object()
    for lu in (0, 1, 2):
        m.solve_factored(lu, xs, al, x)
    assert calls == [(2.0, 0.125, xs, al, x, False, False), (1.0, 0.5, xs, al, x, False, False),
                     (3.0, 4.0, xs, al, x, False, False)]
    assert all(type(v) is float for c in calls for v in c[:2])
    assert [m.lu_bytes(lu) for lu in (0, 1, 2)] == [0, 0, 0]
    with pytest.raises(IndexError):
        m.solve_factored(3, xs, al, x)
    m.ex = None                                         # (__del__ must not reach for a handle that was never made)


def test_solver_on_a_stand_in_modal_solve_factors_nothing():
    """SolverBase picks `modal` over the pack in factor / solve / solve_lincomb / factor_bytes: a stand-in that records."""
    s = pc.taylor_green(d3, (12, 20, 8), "RK222", **KW)[0]
    calls = []

    class Modal:
        MAX_RHS_TERMS = 8
        pairs = []

        def factor(self, a, b, reuse=-1):
            if reuse < 0:
                self.pairs.append(None)
                reuse = len(self.pairs) - 1
            self.pairs[reuse] = (a, b)
            return reuse

        def lu_bytes(self, lu):
            return 0

        def solve_factored(self, lu, xs, alphas, x):
            calls.append((lu, len(xs), list(alphas)))

    s.modal = Modal()
    lu0, lu1 = s.factor(1.0, 0.5), s.factor(1.0, 0.25)
    assert (lu0, lu1) == (0, 1) and s.factor(1.0, 0.125, reuse=0) == 0
    assert s._lu_params == {0: (1.0, 0.125), 1: (1.0, 0.25)} and s.factor_calls == 0 and s.factor_bytes() == 0
    v = np.ones((s.R, s.nx, s.ny))
    s.solve_lincomb(1, [v] * 8, [0.125] * 8, np.zeros_like(v))
    s.solve_lincomb(0, [v] * 9, [1.0] * 9, np.zeros_like(v))
    assert calls == [(1, 8, [0.125] * 8), (0, 1, [1.0])]
    assert s._last_rhs is not None and (s._last_rhs == 9.0).all()
    with pytest.raises(RuntimeError, match="tile-major right-hand sides need the fused recombined solve"):
        s.solve_lincomb(0, [v], [1.0], np.zeros_like(v), tiled=True)
    s.solve_probe = dict(groups=pc.MATRIX_GROUPS, records=[])
    s.solve_lincomb(1, [v] * 2, [1.0, 2.0], np.zeros_like(v))
    assert calls[-1] == (1, 1, [1.0]) and (s._last_rhs == 3.0).all()
    rec, = s.solve_probe["records"]
    assert rec["path"] == MATERIALISED and rec["terms"] == 1 and (rec["a"], rec["b"]) == (1.0, 0.25)


@pytest.mark.parametrize("name", ["rb2d", "box"])
def test_solve_lincomb_takes_the_materialised_path(name):
    """MAX_RHS_TERMS + 1 terms: one materialised right-hand side whatever the probe; MAX_RHS_TERMS terms: the request,
    and with a probe its record carries the fused label.  Either way the solution is the reference's steps on the
    axpy chain of the terms, bit for bit."""
    s, lu, a, b = solver_of(name)
    n = s.pack.MAX_RHS_TERMS
    rng = np.random.default_rng(3)
    shape = (s.R, s.nx, s.ny)
    xs = [rng.normal(size=shape) for _ in range(n + 1)]
    groups = pc.MATRIX_GROUPS if s.nf == 2 else [(0, 0), (1, 0), (3, 0)]
    outs = []
    try:
        for terms, al in ((xs, list(rng.normal(size=n + 1))), (xs[:n], list(rng.normal(size=n)))):
            s.solve_probe = dict(groups=groups, records=[])
            s._last_rhs = None
            out = np.zeros(shape)
            s.solve_lincomb(lu, terms, al, out)
            rec, = s.solve_probe["records"]
            rhs = np.zeros(shape)
            for v, w in zip(terms, al):
                rhs += w * v
            assert s._last_rhs.tobytes() == rhs.tobytes()
            # (one materialised vector goes through the same steps as its terms would: the axpy chain of one term is exact)
            assert out.tobytes() == reference_steps(s, a, b, [rhs], [1.0], s.P_id is not None).tobytes()
            assert (rec["a"], rec["b"]) == (a, b) and len(rec["rhs"]) == len(rec["x"]) == len(groups)
            assert "skipped" not in rec and not rec["zero_rows"] and not rec["skip_rows"]
            for k, (gx, gy) in enumerate(groups):
                assert rec["rhs"][k].tobytes() == s.gather_pencil(rhs, "equations", gx, gy).tobytes()
                assert rec["x"][k].tobytes() == s.gather_pencil(out, "variables", gx, gy).tobytes()
            outs.append((out, rec, al))
    finally:
        s.solve_probe = None
    (x9, r9, al9), (x8, r8, al8) = outs
    assert r9["path"] == MATERIALISED and r9["terms"] == 1
    assert r8["path"] == "ddh_pencil_solve_lincomb (%d fused terms)" % n and r8["terms"] == n
    # without a probe the same calls leave the same solutions
    for terms, al, want in ((xs, al9, x9), (xs[:n], al8, x8)):
        out = np.zeros(shape)
        s.solve_lincomb(lu, terms, al, out)
        assert out.tobytes() == want.tobytes()
    with pytest.raises(RuntimeError, match="tile-major right-hand sides need the fused recombined solve"):
        s.solve_lincomb(lu, xs[:2], [1.0, 1.0], out, tiled=True)
    with pytest.raises(RuntimeError, match="M.X from the sweep needs the tiled fused recombined solve"):
        s.solve_lincomb(lu, xs[:2], [1.0, 1.0], out, mx_out=np.zeros(shape))
