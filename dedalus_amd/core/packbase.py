"""
What SolverBase (core/solvers.py) and the timesteppers (core/timesteppers.py) ask of a pack, declared in one place.

A pack holds the matrices of all pencils and answers `matvec(mat_id, x, y)`; one that also factors answers
`factor(...) -> lu id` and the request

    solve(lu_id, xs, alphas, x, p_mat_id=None, work=None, zero_rows=None, skip_rows=None, tiled=False, mx=None)

x = (a M + b L)^-1 sum_t alphas[t] xs[t], with p_mat_id: x = P (...) through `work`.  Everything beyond the terms and P
is a capability a pack declares below and the solver asks for before it sends it: a pack that is sent what it did not
declare raises.  No import of the device library here: the mat-vec pack of the sphere and the shell
(core/curviproblem.py) and the test oracle's pack (oracle/np_executor.py) inherit this class like PencilPack
(pencilpack.py) does.
"""

from types import MappingProxyType


class PackBase:
    MAX_RHS_TERMS = 8                   # terms of one solve request
    supports_tiled_rhs = False          # solve(..., tiled=True) and matvec(..., tiled=True): tile-major right-hand sides
    supports_zero_rows = False          # solve(..., zero_rows=, skip_rows=) and matvec(..., owned=True)
    supports_mx_emission = False        # emits_mx / set_mx_band / solve(..., mx=)
    supports_pairing = False            # set_pairing
    supports_row_blocks = False         # set_row_blocks
    supports_state_tiling = False       # set_state_tiled
    supports_block_inverse = False      # set_block_inverse
    variant_epoch = 0                   # counts the changes of the sweep variant (layout decisions depend on it)
    flagged = MappingProxyType({})      # lu id -> cells whose band block is singular (a pack that flags keeps its own dict)

    def lu_bytes(self, lu_id):
        """Device memory of a factorization."""
        return 0


class PreContractPack(PackBase):
    """A pack written before this contract (no PackBase, `solve_lincomb(lu_id, xs, alphas, x)` plus `matvec` instead of the
    request) behind it: SolverBase wraps such a pack once, at construction, so that nothing else has to ask which kind it
    holds.  Only so that a solver still runs on an older executor; every pack of this repository inherits PackBase."""
    supports_pairing = True

    def __init__(self, inner):
        self.__dict__["inner"] = inner

    def __getattr__(self, name):
        return getattr(self.inner, name)

    def __setattr__(self, name, value):
        setattr(self.inner, name, value)

    def lu_bytes(self, lu_id):
        return self.inner.lu_bytes(lu_id)

    def solve(self, lu_id, xs, alphas, x, p_mat_id=None, work=None, **unsupported):
        if any(v not in (None, False) for v in unsupported.values()):
            raise ValueError("a pack without the contract takes terms and P only, not %s" % sorted(unsupported))
        self.inner.solve_lincomb(lu_id, xs, alphas, x if p_mat_id is None else work)
        if p_mat_id is not None:
            self.inner.matvec(p_mat_id, work, x)
