"""Host: the request-based pencil solve (ddh_pencil_solve_req, include/dedalus_hip.h) as far as it can be checked without a
device -- the layout of the ctypes struct against the C struct, the timer's byte accounting of PencilPack.solve, and the
labels a parity probe records for the solve's feature sets."""
import ctypes as C
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

from dedalus_amd import libhip
from dedalus_amd.core.solvers import solve_path_label
from dedalus_amd.pencilpack import PencilPack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = [name for name, _ in libhip.PencilSolveReq._fields_]


def test_ctypes_request_has_the_layout_of_the_c_struct(tmp_path):
    cc = next((c for c in (os.environ.get("CC"), "cc", "gcc", "clang") if c and shutil.which(c)), None)
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include "dedalus_hip.h"\nint main(void) {\n'
                   '    printf("%zu\\n", sizeof(ddh_pencil_solve_req));\n'
                   + "".join('    printf("%%zu\\n", offsetof(ddh_pencil_solve_req, %s));\n' % f for f in FIELDS)
                   + '    printf("%d %d\\n", (int)DDH_MATVEC_OWNED, (int)DDH_MATVEC_TILED);\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    assert int(out[0]) == C.sizeof(libhip.PencilSolveReq)
    for f, line in zip(FIELDS, out[1:]):
        assert int(line) == getattr(libhip.PencilSolveReq, f).offset, f
    assert out[1 + len(FIELDS)].split() == [str(libhip.MATVEC_OWNED), str(libhip.MATVEC_TILED)]


class _Vec:
    def __init__(self, n):
        self.n = n

    def numel(self):
        return self.n


class _Mass:
    row = [0, 0, 1, 2, 5, 5]          # 4 of 6 rows have terms


NROWS, N, LU_BYTES = 6, 6 * 64, 1000000


def _pack(forward, lanes, real, binv):
    p = object.__new__(PencilPack)
    p.nrows, p.matrices = NROWS, [_Mass]
    p.lu_info = lambda lu: dict(forward=forward, backward_lanes=lanes, real=real)
    p.lu_bytes = lambda lu: LU_BYTES
    p._binv_bytes = {0: binv}
    return p


def _before(info, binv, xs, x, zero_rows, skip_rows, mx):
    """The two byte counts `solve_recombined` had, one per branch, before they became PencilPack.solve_bytes: they differ in
    the condition on skip_rows and in the block-inverse override, and the benchmark tools' numbers depend on both."""
    terms = sum(v.numel() for v in xs)
    read = 1.0 - (zero_rows[1] if (zero_rows is not None and info["forward"] == "lean") else 0.0)
    if mx is not None:
        wrote = 1.0 - (skip_rows[1] if skip_rows is not None else 0.0)
        mrows = len(np.unique(np.asarray(_Mass.row)))
        return LU_BYTES + (terms * read + x.numel() * wrote + mx[1].numel() * mrows / float(NROWS)) * 8
    wrote = 1.0 - (skip_rows[1] if (skip_rows is not None and info["backward_lanes"] == 0 and info["real"]) else 0.0)
    nb = LU_BYTES + (terms * read + x.numel() * wrote) * 8
    if binv:
        nb = binv + (terms + 3 * x.numel()) * 8
    return nb


# (forward, backward lanes, real, block-inverse bytes, zero fraction, skip fraction, mx) -> bytes, as recorded before the change
RECORDED = {
    ("lean", 0, 1, 0, None, None, None): 1012288.0,
    ("lean", 0, 1, 0, 0.25, None, None): 1009984.0,
    ("lean", 0, 1, 0, None, 0.5, None): 1010752.0,
    ("lean", 0, 1, 0, 0.25, 0.5, None): 1008448.0,
    ("lean", 0, 1, 0, None, None, 1): 1014336.0,
    ("lean", 0, 1, 0, 0.25, 0.5, 1): 1010496.0,
    ("lean", 4, 1, 0, 0.25, 0.5, None): 1009984.0,          # the cooperative backward sweep stores every unknown ...
    ("lean", 4, 1, 0, 0.25, 0.5, 1): 1010496.0,             # ... but the branch with M.x never asked which sweep runs
    ("general", 4, 0, 0, 0.25, 0.5, None): 1012288.0,
    ("general", 4, 0, 0, 0.25, 0.5, 1): 1012800.0,
    ("lean", 0, 1, 4096, 0.25, 0.5, None): 22528,           # block inverses replace the factors ...
    ("lean", 0, 1, 4096, 0.25, 0.5, 1): 1010496.0,          # ... but not in the branch with M.x
}


def test_solve_bytes_are_those_of_the_former_entry_points():
    xs, x = [_Vec(N)] * 3, _Vec(N)
    seen = 0
    for forward, lanes, real, binv, z, k, m in itertools.product(("lean", "general"), (0, 4), (1, 0), (0, 4096), (None, 0.25),
                                                                 (None, 0.5), (None, 1)):
        p = _pack(forward, lanes, real, binv)
        zero_rows = None if z is None else (_Vec(NROWS), z)
        skip_rows = None if k is None else (_Vec(NROWS), k)
        mx = None if m is None else (0, _Vec(N))
        got = p.solve_bytes(0, xs, x, 3, zero_rows, skip_rows, mx)
        assert got == _before(p.lu_info(0), binv, xs, x, zero_rows, skip_rows, mx), (forward, lanes, real, binv, z, k, m)
        key = (forward, lanes, real, binv, z, k, m)
        if key in RECORDED:
            assert got == RECORDED[key] and type(got) is type(RECORDED[key]), key
            seen += 1
    assert seen == len(RECORDED)
    # without P: the factors, the terms and x, whatever the factorization (formerly `solve` and `solve_lincomb`)
    p = _pack("lean", 0, 1, 4096)
    assert p.solve_bytes(0, [x], x) == 1006144 and p.solve_bytes(0, xs, x) == 1012288


def test_timer_receives_solve_bytes():
    class Timer:
        def run(self, name, nb, fn, *args):
            self.got = (name, nb, fn, args)

    class Executor:
        timer = Timer()

    p = _pack("lean", 0, 1, 0)
    p.executor = Executor()
    xs, x, work = [_Vec(N)] * 2, _Vec(N), _Vec(N)
    zero_rows = (_Vec(NROWS), 0.25)
    p.solve(0, xs, [1.0, 2.0], x, p_mat_id=3, work=work, zero_rows=zero_rows, tiled=True)
    name, nb, fn, args = Executor.timer.got
    assert name == "pencil_solve" and nb == p.solve_bytes(0, xs, x, 3, zero_rows, None, None)
    assert fn == p._solve and args == (0, xs, [1.0, 2.0], x, 3, work, zero_rows, None, True, None)


def test_probe_labels_are_the_recorded_ones():
    assert solve_path_label(False) == "ddh_pencil_solve_lincomb"
    assert solve_path_label(True) == "ddh_pencil_solve_recombined"
    assert solve_path_label(True, masks=True) == "ddh_pencil_solve_recombined_sparse"
    assert solve_path_label(True, tiled=True) == solve_path_label(True, masks=True, tiled=True) == "ddh_pencil_solve_recombined_tiled"
    assert solve_path_label(True, masks=True, tiled=True, mx=True) == solve_path_label(True, tiled=True, mx=True) \
        == "ddh_pencil_solve_recombined_tiled_mx"
