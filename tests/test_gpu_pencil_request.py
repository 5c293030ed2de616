"""GPU: the request-based pencil solve and mat-vec (ddh_pencil_solve_req, DDH_MATVEC_*; include/dedalus_hip.h).

Rejections: on the smallest pack the tile-major path accepts (3-D Rayleigh-Benard, 8 x 8 storage columns, Nz = 8), on packs
with ny = 12 and with nx = 12, and on a one-Fourier-axis pack of 8 modes, one request per condition that violates exactly
that condition.  Each must raise DdhError with the message of that condition and leave x, prefilled with 7.0, untouched: the library refuses on the host
before it launches anything.
Agreement: valid requests in each form the library's former entry points had, bit for bit where those were defined to agree.
All cases run in one worker process (tests/pencil_request_worker.py: the sweep switches are read once per process, and the
8 x 8 pack needs the full-size sweeps to emit M.x)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# case of the worker -> what the message must contain
REJECTIONS = {
    "lu_id": "bad LU id",
    "p_mat_id": "bad matrix id",
    "m_mat_id": "bad matrix id",
    "no_terms": "1 to 8 right-hand-side terms",
    "nine_terms": "1 to 8 right-hand-side terms",
    "term_is_x": "in-place unsupported",
    "term_is_x_without_p": "in-place unsupported",
    "term_is_work": "in-place unsupported",
    "term_is_work_one_axis": "in-place unsupported",
    "no_work": "work and x must be distinct buffers",
    "work_is_x": "work and x must be distinct buffers",
    "no_mx_out": "M.x needs a vector of its own",
    "mx_out_is_x": "M.x needs a vector of its own",
    "mx_out_is_work": "M.x needs a vector of its own",
    "mx_without_tiled": "M.x needs tile-major terms",
    "mx_out_without_m_mat_id": "mx_out without m_mat_id",
    "mx_other_matrix": "have no tables for this matrix",
    "mx_not_emitted": "do not emit M.x",
    "masks_without_p": "row masks need p_mat_id",
    "skip_without_p": "row masks need p_mat_id",
    "tiled_without_p": "tile-major terms need p_mat_id",
    "mx_without_p": "M.x needs p_mat_id",
    "struct_size": "struct_size",
    "band_major_state_unfused": "a kx-band-major state needs the fused recombination",
    "tiled_not_lean": "does not run the lean forward sweep",
    "tiled_ny_12": "tile-major terms need two Fourier axes with storage sizes that are multiples of 8",
    "tiled_nx_12": "tile-major terms need two Fourier axes with storage sizes that are multiples of 8",
    "matvec_tiled_nx_12": "DDH_MATVEC_TILED needs two Fourier axes with storage sizes that are multiples of 8",
    "tiled_one_axis": "tile-major terms need two Fourier axes with storage sizes that are multiples of 8",
    "matvec_tiled_ny_12": "DDH_MATVEC_TILED needs two Fourier axes with storage sizes that are multiples of 8",
    "matvec_tiled_one_axis": "DDH_MATVEC_TILED needs two Fourier axes with storage sizes that are multiples of 8",
    "matvec_tiled_not_window_form": "only the window-form mat-vec",
    "matvec_flags": "unknown flags",
    "matvec_in_place": "in-place unsupported",
}
AGREE = ["one_term_and_eight", "null_masks_and_zero_masks", "unfused_p_and_matvec"]


@pytest.fixture(scope="module")
def result():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "pencil_request_worker.py")], capture_output=True, text=True,
                       timeout=600, env=dict(os.environ, DDH_SWEEP_DEEP="0"), cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    print(res)
    return res


def test_the_small_pack_emits_mx(result):
    # (else the requests with m_mat_id would violate two conditions at once)
    assert result["emits"] is True


def test_the_unfused_cases_ran_the_cooperative_backward_sweep(result):
    # (the sweep that cannot fuse P: what "mx_not_emitted", "band_major_state_unfused" and "unfused_p_and_matvec" rely on)
    assert result["unfused_backward_lanes"] == 4


def test_the_worker_ran_every_case(result):
    assert sorted(result["rejections"]) == sorted(REJECTIONS) and sorted(result["agree"]) == sorted(AGREE)


@pytest.mark.parametrize("case", sorted(REJECTIONS))
def test_request_is_refused_before_any_launch(result, case):
    raised, message, untouched = result["rejections"][case]
    assert raised, case
    assert REJECTIONS[case] in message, (case, message)
    assert untouched, case


@pytest.mark.parametrize("case", AGREE)
def test_former_forms_agree_bit_for_bit(result, case):
    assert result["agree"][case] is True
