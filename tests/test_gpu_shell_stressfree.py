"""GPU: the stress-free LBVP and convection runs of tests/test_shell_stressfree.py on the device (same bounds), the IVP
through the per-ell band LU with the coupled boundary rows or its dense fallback, whichever the plan chooses."""
import pytest

import test_shell_stressfree as host

pytestmark = pytest.mark.gpu


def test_stressfree_lbvp_gpu():
    solver = host.check_lbvp(None)
    assert solver.ex.name == "hip"


@pytest.mark.parametrize("ts", ["RK222", "SBDF2"])
def test_stressfree_convection_end_state_gpu(ts):
    solver = host.check_convection(ts, None)
    assert solver.ex.name == "hip"
    band = solver._band
    print("LHS path:", "dense inverses" if not band else "band LU, dense for ell in %s" % (band["plan"].dense_groups,))
    assert band is not None
