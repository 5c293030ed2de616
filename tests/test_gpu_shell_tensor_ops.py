"""GPU: transpose and radial component of shell tensor fields on the device, through the public d3 names, against the
reference's results (tests/golden/shell_tensor_ops.npz, shell_tensor_volume.npz) with the bound of
tests/test_shell_tensor_ops.py (relative L2 error <= 1e-12)."""
import numpy as np
import pytest

import shell_tensor_cases as st
import test_shell_tensor_ops as host

pytestmark = pytest.mark.gpu


def test_public_names_dispatch_to_the_shell_gpu():
    import dedalus_amd.public as d3
    from dedalus_amd.core.shell import ShMix
    coords, dist, shell, u = st.build(d3, (8, 4, 6))
    assert isinstance(d3.trans(d3.grad(u)), ShMix) and isinstance(d3.radial(u), ShMix)      # not the Cartesian operator
    assert isinstance(d3.angular(u(r=0.7)), ShMix) and dist.executor.name == "hip"


@pytest.mark.parametrize("shape", st.OP_SHAPES, ids=st.tag)
def test_tensor_ops_match_reference_gpu(shape):
    host.check_tasks(shape, None)


def test_transpose_runs_the_mix_kernel_and_repeats_its_bits():
    import dedalus_amd.public as d3
    from dedalus_amd.executor import EllMix
    coords, dist, shell, u = st.build(d3, (20, 10, 9))
    u["c"] = host.GOLD["20x10x9/in_u"].astype(np.float64)
    node = d3.trans(d3.grad(u))
    a = np.array(node.evaluate()["c"])
    b = np.array(node.evaluate()["c"])
    assert isinstance(node._dev[1], EllMix)
    assert np.abs(a).max() > 1 and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_products_are_transposed_on_the_grid_gpu():
    import dedalus_amd.public as d3
    coords, dist, shell, u = st.build(d3, (8, 4, 6))
    u["c"] = host.GOLD["8x4x6/in_u"].astype(np.float64)
    uu = u * u
    ex = dist.executor
    g = np.array(ex.download(uu.eval_g()))
    gt = np.array(ex.download(d3.trans(uu).eval_g()))
    assert np.array_equal(gt.reshape((3, 3) + g.shape[1:]), g.reshape((3, 3) + g.shape[1:]).transpose(1, 0, 2, 3, 4))
