"""GPU: ddh_ell_mix_apply (csrc/ddh_ellmix.hip) pinned at the edges of its launch shape (tests/shell_tensor_cases.py).

A longdouble evaluation of the same mix, entry by entry within (K + 2) u sum |q| |x| (K: the largest number of terms of one
output component, u = 2^-53; the form of tests/test_gpu_swsh_kernels.py).  Input and output sit inside NaN guards, and
every input slot without a mode -- the msin part of m = 0 among them -- holds NaN: those slots receive +0, nothing outside
the output changes, two calls give identical bits."""
import numpy as np
import pytest

import shell_tensor_cases as st

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
GUARD = 4096


@pytest.fixture(scope="module")
def ex():
    from dedalus_amd.executor import HipExecutor
    return HipExecutor()


def guarded(ex, n, fill, misalign):
    """n doubles inside NaN guards; misalign: the body starts 8 bytes off a 16-byte boundary"""
    lead = GUARD + (1 if misalign else 0)
    buf = ex.dev.empty((n + 2 * GUARD + 2,))
    buf.fill_(float("nan"))
    body = buf[lead:lead + n]
    body.fill_(fill)
    assert (body.data_ptr() % 16 == 8) == bool(misalign)
    return buf, body, lead


def guards_intact(ex, buf, lead, n):
    h = np.array(ex.download(buf))
    return np.isnan(h[:lead]).all() and np.isnan(h[lead + n:]).all()


def test_symbols_exported():
    from dedalus_amd import libhip
    assert {"ddh_ell_mix_create", "ddh_ell_mix_apply"} <= set(libhip.SIGNATURES)


@pytest.mark.parametrize("label", [c[0] for c in st.KERNEL_CASES])
def test_ell_mix_kernel_pinned(ex, label):
    nm, nl, nr, nco, nci, terms, slot_map, x, misalign = st.kernel_case(label)
    ref, mag, K = st.kernel_reference(nm, nl, nr, nco, terms, slot_map, x)
    dev = ex.make_ell_mix(nm, nl, nr, nco, nci, terms, slot_map)
    n = nco * 2 * nm * nl * nr
    xbuf, xd, xlead = guarded(ex, x.size, 0.0, misalign)
    xd.copy_(ex.from_host(np.ascontiguousarray(x)).reshape(-1))
    xd = xd.reshape(x.shape)
    outs = []
    for call in range(2):
        ybuf, yd, ylead = guarded(ex, n, 7.0, misalign)
        dev.apply(xd, yd.reshape(nco, 2 * nm, nl, nr))
        ex.sync()
        assert guards_intact(ex, ybuf, ylead, n), "the kernel wrote outside its output"
        outs.append(np.array(ex.download(yd)).reshape(nco, 2 * nm, nl, nr))
    assert guards_intact(ex, xbuf, xlead, x.size)
    y = outs[0]
    assert np.array_equal(y.view(np.uint64), outs[1].view(np.uint64)), "two calls differ"
    assert not np.isnan(y).any(), "a slot without a mode was read"
    dead = y[:, slot_map < 0, :]
    assert dead.size and np.all(dead.view(np.uint64) == 0), "slots without a mode must hold +0"
    bound = (K + 2) * U * mag
    err = np.abs(y.astype(np.longdouble) - ref)
    worst = float((err / np.maximum(bound, np.finfo(np.float64).tiny)).max())
    print("%s: worst error / bound %.3f, K = %d" % (label, worst, K))
    assert np.abs(ref).max() > 0.5 and np.all(err <= bound), (label, worst)
