"""The banded term-list kernel (csrc/ddh_sphere.hip): both instances of ell_terms_kernel (with and without rotated terms)
keep their eight accumulators in registers, without scratch, read from the compiler's resource report (no GPU needed)."""
from test_kernel_resources import _usage


def test_ell_terms_kernel_has_no_scratch():
    u = _usage("ddh_sphere.hip")
    hot = {k: v for k, v in u.items() if "ell_terms_kernel" in k}
    assert len(hot) == 2, list(u)
    for k, v in hot.items():
        print(k, v)
        assert v["scratch"] == 0, (k, v)
