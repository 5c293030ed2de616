"""The component-mix kernel (csrc/ddh_ellmix.hip) is a streaming kernel: both instances (16-byte and 8-byte units) keep
their accumulators in registers, without scratch, read from the compiler's resource report (no GPU needed)."""
from test_kernel_resources import _usage


def test_ell_mix_kernel_has_no_scratch():
    u = _usage("ddh_ellmix.hip")
    hot = {k: v for k, v in u.items() if "ell_mix_kernel" in k}
    assert len(hot) == 2, list(u)
    for k, v in hot.items():
        print(k, v)
        assert v["scratch"] == 0 and v["vgprs"] <= 64 and v["waves"] >= 8, (k, v)
