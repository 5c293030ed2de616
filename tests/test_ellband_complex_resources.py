"""Compiler resource figures of csrc/ddh_ellband.hip (no GPU).
Plain compile (tests/test_kernel_resources.py::_usage, WITHOUT the unroll threshold of dedalus_amd/build.py::FILE_FLAGS):
every complex factor and sweep instance keeps its windows in registers (no scratch), and the real instances report the
VGPR and scratch figures they had before the complex instances were added, read from that source with the same command --
the real sweeps' figures below include the scratch this plain compile gives their wider windows, which the library's own
flags remove.
The shipped configuration (the flags of dedalus_amd/build.py, FILE_FLAGS included): no instance, real or complex, has
scratch."""
import os
import re
import subprocess

from test_kernel_resources import CSRC, _usage

# instance -> (VGPRs, scratch bytes / lane) on the parent commit
REAL = {
    "ellband_factor_kernelE": (27, 0),
    "ellband_forward_kernelILi12E": (120, 0),
    "ellband_forward_kernelILi20E": (164, 0),
    "ellband_forward_kernelILi28E": (135, 720),
    "ellband_forward_kernelILi36E": (92, 944),
    "ellband_backward_kernelILi24E": (126, 0),
    "ellband_backward_kernelILi40E": (164, 0),
    "ellband_backward_kernelILi56E": (124, 464),
    "ellband_backward_kernelILi64E": (166, 528),
    "ellband_backward_kernelILi96E": (88, 976),
}
COMPLEX = ["ellband_factor_cx_kernelE"] + ["ellband_forward_cx_kernelILi%dE" % nw for nw in (12, 20, 28, 36)] \
    + ["ellband_backward_cx_kernelILi%dE" % wt for wt in (24, 40, 56, 64)]


def test_complex_instances_have_no_scratch_and_real_instances_are_unchanged():
    u = _usage("ddh_ellband.hip")

    def one(tag):
        hit = [k for k in u if tag in k]
        assert len(hit) == 1, (tag, list(u))
        return u[hit[0]]
    for tag in COMPLEX:
        assert one(tag)["scratch"] == 0, (tag, one(tag))
    assert not [k for k in u if "ellband_backward_cx_kernelILi96E" in k]        # (does not fit the registers: refused at create)
    for tag, (vgprs, scratch) in REAL.items():
        got = one(tag)
        assert (got["vgprs"], got["scratch"]) == (vgprs, scratch), (tag, got)


def test_no_instance_of_the_shipped_build_has_scratch():
    from dedalus_amd import build
    cmd = [build._hipcc()] + build.FLAGS + build.FILE_FLAGS["ddh_ellband.hip"] + [
        "--cuda-device-only", "-c", os.path.join(CSRC, "ddh_ellband.hip"), "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(names) == len(scratch) and len(names) >= len(REAL) + len(COMPLEX)
    for tag in list(REAL) + COMPLEX:
        hit = [sc for n, sc in zip(names, scratch) if tag in n]
        assert hit == [0], (tag, hit)
