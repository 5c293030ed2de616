"""Register budget of the backward sweep that also writes M.X (solve_backward_kernel<2, 17, true, false, true, 4, true>, read
from the compiler like tests/test_kernel_resources.py; no GPU needed).

The instance runs at 4 waves per SIMD, i.e. within 128 VGPRs.  Compiler figures when the instance was added: the plain
fused sweep <..., 4, false> 128 VGPRs / 12 bytes of scratch per lane, the emitting one 128 VGPRs / 40 bytes (101 scalar
registers: the 18 wave-uniform coefficients of a row of M P); without the occupancy bound the emitting instance takes 140
VGPRs and no scratch.  In the ISA the 40 bytes are five stores in front of the row loop's header and five reloads behind its
exit (loop-invariant values saved once per thread, like the plain instance's 12 bytes); the loop itself touches no scratch.
The bounds below are those figures: a value spilled inside the loop would add to them."""
import pytest

from test_kernel_resources import _usage


def test_emitting_backward_sweep_keeps_its_registers():
    u = _usage("ddh_pencil.hip")
    emit = [n for n in u if "solve_backward_kernelILi2ELi17ELb1ELb0ELb1ELi4ELb1E" in n]
    plain = [n for n in u if "solve_backward_kernelILi2ELi17ELb1ELb0ELb1ELi4ELb0E" in n]
    assert len(emit) == 1 and len(plain) == 1, [n for n in u if "solve_backward_kernel" in n]
    print(emit[0], u[emit[0]], plain[0], u[plain[0]])
    assert u[emit[0]]["vgprs"] <= 128 and u[emit[0]]["waves"] >= 4 and u[emit[0]]["scratch"] <= 40, u[emit[0]]
    assert u[plain[0]]["vgprs"] <= 128 and u[plain[0]]["waves"] >= 4 and u[plain[0]]["scratch"] <= 12, u[plain[0]]
