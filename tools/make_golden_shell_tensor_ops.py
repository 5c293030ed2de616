"""Golden data of the shell transpose and radial component: runs the unmodified reference on the CPU (oracle.refshim; the
spin recombination needs oracle/_ref from `python oracle/build_ref.py`) over the cases of tests/shell_tensor_cases.py and
writes tests/golden/shell_tensor_ops.npz and tests/golden/shell_tensor_volume.npz (two files: each stays well under 1 MB).

    python tools/make_golden_shell_tensor_ops.py

Per shape `<shape>/`: the input coefficients `in_u` (float32 values, so no test depends on a random stream and the file
stays small) and the reference's result of every task as coefficients (`<task>`, float64).  The reference has no
RadialComponent of a shell (volume) operand: for those tasks (second file) the stored result is the reference's own coordinate component,
operand['g'] sliced at the radial entry of the index and transformed back in the operand's basis."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import refshim  # noqa: E402
import shell_tensor_cases as st  # noqa: E402
from make_golden_shell_vector_ops import random_input  # noqa: E402


def main():
    d3 = refshim.load_reference()
    out, vol = {}, {}
    for si, shape in enumerate(st.OP_SHAPES):
        coords, dist, shell, u = st.build(d3, shape)
        key = st.tag(shape) + "/"
        out[key + "in_u"] = random_input(u, 11 + si)

        def reset():
            u.change_scales(1)
            u["c"] = out[key + "in_u"].astype(np.float64)

        for name, expr in st.ref_tasks(d3, u).items():
            reset()
            res = expr.evaluate()
            res.change_scales(1)
            out[key + name] = np.array(res["c"])
        for name, (operand, index) in st.volume_operands(d3, u).items():
            reset()
            full = operand.evaluate()
            full.change_scales(1)
            comp = dist.Field(bases=full.domain.bases, tensorsig=full.tensorsig[:index] + full.tensorsig[index + 1:])
            comp["g"] = np.take(np.array(full["g"]), 2, axis=index)
            vol[key + name] = np.array(comp["c"])
        for d in (out, vol):
            for name, a in d.items():
                if name.startswith(key):
                    print(name, a.shape, float(np.abs(a).max()))
    for fname, d in (("shell_tensor_ops.npz", out), ("shell_tensor_volume.npz", vol)):
        path = os.path.join(ROOT, "tests", "golden", fname)
        np.savez_compressed(path, **d)
        print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
