"""Golden data of the shell cross product and curl: runs the unmodified reference on the CPU (oracle.refshim; the spin
recombination needs oracle/_ref from `python oracle/build_ref.py`) over the cases of tests/shell_vector_cases.py and
writes tests/golden/shell_vector_ops.npz.

    python tools/make_golden_shell_vector_ops.py

Per case `<kind>/<shape>/`: the input coefficient arrays (`in_u`, `in_v`; float32 values, so no test depends on a random
stream and the file stays small) and the reference's result of every task as coefficients (`<task>`, float64)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import refshim  # noqa: E402
import shell_vector_cases as sv  # noqa: E402


def random_input(field, seed):
    """Random coefficients in every valid mode (one grid round trip drops the invalid ones), rounded to float32."""
    field.fill_random("c", seed=seed, distribution="standard_normal")
    field.change_scales(1)
    field["g"] = np.array(field["g"])
    c32 = np.array(field["c"]).astype(np.float32)
    field["c"] = c32.astype(np.float64)
    return c32


def numexpr_stand_in():
    """numexpr is not installed where the fixtures are made and the shim seeds an import stub for it; the reference's
    CrossProduct.operate hands numexpr plain arithmetic on arrays of its own frame, which NumPy evaluates as well."""
    def evaluate(expr, out=None, **kw):
        res = eval(expr, {"__builtins__": {}}, dict(sys._getframe(1).f_locals))
        if out is None:
            return res
        out[...] = res
        return out
    sys.modules["numexpr"].evaluate = evaluate


def main():
    d3 = refshim.load_reference()
    try:
        import numexpr
        numexpr.evaluate("a + 1", local_dict=dict(a=np.zeros(1)))
    except Exception:
        numexpr_stand_in()
    out = {}
    for kind, shapes in (("curl", sv.CURL_SHAPES), ("cross", sv.CROSS_SHAPES)):
        for si, shape in enumerate(shapes):
            coords, dist, shell, u, v = sv.build(d3, shape)
            key = "%s/%s/" % (kind, sv.tag(shape))
            out[key + "in_u"] = random_input(u, 7 + si)
            if kind == "cross":
                out[key + "in_v"] = random_input(v, 70 + si)
            tasks = sv.curl_tasks(d3, u) if kind == "curl" else sv.cross_tasks(d3, coords, dist, shell, u, v)
            for name, expr in tasks.items():
                for f, k in ((u, "in_u"), (v, "in_v")):          # every task starts from the stored coefficients
                    if key + k in out:
                        f.change_scales(1)
                        f["c"] = out[key + k].astype(np.float64)
                res = expr.evaluate()
                res.change_scales(1)
                out[key + name] = np.array(res["c"])
                print(key + name, out[key + name].shape, float(np.abs(out[key + name]).max()))
    path = os.path.join(ROOT, "tests", "golden", "shell_vector_ops.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
