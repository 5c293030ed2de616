"""Case tables and longdouble references for the pointwise map and broadcast kernels of dedalus_amd/csrc/ddh_gridmap.hip,
importable without a device.  tests/test_gpu_grid_map.py runs the kernels on them, tests/test_grid_map_host.py checks the
tables themselves, tests/test_gpu_pointwise_expressions.py uses the bounds for whole expressions.

Errors are measured against NumPy evaluated in np.longdouble on the same float64 inputs, in units of U |ref|."""
import numpy as np

import grid_cases as gc

LD, U, GUARD = gc.LD, gc.U, gc.GUARD
stream_tags = gc.stream_tags

# the ufuncs of the reference's UnaryGridFunction table (core/operators.py:534-556), by ufunc.__name__
UFUNCS = ("absolute sign exp exp2 log log2 log10 sqrt square sin cos tan arcsin arccos arctan sinh cosh tanh arcsinh "
          "arccosh arctanh").split()
OPS = UFUNCS + ["recip", "pow"]
# one IEEE operation per point and no fast-math in the build: bit for bit NumPy float64
EXACT = ("absolute", "sign", "square", "sqrt", "recip")
POW_EXACT = (0.5, -1)                       # run as sqrt / recip
SIZES = gc.LINCOMB_SIZES                    # 1, 2, 3, 255, 100003, 1048578, 3000001: tail only ... several passes
# (exponent, inputs): positive bases for every exponent, signed bases for the odd integer one
POW_CASES = ((3, "positive"), (-2, "positive"), (2.5, "positive"), (-0.5, "positive"), (3, "signed"),
             (0.5, "positive"), (-1, "positive"))

# Worst |error| / (U |ref|) per function over SIZES on the MI355X, rounded up to a whole ulp, plus one ulp (the inputs are
# one seeded sample; a neighbouring input may round the other way).  Source: profiles/grid_map_parity.txt, which also holds
# NumPy float64's own error on the same inputs.  "pow": the non-integer exponents of POW_CASES.
BOUNDS = {
    # every measured worst case lies between 1.02 U (cosh) and 1.99 U (pow): 2 U rounded up, 3 U with the extra ulp
    "exp": 3, "exp2": 3, "log": 3, "log2": 3, "log10": 3, "sin": 3, "cos": 3, "tan": 3, "arcsin": 3, "arccos": 3,
    "arctan": 3, "sinh": 3, "cosh": 3, "tanh": 3, "arcsinh": 3, "arccosh": 3, "arctanh": 3, "pow": 3,
}


def powi_bound(p):
    """|p| - 1 multiplications in sequence, one division for p < 0: (|p| - 1 + [p < 0]) U, derived"""
    return abs(int(p)) - 1 + (1 if p < 0 else 0)


def pow_is_repeated_multiplication(p):
    return float(p) == int(p) and 1 <= abs(int(p)) <= 8 and p not in POW_EXACT


def _seed(op, n, extra=0):
    return (OPS.index(op) * 7919 + n % 100003 + 31 * extra) % (1 << 31)


def map_input(op, n, kind="positive", p=0.0):
    """seeded float64 inputs inside the function's domain"""
    rng = np.random.default_rng(_seed(op, n, int(10 * p) + (kind == "signed")))
    if op in ("exp", "exp2", "sinh", "cosh"):
        return rng.uniform(-20.0, 20.0, n)
    if op in ("sin", "cos", "tan"):
        return rng.uniform(-100.0, 100.0, n)
    if op in ("log", "log2", "log10", "sqrt"):
        return 10.0 ** rng.uniform(-6.0, 6.0, n)                  # (0, 1e6]
    if op in ("arcsin", "arccos"):
        return rng.uniform(-1.0, 1.0, n)
    if op == "arccosh":
        return 10.0 ** rng.uniform(0.0, 6.0, n)                   # [1, 1e6]
    if op == "arctanh":
        x = rng.uniform(-1.0, 1.0, n) * (1.0 - 2.0 ** -30)        # (-1, 1)
        return x
    if op == "pow" and kind == "positive":
        return 10.0 ** rng.uniform(-3.0, 3.0, n)
    return rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)  # signed, never zero


def numpy_map(op, x, p=0.0):
    """NumPy's own result in the dtype of x (float64: what the host path computed; longdouble: the reference)"""
    with np.errstate(all="ignore"):
        if op == "recip":
            return 1 / x
        if op == "pow":
            if p == 0.5:
                return np.sqrt(x)
            if p == -1:
                return 1 / x
            return np.power(x, x.dtype.type(p))
        return getattr(np, op)(x)


def reference(op, x, p=0.0):
    return numpy_map(op, np.asarray(x, dtype=LD), p)


def ulp_ratio(got, ref):
    """worst |got - ref| / (U |ref|); where ref == 0 the result must be 0 too"""
    got, ref = np.asarray(got, dtype=LD), np.asarray(ref, dtype=LD)
    zero = ref == 0
    assert np.all(got[zero] == 0)
    if zero.all():
        return 0.0
    return float(np.max(np.abs(got[~zero] - ref[~zero]) / (U * np.abs(ref[~zero]))))


# ---- special values ---------------------------------------------------------------------------------------------------
OUT_OF_DOMAIN = {"log": -1.0, "log2": -1.0, "log10": -1.0, "sqrt": -1.0, "arcsin": 2.0, "arccos": -2.0, "arccosh": 0.5,
                 "arctanh": 2.0}
HUGE = 1.0e300                              # functions defined on the whole line get a huge finite argument instead
SPECIAL_N = 3000001                         # three grid-stride passes of 16-byte words and an odd last element
SPECIAL_POW = (3, -2, 2.5, -0.5)


def special_values(op, p=0.0):
    extra = OUT_OF_DOMAIN.get(op, HUGE)
    if op == "pow":
        extra = -1.5                        # negative base: NaN for the non-integer exponents
    return np.array([0.0, -0.0, np.inf, -np.inf, np.nan, extra])


def special_positions(n=SPECIAL_N):
    """start of the run of planted values at the first index, in the final grid-stride pass, at the last index"""
    k = len(special_values("exp"))
    n2 = n // 2
    last_start = ((n2 - 1) // gc.STREAM_PASS) * gc.STREAM_PASS
    assert last_start > 0
    mid = 2 * (last_start + (n2 - last_start) // 3)
    return (0, mid, n - k)


def special_input(op, p=0.0, kind="positive"):
    x = map_input(op, SPECIAL_N, kind, p)
    v = special_values(op, p)
    for at in special_positions():
        x[at:at + v.size] = v
    return x


# ---- broadcast --------------------------------------------------------------------------------------------------------
BROADCAST_SHAPES = ((1, 1, 2), (3, 5, 7), (4, 6, 258), (96, 8, 12))
BROADCAST_NCOMP = (1, 3)
BROADCAST_MASKS = tuple(tuple(bool(m >> k & 1) for k in range(3)) for m in range(1, 8))      # every non-empty mask
BROADCAST_CASES = [(s, m, c) for s in BROADCAST_SHAPES for m in BROADCAST_MASKS for c in BROADCAST_NCOMP]


def broadcast_input(shape, present, ncomp):
    """every entry distinct: -> (operand [ncomp][present axes, 1 elsewhere], np.broadcast_to of it, contiguous)"""
    src = tuple(s if p else 1 for s, p in zip(shape, present))
    a = (np.arange(ncomp * int(np.prod(src)), dtype=np.float64) + 0.25).reshape((ncomp,) + src)
    return a, np.ascontiguousarray(np.broadcast_to(a, (ncomp,) + tuple(shape)))
