"""Reduced analysis tasks (slices, profiles, integrals) shared by the golden generator (tools/make_golden_reduced.py, run
against the reference) and the tests (run against dedalus_amd): the SAME text builds the fields and the task expressions
from whichever d3 namespace it is given.  Inputs are coefficient arrays stored in tests/golden/reduced_tasks.npz."""
import numpy as np

DEALIAS = 3 / 2
# case -> (coordinate names, sizes, bounds)
CASES = {
    "f1": (("x",), (64,), ((1.0, 11.0),)),
    "rb2d": (("x", "z"), (64, 32), ((-1.0, 3.0), (0.0, 1.0))),
    "rb3d": (("x", "y", "z"), (32, 32, 16), ((0.0, 4.0), (-2.0, 2.0), (0.0, 1.0))),
}
OUTPUTS = (("c", 1.0), ("g", 1.0), ("g", 1.5))          # (layout, scale) recorded per task


def out_key(layout, scale):
    return layout if layout == "c" else ("g1" if scale == 1.0 else "g15")


def build(d3, case, dist_kw=None):
    """-> (dist, coordinates by name, bases by name, fields by name)"""
    names, sizes, bounds = CASES[case]
    if len(names) == 1:
        cs = d3.Coordinate(names[0])
        cd = {names[0]: cs}
    else:
        cs = d3.CartesianCoordinates(*names)
        cd = {n: cs[n] for n in names}
    dist = d3.Distributor(cs, dtype=np.float64, **(dist_kw or {}))
    bases = {}
    for n, N, bd in zip(names, sizes, bounds):
        if n == "z":
            bases[n] = d3.ChebyshevT(cd[n], size=N, bounds=bd, dealias=DEALIAS)
        else:
            bases[n] = d3.RealFourier(cd[n], size=N, bounds=bd, dealias=DEALIAS)
    B = tuple(bases[n] for n in names)
    f = dict(b=dist.Field(name="b", bases=B))
    if len(names) > 1:
        f["u"] = dist.VectorField(cs, name="u", bases=B)
        f["ez"] = cs.unit_vector_fields(dist)[-1]
    return dist, cd, bases, f


def positions(case):
    names, sizes, bounds = CASES[case]
    lo, hi = bounds[0]
    p = dict(x_on=lo + (hi - lo) * 5 / sizes[0], x_off=lo + 0.3137 * (hi - lo))
    if "y" in names:
        ylo, yhi = bounds[names.index("y")]
        p["y0"] = ylo + 0.777 * (yhi - ylo)
    if "z" in names:
        p["z0"] = 0.37
    return p


def tasks(d3, case, cd, f):
    """name -> expression, in a fixed order"""
    names = CASES[case][0]
    p = positions(case)
    b = f["b"]
    x = cd["x"]
    dx = lambda A: d3.Differentiate(A, x)
    t = {}
    t["b_x_on"] = b(x=p["x_on"])
    t["b_x_off"] = b(x=p["x_off"])
    t["b_x_left"] = b(x="left")
    t["dx_of_b_x"] = dx(b(x=p["x_off"]))
    t["ave_x"] = d3.Average(b, x)
    t["integ_x"] = d3.Integrate(b, x)
    t["integ_all"] = d3.Integrate(b)
    if "z" in names:
        u, ez, z = f["u"], f["ez"], cd["z"]
        dz = lambda A: d3.Differentiate(A, z)
        hor = tuple(cd[n] for n in names if n != "z")
        t["u_x"] = u(x=p["x_off"])
        t["b_x_z"] = b(x=p["x_off"])(z=p["z0"])
        t["dz_b_x"] = dz(b)(x=p["x_off"])
        t["ave_hor"] = d3.Average(b, hor)
        t["ave_flux_hor"] = d3.Average(b * (u @ ez), hor)
        t["ave_x_times_ave_x"] = d3.Average(b, x) * d3.Average(u @ ez, x)
        t["ave_x_z"] = d3.Average(b, x)(z=p["z0"])
    if "y" in names:
        t["b_y"] = b(y=p["y0"])
    return t


def load_inputs(gold, case, f):
    """Set the fields from the stored coefficient arrays (float32 values: exactly representable, half the file)."""
    for k in ("b", "u"):
        if k in f:
            f[k]["c"] = gold["%s/in/%s" % (case, k)].astype(np.float64)


def record(out):
    """{key: array} of an evaluated task: 'c' at scale 1, 'g' at scales 1 and 3/2"""
    res = {}
    for layout, scale in OUTPUTS:
        out.change_scales(scale)
        res[out_key(layout, scale)] = np.array(out[layout])
    return res
