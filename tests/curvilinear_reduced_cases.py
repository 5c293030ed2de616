"""Reduced analysis tasks of sphere and shell fields (slices along phi / theta, zonal means, shell averages) shared by the
golden generator (tools/make_golden_curvilinear_reduced.py, run against the reference) and the tests (run against
dedalus_amd): the SAME text builds the fields and the task expressions from whichever d3 namespace it is given.  Inputs
are coefficient arrays stored in tests/golden/curvilinear_reduced.npz."""
import numpy as np

DEALIAS = 3 / 2
# case -> (kind, shape, radii or radius)
CASES = {
    "shell_16_12_8": ("shell", (16, 12, 8), (0.7, 1.9)),
    "shell_16_10_6": ("shell", (16, 10, 6), (1.0, 2.5)),
    "sphere_16_8": ("sphere", (16, 8), 1.0),
    "sphere_12_10": ("sphere", (12, 10), 2.0),
}
SCALES = (1.0, 1.5)


def out_key(scale):
    return "g1" if scale == 1.0 else "g15"


def build(d3, case, dist_kw=None):
    """-> (dist, coords, basis, fields by name)"""
    kind, shape, size = CASES[case]
    if kind == "shell":
        coords = d3.SphericalCoordinates("phi", "theta", "r")
        dist = d3.Distributor(coords, dtype=np.float64, **(dist_kw or {}))
        basis = d3.ShellBasis(coords, shape=shape, radii=size, dealias=DEALIAS, dtype=np.float64)
        f = dict(b=dist.Field(name="b", bases=basis), u=dist.VectorField(coords, name="u", bases=basis))
        er = dist.VectorField(coords, bases=basis.radial_basis)
        er["g"][2] = 1
        f["er"] = er
    else:
        coords = d3.S2Coordinates("phi", "theta")
        dist = d3.Distributor(coords, dtype=np.float64, **(dist_kw or {}))
        basis = d3.SphereBasis(coords, shape, radius=size, dealias=DEALIAS, dtype=np.float64)
        f = dict(h=dist.Field(name="h", bases=basis), v=dist.VectorField(coords, name="v", bases=basis))
    return dist, coords, basis, f


def input_names(case):
    return ("b", "u") if CASES[case][0] == "shell" else ("h", "v")


def tasks(d3, case, coords, f):
    """name -> expression, in a fixed order"""
    t = {}
    phi = coords["phi"]
    if CASES[case][0] == "shell":
        b, u, er, S2 = f["b"], f["u"], f["er"], coords.S2coordsys
        t["b_theta"] = b(theta=0.7)
        t["u_theta"] = u(theta=0.7)
        t["bu_theta"] = (b * u)(theta=2.1)
        t["b_theta_equator"] = b(theta=np.pi / 2)
        t["b_phi"] = b(phi=1.0)
        t["u_phi"] = u(phi=1.0)
        t["flux_phi"] = (er @ (u * b))(phi=3 * np.pi / 2)
        t["ave_phi_b"] = d3.Average(b, phi)
        t["ave_phi_u"] = d3.Average(u, phi)
        t["ave_S2_b"] = d3.Average(b, S2)
        t["ave_S2_buu"] = d3.Average(b * (u @ u), S2)
    else:
        h, v = f["h"], f["v"]
        t["h_theta"] = h(theta=0.7)
        t["v_theta"] = v(theta=0.7)
        t["hv_theta"] = (h * v)(theta=2.1)
        t["h_theta_equator"] = h(theta=np.pi / 2)
        t["h_phi"] = h(phi=1.0)
        t["v_phi"] = v(phi=1.0)
        t["hv_phi"] = (h * v)(phi=3 * np.pi / 2)
        t["ave_phi_h"] = d3.Average(h, phi)
        t["ave_phi_v"] = d3.Average(v, phi)
    return t


def load_inputs(gold, case, f):
    """Set the fields from the stored coefficient arrays (float32 values: exactly representable, half the file)."""
    for k in input_names(case):
        f[k]["c"] = gold["%s/in/%s" % (case, k)].astype(np.float64)


def record(out, scales=SCALES):
    """{key: array} of an evaluated task: 'g' at scales 1 and 3/2.  The reference returns the two interpolations as fields
    locked to the scales they were formed at (the dealias scales): a scale it refuses is left out."""
    res = {}
    for scale in scales:
        try:
            out.change_scales(scale)
        except ValueError:
            continue
        res[out_key(scale)] = np.array(out["g"])
    return res
