"""Seeded cases of the fused CFL reduction (ddh_grid_cfl_sum) at the edges of its launch shape, shared by
tests/test_cfl_sum_host.py and tests/test_gpu_cfl_sum_kernel.py.  The expected value of a case is NumPy in longdouble:
max over the grid of sum_t f_t with explicit broadcasting, written from the definitions of the reference (extras/
flow_tools.py:199-204, core/basis.py:6078-6113, 6156-6204), not from the product code.

A term is a dict in the executor's format (HipExecutor.cfl_sum_max) with host arrays: kind, data [ncomp][own grid],
bcast per axis; velocity: comp_axis (None = no basis along that component's axis), inv per component; shell: inv =
(inv_h, inv_dr) over the last axis; s2: inv_h."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
GUARD = 64
BLOCK, GRID_CAP = 256, 2048                       # cfl_sum_kernel: 256 threads, stream_grid caps the grid at 256 * 8 blocks
FULL = BLOCK * GRID_CAP
MAX_TERMS = 8

# n -> storage grid; primes stay one axis (a launch-shape edge does not depend on the factorisation)
SHAPES = {
    1: (1,), 255: (15, 17), 256: (16, 16), 257: (257, 1), FULL - 1: (FULL - 1,), FULL: (64, 128, 64), FULL + 1: (3, (FULL + 1) // 3),
    5 * 7 * 9: (5, 7, 9),
}
assert all(int(np.prod(s)) == n for n, s in SHAPES.items())
SIZES = sorted(SHAPES)
LISTS = ("one_velocity", "two_velocities_scalar", "scalar_bcast_first", "scalar_bcast_last", "scalar_constant",
         "shell_profile", "s2_scalar", "eight")
PLANTS = ("none", "first", "last")
CASES = [(name, n) for name in LISTS for n in SIZES]


def _own(shape, bcast):
    return tuple(1 if b else n for n, b in zip(shape, bcast))


def _velocity(rng, shape, bcast=None, skip=()):
    naxes = len(shape)
    bcast = [0] * naxes if bcast is None else list(bcast)
    own = _own(shape, bcast)
    comp_axis = [None if c in skip else c for c in range(naxes)]
    inv = [None if ax is None else rng.uniform(0.5, 2.0, shape[ax]) for ax in comp_axis]
    return dict(kind="velocity", data=rng.uniform(-1, 1, (naxes,) + own), bcast=bcast, comp_axis=comp_axis, inv=inv)


def _scalar(rng, shape, bcast=None):
    bcast = [0] * len(shape) if bcast is None else list(bcast)
    return dict(kind="scalar", data=rng.uniform(-1, 1, (1,) + _own(shape, bcast)), bcast=bcast)


def _shell(rng, shape):
    nr = shape[-1]
    return dict(kind="shell", data=rng.uniform(-1, 1, (3,) + tuple(shape)), bcast=[0] * len(shape),
                inv=(rng.uniform(0.5, 2.0, nr), rng.uniform(0.5, 2.0, nr)))


def _s2(rng, shape):
    return dict(kind="s2", data=rng.uniform(-1, 1, (2,) + tuple(shape)), bcast=[0] * len(shape), inv_h=float(rng.uniform(0.5, 2.0)))


def _flags(shape, which):
    """broadcast flags: along the first axis only, the last only, all axes, all but the last"""
    k = len(shape)
    return {"first": [1] + [0] * (k - 1), "last": [0] * (k - 1) + [1], "all": [1] * k, "profile": [1] * (k - 1) + [0]}[which]


def terms_of(name, n, plant="none"):
    """the term list of case (name, n); plant: the point made the maximum ("first" / "last" grid point; "none": wherever
    the random data puts it).  The first term of every list is a velocity on the full grid: the plant goes there."""
    shape = SHAPES[n]
    rng = np.random.default_rng([LISTS.index(name), n])
    if name == "one_velocity":
        terms = [_velocity(rng, shape)]
    elif name == "two_velocities_scalar":
        terms = [_velocity(rng, shape), _velocity(rng, shape), _scalar(rng, shape)]
    elif name in ("scalar_bcast_first", "scalar_bcast_last", "scalar_constant"):
        which = {"scalar_bcast_first": "first", "scalar_bcast_last": "last", "scalar_constant": "all"}[name]
        terms = [_velocity(rng, shape), _scalar(rng, shape, _flags(shape, which))]
    elif name == "shell_profile":
        terms = [_shell(rng, shape), _scalar(rng, shape, _flags(shape, "profile"))]
    elif name == "s2_scalar":
        terms = [_s2(rng, shape), _scalar(rng, shape)]
    else:
        several = len(shape) > 1
        terms = [_velocity(rng, shape), _scalar(rng, shape), _velocity(rng, shape, skip=(len(shape) - 1,) if several else ()),
                 _scalar(rng, shape, _flags(shape, "profile")), _s2(rng, shape), _shell(rng, shape),
                 _scalar(rng, shape, _flags(shape, "all")),
                 _velocity(rng, shape, bcast=_flags(shape, "first") if several else None, skip=(0,) if several else ())]
        assert len(terms) == MAX_TERMS
    assert terms[0]["kind"] != "scalar" and not any(terms[0]["bcast"])
    if plant != "none":
        flat = terms[0]["data"].reshape(terms[0]["data"].shape[0], -1)
        flat[0, 0 if plant == "first" else n - 1] = 1000.0         # inv >= 0.5: 500 or more against a sum below 50
    return terms, shape


def ncomp_of(terms):
    return max(t["data"].shape[0] for t in terms)


def _along(a, axis, naxes, dtype):
    sh = [1] * naxes
    sh[axis] = -1
    return np.asarray(a, dtype=dtype).reshape(sh)


def frequency_field(terms, shape, dtype=LD):
    """sum_t f_t on the grid, in `dtype` (longdouble: the reference value; float64: the direct evaluation)"""
    k = len(shape)
    total = np.zeros(shape, dtype=dtype)
    for t in terms:
        d = np.asarray(t["data"], dtype=dtype)
        if t["kind"] == "scalar":
            f = np.abs(d[0])
        elif t["kind"] == "velocity":
            f = np.zeros(d.shape[1:], dtype=dtype)
            for c, ax in enumerate(t["comp_axis"]):
                if ax is not None:
                    f = f + np.abs(d[c]) * _along(t["inv"][c], ax, k, dtype)
        elif t["kind"] == "shell":
            f = np.sqrt(d[0] * d[0] + d[1] * d[1]) * _along(t["inv"][0], k - 1, k, dtype) \
                + np.abs(d[2]) * _along(t["inv"][1], k - 1, k, dtype)
        else:
            f = np.sqrt(d[0] * d[0] + d[1] * d[1]) * dtype(t["inv_h"])
        total = total + np.broadcast_to(f, shape)
    return total


def expected(terms, shape):
    """(longdouble maximum, flat index where it sits)"""
    f = frequency_field(terms, shape).reshape(-1)
    at = int(np.argmax(f))
    return f[at], at
