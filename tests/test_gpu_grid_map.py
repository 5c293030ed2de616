"""GPU: ddh_grid_map and ddh_grid_broadcast (dedalus_amd/csrc/ddh_gridmap.hip) through the C ABI and HipExecutor, on the
cases of tests/grid_map_cases.py.

  absolute sign square sqrt recip, pow at p = 0.5 and p = -1     bit for bit NumPy float64 (one IEEE operation per point)
  integer powers by repeated multiplication                      |error| <= (|p| - 1 + [p < 0]) U |ref|, derived
  every other function                                           |error| <= BOUNDS[op] U |ref| against NumPy in longdouble;
                                                                 BOUNDS is the measured worst case rounded up plus one ulp
  broadcast                                                      bit for bit np.broadcast_to
Every output buffer carries 64 guard doubles past its end, NaN before the call and still NaN after it; the payload is
NaN-filled too and holds no NaN afterwards.  With DDH_GRID_MAP_PARITY_OUT=<file> the worst error per function, and NumPy
float64's own on the same inputs, are written there (profiles/grid_map_parity.txt)."""
import ctypes as C
import os

import numpy as np
import pytest

import grid_map_cases as mc

pytestmark = pytest.mark.gpu

RATIOS = {}            # function -> [worst device error, worst NumPy float64 error], in U |ref|


def note(name, dev, host):
    r = RATIOS.setdefault(name, [0.0, 0.0])
    r[0], r[1] = max(r[0], float(dev)), max(r[1], float(host))


@pytest.fixture(scope="module", autouse=True)
def parity_record():
    yield
    path = os.environ.get("DDH_GRID_MAP_PARITY_OUT")
    if path:
        with open(path, "w") as fh:
            fh.write("# worst |error| / (U |ref|), U = 2^-53, ref = NumPy in longdouble on the same float64 inputs, over the\n"
                     "# sizes %s (tests/test_gpu_grid_map.py, tests/grid_map_cases.py); 0 = bit for bit\n"
                     % " ".join(str(n) for n in mc.SIZES))
            fh.write("# %-20s %12s %14s\n" % ("function", "ddh_grid_map", "numpy float64"))
            for name, (dev, host) in sorted(RATIOS.items()):
                fh.write("%-22s %12.4f %14.4f\n" % (name, dev, host))


@pytest.fixture(scope="module")
def ex():
    from dedalus_amd.executor import HipExecutor
    return HipExecutor()


def launches():
    from dedalus_amd import libhip
    count = C.c_long(-1)
    libhip.call("ddh_grid_map_launches", C.byref(count))
    return count.value


def guarded(ex, n, offset=0):
    """-> (buffer of offset + n + GUARD doubles, all NaN; view of n doubles starting `offset` doubles in)"""
    buf = ex.dev.empty(offset + n + mc.GUARD)
    buf.fill_(float("nan"))
    return buf, buf[offset:offset + n]


def payload(ex, buf, n, offset=0, nan_ok=False):
    ex.sync()
    host = ex.download(buf)
    assert host.size == offset + n + mc.GUARD
    assert np.isnan(host[:offset]).all() and np.isnan(host[offset + n:]).all(), "guard region overwritten"
    assert nan_ok or not np.isnan(host[offset:offset + n]).any(), "payload entries left unwritten"
    return host[offset:offset + n]


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def check(op, p, x, got, tag=None):
    """the parity rule of one function on one input array; records and returns the device's worst error"""
    name = tag or op
    if op in mc.EXACT or (op == "pow" and p in mc.POW_EXACT):
        assert same_bits(got, mc.numpy_map(op, x, p)), name
        note(name, 0.0, 0.0)
        return 0.0
    ref = mc.reference(op, x, p)
    dev, host = mc.ulp_ratio(got, ref), mc.ulp_ratio(mc.numpy_map(op, x, p), ref)
    note(name, dev, host)
    if op == "pow" and mc.pow_is_repeated_multiplication(p):
        bound = mc.powi_bound(p)
    else:
        bound = mc.BOUNDS.get(op)
    print("%s n=%d error %.4f U (numpy float64 %.4f U), bound %s U" % (name, x.size, dev, host, bound))
    assert bound is not None, "no bound recorded for %s" % op
    assert dev <= bound, (name, x.size, dev, bound)
    return dev


def pow_tag(p, kind="positive"):
    return "pow p=%g%s" % (p, " signed" if kind == "signed" else "")


# ---- every op at every size -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", mc.SIZES)
@pytest.mark.parametrize("op", [o for o in mc.OPS if o != "pow"])
def test_map(ex, op, n):
    x = mc.map_input(op, n)
    before = launches()
    buf, out = guarded(ex, n)
    ex.grid_map(out, ex.from_host(x), op)
    got = payload(ex, buf, n)
    assert launches() == before + 1
    check(op, 0.0, x, got)


@pytest.mark.parametrize("n", mc.SIZES)
@pytest.mark.parametrize("p,kind", mc.POW_CASES)
def test_pow(ex, p, kind, n):
    x = mc.map_input("pow", n, kind, p)
    buf, out = guarded(ex, n)
    ex.grid_map(out, ex.from_host(x), "pow", p)
    got = payload(ex, buf, n)
    integer = mc.pow_is_repeated_multiplication(p)
    check("pow", p, x, got, tag=pow_tag(p, kind) if integer or p in mc.POW_EXACT else "pow")
    if not integer and p not in mc.POW_EXACT:
        note(pow_tag(p, kind), mc.ulp_ratio(got, mc.reference("pow", x, p)),
             mc.ulp_ratio(mc.numpy_map("pow", x, p), mc.reference("pow", x, p)))


# ---- special values ---------------------------------------------------------------------------------------------------
def _same_specials(got, ref):
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "NaN-ness differs from NumPy's"
    inf = np.isinf(ref)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], ref[inf]), "infinities differ from NumPy's"
    zero = ref == 0
    assert np.array_equal(got == 0, zero) and np.array_equal(np.signbit(got[zero]), np.signbit(ref[zero])), \
        "zeros or their signs differ from NumPy's"


@pytest.mark.parametrize("op,p", [(o, 0.0) for o in mc.OPS if o != "pow"] + [("pow", p) for p in mc.SPECIAL_POW])
def test_special_values_are_numpys(ex, op, p):
    """+-0, +-inf, NaN and an out-of-domain (or huge) argument at the first index, in the final grid-stride pass and at the
    last index (the scalar tail): NaN-ness, infinities and the signs of zeros are NumPy's"""
    x = mc.special_input(op, p)
    n = x.size
    buf, out = guarded(ex, n)
    ex.grid_map(out, ex.from_host(x), op, p)
    got = payload(ex, buf, n, nan_ok=True)
    ref = mc.numpy_map(op, x, p)
    k = len(mc.special_values(op, p))
    for at in mc.special_positions():
        print(op, p, at, got[at:at + k], ref[at:at + k])
    _same_specials(got, ref)
    planted = np.zeros(n, bool)
    for at in mc.special_positions():
        planted[at:at + k] = True
    assert np.isnan(got[planted]).any() and not np.isnan(got[~planted]).any()


# ---- aliasing and alignment -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op,p", [("sqrt", 0.0), ("tanh", 0.0), ("pow", 3)])
def test_map_in_place(ex, op, p):
    n = 100003
    x = mc.map_input(op, n, "signed" if op == "pow" else "positive", p)
    buf, out = guarded(ex, n)
    ex.upload(out, x)
    ex.grid_map(out, out, op, p)
    check(op, p, x, payload(ex, buf, n), tag=pow_tag(p, "signed") if op == "pow" else None)


@pytest.mark.parametrize("n", [255, 100003])
@pytest.mark.parametrize("off_in,off_out", [(1, 1), (1, 0), (0, 1)])
@pytest.mark.parametrize("op", ["recip", "exp"])
def test_map_of_views_one_double_into_their_buffers(ex, op, n, off_in, off_out):
    """a component slice of an odd-sized array is 8 bytes off a 16-byte boundary: the scalar path"""
    x = mc.map_input(op, n)
    src = ex.from_host(np.concatenate([np.full(off_in, np.nan), x]))
    a = src[off_in:]
    buf, out = guarded(ex, n, off_out)
    assert a.data_ptr() % 16 == 8 * off_in and out.data_ptr() % 16 == 8 * off_out
    ex.grid_map(out, a, op)
    check(op, 0.0, x, payload(ex, buf, n, off_out))


# ---- broadcast --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,present,ncomp", mc.BROADCAST_CASES)
def test_broadcast(ex, shape, present, ncomp):
    a, ref = mc.broadcast_input(shape, present, ncomp)
    n = ref.size
    before = launches()
    buf, out = guarded(ex, n)
    ex.grid_broadcast(out, ex.from_host(a), ncomp, shape, present)
    assert same_bits(payload(ex, buf, n), ref.reshape(-1))
    assert launches() == before + 1
    # ... and into a buffer 8 bytes off a 16-byte boundary
    buf, out = guarded(ex, n, 1)
    ex.grid_broadcast(out, ex.from_host(a), ncomp, shape, present)
    assert same_bits(payload(ex, buf, n, 1), ref.reshape(-1))


# ---- error handling ---------------------------------------------------------------------------------------------------
def test_unknown_op_and_empty_array_launch_nothing(ex):
    from dedalus_amd import libhip
    from dedalus_amd.device import ptr
    lib = libhip.load()
    n = 1000
    buf, out = guarded(ex, n)
    x = ex.from_host(np.ones(n))
    before = launches()
    for bad in (-1, len(mc.OPS), 99):
        assert lib.ddh_grid_map(ptr(out), ptr(x), n, bad, 0.0, ex.dev.stream) != 0
        assert b"ddh_grid_map" in lib.ddh_last_error() and b"op" in lib.ddh_last_error()
    with pytest.raises(NotImplementedError):
        ex.grid_map(out, x, "erf")
    for empty in (0, -5):
        assert lib.ddh_grid_map(ptr(out), ptr(x), empty, 0, 0.0, ex.dev.stream) == 0
    shape, present = (C.c_long * 3)(4, 0, 8), (C.c_int * 3)(1, 1, 1)
    assert lib.ddh_grid_broadcast(ptr(out), ptr(x), 1, shape, present, ex.dev.stream) == 0
    assert lib.ddh_grid_broadcast(ptr(out), ptr(x), 0, shape, present, ex.dev.stream) != 0
    ex.sync()
    assert launches() == before
    assert np.isnan(ex.download(buf)).all()                               # nothing was written
    assert ex.MAP_OPS == {name: i for i, name in enumerate(mc.OPS)}
