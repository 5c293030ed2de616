"""CPU: the C-ABI shared library builds, loads, and exports every symbol include/dedalus_hip.h declares."""
import os
import re

from dedalus_amd import build, libhip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_builds_and_exports_header_symbols():
    build.build_library()
    lib = libhip.load()
    header = open(os.path.join(ROOT, "include", "dedalus_hip.h")).read()
    declared = set(re.findall(r"\b(ddh_[a-z0-9_]+)\s*\(", header))
    declared -= {"ddh_handle"}
    assert len(declared) > 20
    for name in sorted(declared):
        assert hasattr(lib, name), "symbol %s declared in the header but not exported" % name
    bound = set(libhip.SIGNATURES) | {"ddh_last_error"}
    assert declared == bound, (declared ^ bound)


def test_error_reporting_without_gpu():
    lib = libhip.load()
    # invalid handle -> negative status and a message; no device work involved
    assert lib.ddh_destroy(123456789) != 0
    assert b"invalid handle" in lib.ddh_last_error()


def test_wave_size_table_is_the_listed_sizes():
    """ddh_fft_wave_size (generated from the X-macros the dispatch is generated from) answers "covered" exactly for the
    sizes the GPU tests list, kind by kind, over every (N, M) in 16..1024; no GPU involved."""
    import ctypes as C

    from test_gpu_wave_transforms import WAVE_CHEB_SIZES, WAVE_RFFT_SIZES

    assert len(set(WAVE_CHEB_SIZES)) == 8 and len(set(WAVE_RFFT_SIZES)) == 4
    lib = libhip.load()
    covered = C.c_int(-1)
    got = {0: set(), 1: set()}
    for kind in (0, 1):
        for N in range(16, 1025):
            for M in range(16, 1025):
                assert lib.ddh_fft_wave_size(kind, N, M, C.byref(covered)) == 0
                assert covered.value in (0, 1)
                if covered.value:
                    got[kind].add((N, M))
    assert got[0] == set(WAVE_RFFT_SIZES)
    assert got[1] == set(WAVE_CHEB_SIZES)
    # a pair of one kind is not reported for the other kind unless both lists hold it
    both = set(WAVE_RFFT_SIZES) & set(WAVE_CHEB_SIZES)
    assert (got[0] & got[1]) == both
    # other kinds (complex FFT) and a null pointer are errors, not "not covered"
    assert lib.ddh_fft_wave_size(2, 192, 128, C.byref(covered)) != 0
    assert lib.ddh_fft_wave_size(1, 192, 128, None) != 0
