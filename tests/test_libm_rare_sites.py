"""The two libm call sites whose "rare" arguments are the common case of a run, against the live libm, bit for bit (CPU, host
compilation of the device source, in the style of tests/test_libm.py's sweeps).

TDFCND raises TKICE and 0.57 to SMCMAX - XU and XU, which are exactly zero in every soil layer without ice or without liquid water;
CANWATER raises FWET to 0.667, and FWET is exactly zero for a canopy that holds no water.  Both used to send their wave through
powf's cold blocks in nearly every step.  powf_constbaseN_ now leaves y = +-0 to its general path, and nmp_powf_zero_base takes
0 ** y by a select: the results must be libm's for EVERY argument, the rare ones (subnormal, inf, NaN, negative, out of range)
included -- those still take the cold blocks.

The bound is zero mismatches: both sides are the same IEEE operations.  NMP_LIBM_STRIDE=1 makes the sweeps exhaustive."""
import ctypes as C
import os
import struct
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host_emul", "rare_sites_check.hip")
LIB = os.path.join(HERE, "host_emul", "librare_sites_check.so")


def build():
    csrc = os.path.join(ROOT, "noahmp_amd", "csrc")
    deps = [SRC] + [os.path.join(csrc, f) for f in ("nmp_libm.hpp", "nmp_libm_tables.inc", "nmp_dev_common.hpp")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off",
                               "-mfma", "-Wno-unused-value", "-I" + csrc, "-I" + os.path.join(ROOT, "include"), SRC, "-o", LIB, "-lpthread"])


def _lib():
    build()
    try:
        import torch  # noqa: F401  (see noahmp_amd/abi.py::load_library: map torch's HIP runtime first)
    except ImportError:
        pass
    lib = C.CDLL(LIB)
    lib.rare_sites_check.restype = C.c_long
    lib.rare_sites_check.argtypes = [C.c_int, C.c_uint32, C.c_int, C.POINTER(C.c_uint32), C.c_int, C.POINTER(C.c_uint32)]
    lib.rare_sites_log2base.restype = C.c_double
    lib.rare_sites_log2base.argtypes = [C.c_int]
    return lib


def _bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


# +-0, subnormals, the smallest normals, +-1, +-inf, quiet and signalling NaNs of both signs, integers (odd, even) and halves
SPECIAL = [0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007fffff, 0x807fffff, 0x00800000, 0x80800000, 0x3f800000, 0xbf800000,
           0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x7fa00000, 0xffa00000, 0x7f800001, 0x7f7fffff, 0xff7fffff,
           0x40000000, 0xc0000000, 0x40400000, 0xc0400000, 0x3f000000, 0xbf000000, 0x3f2ac083]


def _range_end_exponents(lib):
    """exponents that put |y log2 BASE| just below and just above 126 and 150 for both bases, with both signs"""
    out = []
    for which in (0, 1):
        l2 = abs(lib.rare_sites_log2base(which))
        for lim in (126.0, 127.0, 128.0, 149.0, 150.0, 151.0):
            b = _bits(lim / l2)
            for d in range(-3, 4):
                out += [b + d, (b + d) | 0x80000000]
    return out


@pytest.mark.parametrize("what", [0, 1], ids=["tdfcnd_constbase_pow", "canwater_fwet_pow"])
def test_rare_site_forms_match_libm(what):
    lib = _lib()
    extra = SPECIAL + _range_end_exponents(lib)
    arr = (C.c_uint32 * len(extra))(*extra)
    fb = C.c_uint32(0)
    stride = int(os.environ.get("NMP_LIBM_STRIDE", "61"))
    n = lib.rare_sites_check(what, stride, 8, arr, len(extra), C.byref(fb))
    assert n == 0, "%d mismatches, first at bits 0x%08x" % (n, fb.value)
