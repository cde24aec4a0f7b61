"""The unchecked libm forms of nmp_libm.hpp (expf_u_, logf_u_, powf_u_, the batched, pair and constant-base forms) against the checked
ones, bit for bit (CPU, host compilation of the device source, in the style of tests/test_libm.py's sweeps).

An unchecked form runs the general path only and ORs into `suspect` the predicate its checked form branches on.  The property the
optimistic regions of the land kernel rest on: wherever `suspect` stays 0, the bits are the checked form's (NaN = NaN) -- and, for the
scalar forms, `suspect` is raised exactly where the checked form's test is true.  powf is also compared with the live libm there.

The bound is zero failures: with the test false both forms are the same IEEE operations on the same values.  Every sweep is exhaustive:
all 2^32 arguments of expf and logf, all 2^32 exponents of the constant-base form, all 2^32 bases for every exponent the kernels use
(about 50 s per pair of exponents on 8 cores).  NMP_LIBM_STRIDE=n walks every n-th pattern instead, for a quick look while developing."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host_emul", "libm_unchecked_check.hip")
LIB = os.path.join(HERE, "host_emul", "liblibm_unchecked_check.so")
STRIDE = int(os.environ.get("NMP_LIBM_STRIDE", "1"))
THREADS = max(1, min(16, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)))


def build():
    csrc = os.path.join(ROOT, "noahmp_amd", "csrc")
    deps = [SRC] + [os.path.join(csrc, f) for f in ("nmp_libm.hpp", "nmp_libm_tables.inc", "nmp_dev_common.hpp")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off",
                               "-mfma", "-Wno-unused-value", "-I" + csrc, "-I" + os.path.join(ROOT, "include"), SRC, "-o", LIB, "-lpthread"])


@pytest.fixture(scope="module")
def lib():
    build()
    try:
        import torch  # noqa: F401  (see noahmp_amd/abi.py::load_library: map torch's HIP runtime first)
    except ImportError:
        pass
    lib = C.CDLL(LIB)
    lib.libm_unchecked_sweep.restype = C.c_long
    lib.libm_unchecked_sweep.argtypes = [C.c_int, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]
    lib.libm_unchecked_pairs.restype = C.c_long
    lib.libm_unchecked_pairs.argtypes = [C.POINTER(C.c_uint32), C.c_int, C.POINTER(C.c_uint32), C.c_int, C.POINTER(C.c_uint32)]
    lib.libm_unchecked_log2.restype = C.c_double
    lib.libm_unchecked_log2.argtypes = [C.c_uint32]
    return lib


def _bits(x):
    return struct.unpack("<I", struct.pack("<f", np.float32(x)))[0]


def _bexp_spread():
    """BEXP of both tables of SOILPARM.TBL (STAS, STAS-RUC): the smallest and the largest of each"""
    out, cur = [], None
    for ln in open(os.path.join(HERE, "golden", "tables", "SOILPARM.TBL")):
        if ln.startswith("STAS"):
            cur = []
            out.append(cur)
        elif cur is not None and ln[:1].isdigit() and ln.count(",") > 5:
            b = float(ln.split(",")[1])
            if b > 0:
                cur.append(b)
    assert len(out) == 2 and all(len(t) >= 12 for t in out)
    return sorted({np.float32(v) for t in out for v in (min(t), max(t))})


def _kernel_exponents():
    """(name, y, y2): every exponent the kernels raise a variable base to, two per sweep (each base goes to both, and through the pair
    form with both: WDFCND's BEXP+2 with 2 BEXP+3)"""
    f = np.float32
    ex = [("0.25,0.5", f(0.25), f(0.5)), ("-0.25,2/3", f(-0.25), f(2.0) / f(3.0)), ("0.667,4", f(0.667), f(4.0))]
    for b in _bexp_spread():
        ex.append(("bexp%.2f:B+2,2B+3" % b, b + f(2.0), f(2.0) * b + f(3.0)))
        ex.append(("bexp%.2f:-B,-1/B" % b, -b, f(-1.0) / b))
    return ex


EXPONENTS = _kernel_exponents()


@pytest.mark.parametrize("what", [0, 1, 3], ids=["expf", "logf", "constbase_pow"])
def test_unchecked_equals_checked_where_not_suspect(lib, what):
    fb = C.c_uint32(0)
    n = lib.libm_unchecked_sweep(what, STRIDE, THREADS, 0, 0, C.byref(fb))
    assert n == 0, "%d failures, first at bits 0x%08x" % (n, fb.value)


@pytest.mark.parametrize("name,y,y2", EXPONENTS, ids=[e[0] for e in EXPONENTS])
def test_unchecked_powf_all_bases(lib, name, y, y2):
    """powf_u_, powfN_u_<2>, powfN_u_<4>, powf_pairN_u_<4>: every base of the 2^32 space to two exponents of the kernels"""
    fb = C.c_uint32(0)
    n = lib.libm_unchecked_sweep(2, STRIDE, THREADS, _bits(y), _bits(y2), C.byref(fb))
    assert n == 0, "%d failures, first at base bits 0x%08x (y = %r, y2 = %r)" % (n, fb.value, y, y2)


# +-0, subnormals, the smallest normals, +-1, +-inf, quiet and signalling NaNs of both signs, integers (odd, even), halves, large and tiny
SPECIAL = [0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007fffff, 0x807fffff, 0x00800000, 0x80800000, 0x3f800000, 0xbf800000,
           0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x7fa00000, 0xffa00000, 0x7f800001, 0xff800001, 0x7f7fffff, 0xff7fffff,
           0x40000000, 0xc0000000, 0x40400000, 0xc0400000, 0x40a00000, 0xc0a00000, 0x3f000000, 0xbf000000, 0x3fc00000, 0xbfc00000,
           0x3f2ac083, 0x4b800000, 0xcb800000, 0x4b800001, 0xcb800001, 0x4b000001, 0x7e967699, 0x0da24260, 0x42b00000, 0xc2b00000,
           0x42b17218, 0xc2cff1b5, 0x42aeac50, 0xc2aeac50]


def test_unchecked_structured_special_set(lib):
    """zeros, subnormals, infinities, quiet / signalling NaNs, negative bases with odd / even / non-integer exponents, and exponents that put
    |y log2 x| on both sides of 126 and 150 for a set of bases, through every form"""
    xs = list(SPECIAL) + [_bits(v) for v in (2.0, 0.5, 1.5, 10.0, 1e-3, 0.01, 0.3, 0.999, 1.001, -2.0, -0.5, 3e38, 2e-38)]
    ys = list(SPECIAL) + [_bits(e[1]) for e in EXPONENTS]
    for xb in [_bits(v) for v in (2.0, 0.5, 1.5, 10.0, 1e-3, 0.01, 0.3, 0.999, 1.001)]:
        l2 = abs(lib.libm_unchecked_log2(xb))
        for lim in (125.0, 126.0, 127.0, 128.0, 149.0, 150.0, 151.0):
            b = _bits(lim / l2)
            if b >= 0x7f800000:
                continue
            for d in range(-2, 3):
                ys += [b + d, (b + d) | 0x80000000]
    xa, ya = (C.c_uint32 * len(xs))(*xs), (C.c_uint32 * len(ys))(*ys)
    fb = (C.c_uint32 * 2)(0, 0)
    n = lib.libm_unchecked_pairs(xa, len(xs), ya, len(ys), fb)
    assert n == 0, "%d failing combinations, first x bits 0x%08x with y bits / form 0x%08x" % (n, fb[0], fb[1])
