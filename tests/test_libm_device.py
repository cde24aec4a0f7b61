"""The libm forms of nmp_libm.hpp / nmp_dev_common.hpp run as DEVICE code (tests/host_emul/libm_device_check.hip), compiled with the
library's own flags (noahmp_amd.build.FLAGS): the code objects under test get the optimisation level and the -mllvm options of the ones
that ship, the tables staged in LDS, the spelled-out exp2 table add, float64 v_fma and the device's own conversions.

1a (test_device_unchecked_*): the properties of tests/test_libm_unchecked.py, over all 2^32 patterns on the device -- wherever an
unchecked form leaves `suspect` 0 its bits are the checked form's (NaN = NaN), `suspect` of a scalar form is raised exactly where the
checked form's own predicate is true, and a batch that holds a suspect element raises it.  expf / logf: the scalar form and every
position of a batch of four; the constant-base form: all 2^32 exponents at all 8 positions; the powf family: all 2^32 bases, four
consecutive ones per thread, for every exponent pair of test_libm_unchecked.EXPONENTS; Libm<false>'s pow_quarter2 / pow_half /
pow_neg_quarter against Libm<true>'s over all 2^32 bases.  The bound is zero failures: with the predicate false both sides are the
same IEEE operations.  Both sides are called through functions that are not inlined, or the comparison would fold.

1b (test_device_*_match_libm): every form, checked and (where `suspect` stays 0) unchecked, against the host's ::powf / ::expf /
::logf -- the structured set of test_libm_unchecked.py as a full cross product at every batch position, every exponent of the kernels
with 2^22 bases spread over all 2^32 patterns (stride 1024, another start per exponent: negative, subnormal and non-finite bases
included), and the two rare sites of tests/test_libm_rare_sites.py.  Zero mismatches; ::expf is taken as the pinned build at the two
arguments where glibc's builds differ (tests/test_libm.py), so that bound is zero on any host.  test_staged_tables_* reads back the
LDS copies libm_stage_tables() makes and compares the 96 words with the committed constants.

NMP_LIBM_STRIDE=n walks every n-th pattern (every n-th block of four bases) of the exhaustive sweeps for a quick look; default 1.

Times: NOT MEASURED YET -- no MI355X could be had while this module was written, so no case of it has run on a device.  Expected from
the instruction counts (about 2.5 k static instructions per thread for four bases through every form, 2^30 threads): well under a few
seconds per parametrised case.  Whoever runs it first writes the times here, and splits the base range of any case that takes more than
about 10 s over more cases (the `lo` / `count` arguments of libm_dev_sweep) instead of thinning it."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from test_libm import EXPF_DISCRIMINATING
from test_libm_rare_sites import SPECIAL as RARE_SPECIAL
from test_libm_unchecked import EXPONENTS, SPECIAL

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host_emul", "libm_device_check.hip")
LIB = os.path.join(HERE, "host_emul", "liblibm_device_check.so")
STRIDE = int(os.environ.get("NMP_LIBM_STRIDE", "1"))
THREADS = max(1, min(16, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)))
POW_FORMS = ["powf_", "powfN_<2>", "powfN_<4>", "powf_pairN_<4>", "powf_u_", "powfN_u_<2>", "powfN_u_<4>", "powf_pairN_u_<4>"]
EXPLOG_FORMS = ["expf_", "expfN_<4>", "logf_", "logfN_<4>", "expf_u_", "expfN_u_<4>", "logf_u_", "logfN_u_<4>"]
RARE_FORMS = ["nmp_powf_constbaseN<8>", "powf_constbaseN_u_<8>", "nmp_powf_zero_base"]


def build_command():
    from noahmp_amd.build import CSRC, FLAGS
    return [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + FLAGS + ["-I" + CSRC, "-shared", SRC, "-o", LIB, "-lpthread"]


def build():
    """The checker with the library's flags (noahmp_amd.build.FLAGS + the csrc include path + -shared)."""
    from noahmp_amd.build import CSRC
    deps = [SRC] + [os.path.join(CSRC, f) for f in ("nmp_libm.hpp", "nmp_libm_tables.inc", "nmp_dev_common.hpp")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(build_command())


@pytest.fixture(scope="module")
def lib():
    build()
    try:
        import torch  # noqa: F401  (see noahmp_amd/abi.py::load_library: map torch's HIP runtime first)
    except ImportError:
        pass
    lib = C.CDLL(LIB)
    u32p, lp = C.POINTER(C.c_uint32), C.POINTER(C.c_long)
    lib.libm_dev_sweep.restype = C.c_long
    lib.libm_dev_sweep.argtypes = [C.c_int, C.c_uint32, C.c_ulonglong, C.c_uint32, C.c_uint32, C.c_uint32, u32p]
    lib.libm_dev_pow_vs_host.restype = C.c_long
    lib.libm_dev_pow_vs_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_long, C.c_int, C.c_int, lp, u32p]
    lib.libm_dev_explog_vs_host.restype = C.c_long
    lib.libm_dev_explog_vs_host.argtypes = [C.c_void_p, C.c_long, C.c_int, C.c_int, u32p, C.c_int, lp, u32p]
    lib.libm_dev_rare_vs_host.restype = C.c_long
    lib.libm_dev_rare_vs_host.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_int, lp, u32p]
    lib.libm_dev_tables.restype = C.c_long
    lib.libm_dev_tables.argtypes = [C.c_void_p, C.c_void_p]
    lib.libm_dev_log2.restype = C.c_double
    lib.libm_dev_log2.argtypes = [C.c_uint32]
    lib.libm_dev_log2base.restype = C.c_double
    lib.libm_dev_log2base.argtypes = [C.c_int]
    return lib


def _bits(x):
    return struct.unpack("<I", struct.pack("<f", np.float32(x)))[0]


def test_checker_cross_compiles_with_the_library_flags():
    """CPU: the checker builds for gfx950 from noahmp_amd.build.FLAGS -- the optimisation level and every -mllvm option of the library"""
    from noahmp_amd.build import FLAGS
    cmd = build_command()
    assert all(f in cmd for f in FLAGS) and "--offload-arch=gfx950" in cmd and "-O3" in cmd and cmd.count("-mllvm") == FLAGS.count("-mllvm") >= 2
    assert not any(f in cmd for f in ("-O2", "-O0", "-mfma"))
    build()
    assert os.path.getmtime(LIB) >= os.path.getmtime(SRC)
    code = open(LIB, "rb").read()
    assert b"gfx950" in code and all(k in code for k in (b"sweep_kernel", b"pow_vs_host_kernel", b"explog_vs_host_kernel", b"rare_vs_host_kernel", b"tables_kernel"))


# ---- 1a
def _sweep(lib, what, count, y=0, y2=0):
    fb = C.c_uint32(0)
    n = lib.libm_dev_sweep(what, 0, count // STRIDE, STRIDE, y, y2, C.byref(fb))
    assert n >= 0, "HIP error"
    return n, fb.value


@pytest.mark.gpu
@pytest.mark.parametrize("what,name", [(0, "expf"), (1, "logf"), (3, "constbase_pow"), (4, "region_wrappers")],
                         ids=["expf", "logf", "constbase_pow", "region_wrappers"])
def test_device_unchecked_equals_checked_where_not_suspect(lib, what, name):
    n, fb = _sweep(lib, what, 1 << 32)
    assert n == 0, "%s on the GPU: %d failing patterns, the smallest 0x%08x" % (name, n, fb)


@pytest.mark.gpu
@pytest.mark.parametrize("name,y,y2", EXPONENTS, ids=[e[0] for e in EXPONENTS])
def test_device_unchecked_powf_all_bases(lib, name, y, y2):
    """powf_u_, powfN_u_<2>, powfN_u_<4>, powf_pairN_u_<4>: every base of the 2^32 space to two exponents of the kernels"""
    n, fb = _sweep(lib, 2, 1 << 30, _bits(y), _bits(y2))
    assert n == 0, "powf family on the GPU: %d failing blocks of four bases, the smallest at base bits 0x%08x (y = %r, y2 = %r)" % (n, fb, y, y2)


# ---- 1b
def _u32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.uint64).astype(np.uint32))


def _report(forms, counts, first, describe):
    return "; ".join("%s: %d mismatches, first %s" % (forms[i], counts[i], describe(first[i])) for i in range(len(forms)) if counts[i])


def _pow_vs_host(lib, xs, ys, y2s, allpos):
    xs, ys, y2s = _u32(xs), _u32(ys), _u32(y2s)
    counts, first = (C.c_long * len(POW_FORMS))(), (C.c_uint32 * len(POW_FORMS))()
    bad = lib.libm_dev_pow_vs_host(xs.ctypes.data, ys.ctypes.data, y2s.ctypes.data, len(xs), allpos, THREADS, counts, first)
    assert bad >= 0, "HIP error"
    assert bad == 0, _report(POW_FORMS, counts, first, lambda i: "x bits 0x%08x, y bits 0x%08x / 0x%08x" % (xs[i], ys[i], y2s[i]))


def _explog_vs_host(lib, xs, allpos):
    xs = _u32(xs)
    pin = (C.c_uint32 * (2 * len(EXPF_DISCRIMINATING)))(*[v for x, fma, _ in EXPF_DISCRIMINATING for v in (x, fma)])
    counts, first = (C.c_long * len(EXPLOG_FORMS))(), (C.c_uint32 * len(EXPLOG_FORMS))()
    bad = lib.libm_dev_explog_vs_host(xs.ctypes.data, len(xs), allpos, THREADS, pin, len(EXPF_DISCRIMINATING), counts, first)
    assert bad >= 0, "HIP error"
    assert bad == 0, _report(EXPLOG_FORMS, counts, first, lambda i: "x bits 0x%08x" % xs[i])


def _structured(lib):
    """test_libm_unchecked.py::test_unchecked_structured_special_set's bases and exponents"""
    plain = [_bits(v) for v in (2.0, 0.5, 1.5, 10.0, 1e-3, 0.01, 0.3, 0.999, 1.001)]
    xs = list(SPECIAL) + plain + [_bits(v) for v in (-2.0, -0.5, 3e38, 2e-38)]
    ys = list(SPECIAL) + [_bits(e[1]) for e in EXPONENTS] + [_bits(e[2]) for e in EXPONENTS]
    for xb in plain:
        l2 = abs(lib.libm_dev_log2(xb))
        for lim in (125.0, 126.0, 127.0, 128.0, 149.0, 150.0, 151.0):
            b = _bits(lim / l2)
            if b >= 0x7f800000:
                continue
            for d in range(-2, 3):
                ys += [b + d, (b + d) | 0x80000000]
    return xs, ys


@pytest.mark.gpu
def test_device_structured_set_matches_libm(lib):
    """zeros, subnormals, infinities, quiet / signalling NaNs, negative bases with odd / even / non-integer exponents, and exponents that
    put |y log2 x| on both sides of 126 and 150: every x with every y through every powf form at every batch position, every pattern
    through the expf / logf forms"""
    xs, ys = _structured(lib)
    X, Y = np.meshgrid(np.array(xs, dtype=np.uint64), np.array(ys, dtype=np.uint64), indexing="ij")
    Y2 = np.roll(Y, -1, axis=1)                            # the pair form's second exponent: the next one of the list
    _pow_vs_host(lib, X.ravel(), Y.ravel(), Y2.ravel(), 1)
    _explog_vs_host(lib, sorted(set(xs + ys)), 1)


FIXED_Y = [("2,3", 2.0, 3.0), ("4,0.5", 4.0, 0.5), ("0.25,-0.25", 0.25, -0.25), ("1.7,2/3", 1.7, np.float32(2.0) / np.float32(3.0))]   # libm_check.hip's fixed_y
KERNEL_PAIRS = list(EXPONENTS) + [(n, np.float32(a), np.float32(b)) for n, a, b in FIXED_Y]


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(len(KERNEL_PAIRS)), ids=[e[0] for e in KERNEL_PAIRS])
def test_device_kernel_exponents_match_libm(lib, case):
    """the exponents the kernels raise a variable base to, each with 2^22 bases spread over all 2^32 patterns"""
    _, y, y2 = KERNEL_PAIRS[case]
    start = (case * 89 + 7) % 1024
    xs = (start + 1024 * np.arange(1 << 22, dtype=np.uint64))
    _pow_vs_host(lib, xs, np.full(xs.shape, _bits(y), dtype=np.uint64), np.full(xs.shape, _bits(y2), dtype=np.uint64), 0)


@pytest.mark.gpu
def test_device_expf_logf_forms_match_libm(lib):
    """expf_ / logf_ / expfN_<4> / logfN_<4> and their unchecked forms on every 1024th pattern"""
    _explog_vs_host(lib, 531 + 1024 * np.arange(1 << 22, dtype=np.uint64), 0)


@pytest.mark.gpu
def test_device_rare_sites_match_libm(lib):
    """TDFCND's constant-base batch with y = +-0 among it and CANWATER's zero base (tests/test_libm_rare_sites.py's list at every batch
    position, and every 1024th pattern)"""
    extra = list(RARE_SPECIAL)
    for which in (0, 1):
        l2 = abs(lib.libm_dev_log2base(which))
        for lim in (126.0, 127.0, 128.0, 149.0, 150.0, 151.0):
            b = _bits(lim / l2)
            for d in range(-3, 4):
                extra += [b + d, (b + d) | 0x80000000]
    strided = 77 + 1024 * np.arange(1 << 22, dtype=np.uint64)
    ys = _u32(np.concatenate([np.repeat(np.array(extra, dtype=np.uint64), 8), strided]))
    pos = np.ascontiguousarray(np.concatenate([np.tile(np.arange(8), len(extra)), np.arange(len(strided)) % 8]).astype(np.uint8))
    counts, first = (C.c_long * len(RARE_FORMS))(), (C.c_uint32 * len(RARE_FORMS))()
    bad = lib.libm_dev_rare_vs_host(ys.ctypes.data, pos.ctypes.data, len(ys), THREADS, counts, first)
    assert bad >= 0, "HIP error"
    assert bad == 0, _report(RARE_FORMS, counts, first, lambda i: "bits 0x%08x at position %d" % (ys[i], pos[i]))


@pytest.mark.gpu
def test_staged_tables_are_the_committed_constants(lib):
    """what libm_stage_tables() leaves in LDS (the tables every device routine reads) against nmp_libm_tables.inc, word for word"""
    staged, committed = np.zeros(96, dtype=np.uint64), np.zeros(96, dtype=np.uint64)
    assert lib.libm_dev_tables(staged.ctypes.data, committed.ctypes.data) == 0, "HIP error"
    assert committed[:32].all() and committed[32:].any()
    bad = np.nonzero(staged != committed)[0]
    assert bad.size == 0, "table word %d (%s[%d]): staged 0x%016x, committed 0x%016x" % (
        bad[0], ("kExp2fTab", "kLogfTab", "kPowfLog2Tab")[bad[0] // 32], bad[0] % 32, staged[bad[0]], committed[bad[0]])
