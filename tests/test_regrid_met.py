"""Elevation-adjusted met group of the forcing regrid (noahmp_hip_forcing_regrid_met; nmp_dev_regrid.hpp::regrid_met).

Air temperature, pressure, specific humidity and downward longwave of a coarse record are regridded bilinearly and moved from the source's
terrain height to the model's: lapse-rate temperature, hypsometric pressure, humidity at constant relative humidity, longwave by the
emissivity and T^4 ratio (Cosgrove et al. 2003).  The contract is the text in include/noahmp_hip.h.  np_met restates it in numpy float32,
one rounded operation per line, with glibc's own expf / powf called per element through ctypes; everything is compared with it bit for
bit (test_regrid.assert_same: equal bits, or both NaN): the per-column function compiled for the host, the kernel at every shape,
and a two-step engine run fed through ForcingRegrid.set_elevation against the same run fed with fine records made by the restatement."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from noahmp_amd import abi
import test_regrid as tr
from test_regrid import F, BIL, NEAR, SOURCES, assert_same, nasty, np_plan, np_regrid, value_cases

D = np.float64
ROOT = tr.ROOT
CSRC = tr.CSRC
SRC = os.path.join(ROOT, "tests", "host_emul", "regrid_met_check.hip")
LIB = os.path.join(ROOT, "tests", "host_emul", "libregrid_met_check.so")
LAPSE = F(-0.0065)
OPERANDS = ("t", "p", "q", "lw", "dz")
SETS = ("physical", "nasty") + tuple("nasty_" + o for o in OPERANDS)


# ---------------------------------------------------------------------------------------------------------------- the restatement
_libm = C.CDLL("libm.so.6")
_libm.expf.restype = C.c_float
_libm.expf.argtypes = [C.c_float]
_libm.powf.restype = C.c_float
_libm.powf.argtypes = [C.c_float, C.c_float]


def expf(x):
    return np.array([_libm.expf(float(v)) for v in x], F)


def powf(x, y):
    return np.array([_libm.powf(float(a), float(b)) for a, b in zip(x, y)], F)


def np_met(tc, pc, qc, lc, d, lapse=LAPSE):
    """The chain of the header text over arrays of regridded values.  lc None: no longwave.  Returns (tf, pf, qf, lf or None)."""
    tc, pc, qc, d = (np.asarray(x, F) for x in (tc, pc, qc, d))
    lapse = F(lapse)
    with np.errstate(all="ignore"):
        prod = lapse * d
        tf = tc + prod
        tsum = tc + tf
        tbar = tsum * F(0.5)
        gd = F(9.81) * d
        rt = F(287.0) * tbar
        hx = gd / rt
        pf = pc / expf(hx)

        def esat(t):
            a = t - F(273.15)
            num = F(17.67) * a
            den = t - F(29.65)
            return F(611.2) * expf(num / den)

        def qsat(es, p):
            num = F(0.622) * es
            part = F(0.378) * es
            den = p - part
            return num / den

        def emis(q, p, t):
            qp = q * p
            e = qp / F(0.622)
            mb = e / F(100.0)
            ex = t / F(2016.0)
            en = expf(-powf(mb, ex))
            one = F(1.0) - en
            return F(1.08) * one
        rh = qc / qsat(esat(tc), pc)
        qf = rh * qsat(esat(tf), pf)
        same = d == 0                                          # either sign; NaN is not
        out = [np.where(same, tc, tf), np.where(same, pc, pf), np.where(same, qc, qf), None]
        if lc is not None:
            lc = np.asarray(lc, F)
            er = emis(qf, pf, tf) / emis(qc, pc, tc)
            le = lc * er
            tf2, tc2 = tf * tf, tc * tc
            tf4, tc4 = tf2 * tf2, tc2 * tc2
            tr_ = tf4 / tc4
            out[3] = np.where(same, lc, le * tr_)
    return out


def filled(plan, g):
    """Columns that BILINEAR fills: base out of range, or a corner of non-zero weight behind the plane."""
    nx, nxny, per = int(g.nx), int(g.nx) * int(g.ny), bool(g.periodic_x)
    b = plan[0].astype(np.int64)
    w = plan[2:].view(F)
    out = (b < 0) | (b >= nxny)
    c1 = np.where(per & (b % nx == nx - 1), b + 1 - nx, b + 1)
    for k, idx in ((1, c1), (2, b + nx), (3, c1 + nx)):
        out |= (w[k] != 0) & (idx >= nxny)
    return out


def corner_reads(plan, g):
    """How often each source cell is read by one bilinear plane: exactly the corners of non-zero weight of the columns not filled."""
    nx, nxny, per = int(g.nx), int(g.nx) * int(g.ny), bool(g.periodic_x)
    want = np.zeros(nxny, np.int32)
    fl = filled(plan, g)
    w = plan[2:].view(F)
    for c in np.flatnonzero(~fl):
        b = int(plan[0, c])
        c1 = b + 1 - nx if (per and b % nx == nx - 1) else b + 1
        for k, i in enumerate((b, c1, b + nx, c1 + nx)):
            if w[k, c] != 0:
                want[i] += 1
    return want


# ---------------------------------------------------------------------------------------------------------------- the inputs
def physical(r, n):
    """t, p, q, lw, dz over the ranges of a real record; some dz are exactly +0.0 and -0.0."""
    dz = r.uniform(-2500.0, 4000.0, n).astype(F)
    z = r.random(n)
    dz[z < 0.06] = F(0.0)
    dz[z < 0.03] = F(-0.0)
    return dict(t=r.uniform(220.0, 320.0, n).astype(F), p=r.uniform(4.5e4, 1.05e5, n).astype(F), q=r.uniform(1e-5, 2.5e-2, n).astype(F),
                lw=r.uniform(100.0, 500.0, n).astype(F), dz=dz)


@functools.lru_cache(maxsize=None)
def case(name, ncell):
    """One plan of value_cases with physical and nasty operands over it, and the bilinear values of every source plane (np_regrid, once)."""
    g = SOURCES[name]
    r = np.random.default_rng(7000 + ncell + len(name))
    plan, _ = value_cases(r, g, ncell)
    nxny = g.nx * g.ny
    phys = physical(r, nxny)
    phys["dz"] = physical(r, ncell)["dz"]
    nas = {o: nasty(r, ncell if o == "dz" else nxny) for o in OPERANDS}
    coarse = {("physical", o): np_regrid(plan, g, phys[o], BIL) for o in OPERANDS[:4]}
    coarse.update({("nasty", o): np_regrid(plan, g, nas[o], BIL) for o in OPERANDS[:4]})
    plan.setflags(write=False)
    return plan, phys, nas, coarse, filled(plan, g)


@functools.lru_cache(maxsize=None)
def reference(name, ncell, which, fill=-999.0):
    """(sources t, p, q, lw; dz; the four restated destination planes) of one input set."""
    plan, phys, nas, coarse, fl = case(name, ncell)
    pick = {o: ("nasty" if which in ("nasty", "nasty_" + o) else "physical") for o in OPERANDS}
    src = [(nas if pick[o] == "nasty" else phys)[o] for o in OPERANDS[:4]]
    dz = (nas if pick["dz"] == "nasty" else phys)["dz"]
    tc, pc, qc, lc = (coarse[(pick[o], o)] for o in OPERANDS[:4])
    want = np_met(tc, pc, qc, lc, dz)
    want = [np.where(fl, F(fill), x).astype(F) for x in want]
    for a in src + [dz] + want:
        a.setflags(write=False)
    return src, dz, want


# ---------------------------------------------------------------------------------------------------------------- CPU
def build():
    deps = [SRC, os.path.join(CSRC, "nmp_dev_regrid.hpp"), os.path.join(CSRC, "nmp_libm.hpp"), os.path.join(CSRC, "nmp_libm_tables.inc"),
            os.path.join(ROOT, "include", "noahmp_hip.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off",
                               "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), SRC, "-o", LIB])


def _host():
    build()
    try:
        import torch  # noqa: F401  (map torch's HIP runtime first, noahmp_amd/abi.py::load_library)
    except ImportError:
        pass
    lib = C.CDLL(LIB)
    P = C.POINTER(C.c_void_p)
    lib.regrid_met_values.argtypes = [C.c_void_p, C.c_long, C.POINTER(abi.RegridSource), P, P, C.c_void_p, C.c_float, C.c_float, P]
    lib.regrid_met_values.restype = None
    lib.regrid_met_chain.argtypes = [C.c_long] + [C.c_void_p] * 5 + [C.c_float] + [C.c_void_p] * 4
    lib.regrid_met_chain.restype = None
    return lib


def _ptrs(arrays):
    return (C.c_void_p * 4)(*[a.ctypes.data if a is not None else None for a in arrays])


def _host_chain(lib, x, lw=True):
    n = x["t"].size
    out = [np.full(n, 7.0, F) for _ in range(4)]
    lib.regrid_met_chain(n, x["t"].ctypes.data, x["p"].ctypes.data, x["q"].ctypes.data, x["lw"].ctypes.data if lw else None,
                         x["dz"].ctypes.data, float(LAPSE), *[o.ctypes.data for o in out])
    return out


@pytest.mark.parametrize("name", list(SOURCES))
def test_host_compilation_equals_np_met_and_reads_no_dropped_corner(name):
    """regrid_met and the corner functions compiled for the host against the restatement: every set, with and without longwave, at the
    shapes of the GPU test; each of the three or four sources is read exactly at the corners of non-zero weight."""
    lib = _host()
    g = SOURCES[name]
    for ncell in (256, 335, 1):
        plan = case(name, ncell)[0]
        reads_want = corner_reads(plan, g)
        for which in SETS:
            src, dz, want = reference(name, ncell, which)
            for lw in (True, False):
                got = [np.full(ncell, 7.0, F) for _ in range(4)]
                reads = [np.zeros(g.nx * g.ny, np.int32) for _ in range(4)]
                lib.regrid_met_values(plan.ctypes.data, ncell, C.byref(g), _ptrs(src[:3] + [src[3] if lw else None]), _ptrs(got), dz.ctypes.data,
                                      float(LAPSE), -999.0, _ptrs(reads))
                for f, o in enumerate(OPERANDS[:4]):
                    what = "%s n=%d set %s lw=%d plane %s" % (name, ncell, which, lw, o)
                    if f == 3 and not lw:
                        assert (got[3] == 7.0).all() and not reads[3].any(), what
                        continue
                    assert_same(got[f], want[f], what)
                    assert np.array_equal(reads[f], reads_want), what


def test_chain_properties():
    lib = _host()
    r = np.random.default_rng(11)
    x = physical(r, 20000)
    tf, pf, qf, lf = _host_chain(lib, x)
    z = x["dz"] == 0
    assert z.sum() > 500 and np.signbit(x["dz"][z]).any() and not np.signbit(x["dz"][z]).all()
    for got, o in zip((tf, pf, qf, lf), OPERANDS):                                  # dz == +-0: the coarse bits
        assert_same(got[z], x[o][z], "dz == 0, " + o)
    nz = ~z
    assert (np.isfinite(tf) & np.isfinite(pf) & np.isfinite(qf) & np.isfinite(lf)).all()
    assert np.array_equal(pf[nz] < x["p"][nz], x["dz"][nz] > 0) and np.array_equal(pf[nz] > x["p"][nz], x["dz"][nz] < 0)
    assert (qf > 0).all() and (lf > 0).all()
    # dst_t is what the existing adjust path makes of the same plan, source and dz
    g = SOURCES["plain"]
    plan = case("plain", 335)[0]
    src, dz, want = reference("plain", 335, "physical")
    old = np.zeros(335, F)
    tr._host().regrid_values(plan.ctypes.data, 335, C.byref(g), src[0].ctypes.data, old.ctypes.data, dz.ctypes.data, float(LAPSE), -999.0, BIL, None)
    got = [np.full(335, 7.0, F) for _ in range(4)]
    lib.regrid_met_values(plan.ctypes.data, 335, C.byref(g), _ptrs(src), _ptrs(got), dz.ctypes.data, float(LAPSE), -999.0, _ptrs([None] * 4))
    assert_same(got[0], old, "dst_t of the met group against the adjust path")
    assert_same(got[0], np_regrid(plan, g, src[0], BIL, dz, LAPSE, -999.0), "dst_t of the met group against np_regrid with adjust")
    # without longwave the other three planes are the same
    t3, p3, q3, l3 = _host_chain(lib, x, lw=False)
    for a, b, o in ((t3, tf, "t"), (p3, pf, "p"), (q3, qf, "q")):
        assert_same(a, b, "no longwave, " + o)
    assert (l3 == 7.0).all()


def test_chain_agrees_with_float64():
    """Every output against a float64 evaluation of the same formulas, relative 1e-5: five times the largest deviation seen on 200 000
    draws (2.04e-6 for q, 7.4e-7 for lw, 1.6e-7 for p), so other draws do not flake while a wrong constant (>= 1e-3) cannot pass."""
    lib = _host()
    r = np.random.default_rng(3)
    x = physical(r, 50000)
    nz = x["dz"] != 0
    x = {k: v[nz] for k, v in x.items()}
    got = _host_chain(lib, x)
    t, p, q, lw, d = (x[o].astype(D) for o in OPERANDS)
    tf = t + D(LAPSE) * d
    tbar = (t + tf) * 0.5
    pf = p / np.exp((D(F(9.81)) * d) / (D(F(287.0)) * tbar))
    esat = lambda t: D(F(611.2)) * np.exp(D(F(17.67)) * (t - D(F(273.15))) / (t - D(F(29.65))))
    qsat = lambda t, p: D(F(0.622)) * esat(t) / (p - D(F(0.378)) * esat(t))
    qf = q / qsat(t, p) * qsat(tf, pf)
    emis = lambda q, p, t: D(F(1.08)) * (1.0 - np.exp(-np.power(q * p / D(F(0.622)) / 100.0, t / 2016.0)))
    lf = lw * (emis(qf, pf, tf) / emis(q, p, t)) * (tf ** 4 / t ** 4)
    for g32, w64, o in zip(got, (tf, pf, qf, lf), OPERANDS):
        dev = np.abs(g32.astype(D) - w64) / np.abs(w64)
        print("float64 agreement %s: max relative deviation %.3g" % (o, dev.max()))
        assert dev.max() <= 1e-5, (o, dev.max())


def test_bindings_regenerate_identically_with_the_met_group():
    from tools import gen_abi
    for rel, text in (("include/noahmp_hip.h", gen_abi.c_header()), ("oracle/ref_harness_gen.f90", gen_abi.ref_harness()),
                      ("noahmp_amd/fortran/module_sf_noahmpdrv_hip.F90", gen_abi.fortran_shim()),
                      ("tests/fortran/shim_wrap_gen.f90", gen_abi.shim_wrap())):
        assert open(os.path.join(ROOT, rel)).read() == text, rel
    hdr = open(os.path.join(ROOT, "include", "noahmp_hip.h")).read()
    for word in ("typedef struct noahmp_regrid_met {", "} noahmp_regrid_met;", "noahmp_hip_forcing_regrid_met(",
                 "#define NOAHMP_HIP_ABI_VERSION 1\n", "#define NOAHMP_HIP_ABI_MINOR 3\n",
                 "pf   = pc / expf((9.81f*d) / (287.0f*tbar))", "esat(t)   = 611.2f * expf((17.67f*(t - 273.15f)) / (t - 29.65f))",
                 "emis(q,p,t) = 1.08f * (1.0f - expf(-powf(((q*p)/0.622f)/100.0f, t/2016.0f)))"):
        assert word in hdr, word
    assert "noahmp_regrid" not in gen_abi.ref_harness()
    f90 = open(os.path.join(ROOT, "noahmp_amd", "fortran", "module_sf_noahmpdrv_hip.F90")).read()
    assert "bind(C, name='noahmp_hip_forcing_regrid_met')" in f90 and "type, bind(C) :: noahmp_regrid_met" in f90
    assert "noahmp_hip_forcing_regrid_met" in abi.EXPORTED_SYMBOLS
    assert [n for n, _ in abi.RegridMet._fields_] == ["src_t", "src_p", "src_q", "src_lw", "dst_t", "dst_p", "dst_q", "dst_lw", "dz", "lapse", "fill"]


def test_ctypes_mirror_of_the_met_group_matches_the_compiled_header(tmp_path):
    names = [n for n, _ in abi.RegridMet._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "noahmp_hip.h"\nint main(){printf("%zu", sizeof(noahmp_regrid_met));' +
                   "".join('printf(" %%zu", offsetof(noahmp_regrid_met, %s));' % n for n in names) +
                   'printf(" %d", NOAHMP_HIP_ABI_MINOR); return 0;}')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    M = abi.RegridMet
    assert out == [C.sizeof(M)] + [getattr(M, n).offset for n in names] + [3]


def test_library_exports_the_met_regrid():
    if not os.path.exists(abi.LIB_PATH):
        from noahmp_amd import build as b
        b.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", abi.LIB_PATH]).decode()
    assert " T noahmp_hip_forcing_regrid_met" in out and " T noahmp_hip_forcing_regrid\n" in out


@pytest.mark.skipif(tr._flang() is None, reason="no flang")
def test_generated_fortran_met_type_and_interface_compile(tmp_path):
    """The regrid part of the generated module with the met group in it compiles, and a caller of the new interface type-checks."""
    from tools import gen_abi
    text = "\n".join(["module regrid_met_abi_check", "  use iso_c_binding", "  implicit none"] + gen_abi.regrid_f90_types() + ["  interface"] +
                     gen_abi.regrid_f90_interfaces() +
                     ["  end interface", "contains", "  function go(plan, ncell, planes) result(rc)",
                      "    type(c_ptr), value :: plan", "    integer(c_int64_t), value :: ncell",
                      "    type(c_ptr), intent(in) :: planes(11)", "    type(noahmp_regrid_source) :: g",
                      "    type(noahmp_regrid_met) :: m", "    type(noahmp_regrid_entry) :: e(1)", "    integer(c_int) :: rc",
                      "    g%nx = 464; g%ny = 224; g%lon0 = -124.9375d0; g%lat0 = 25.0625d0",
                      "    g%dlon = 0.125d0; g%dlat = 0.125d0; g%periodic_x = 0",
                      "    m%src_t = planes(1); m%src_p = planes(2); m%src_q = planes(3); m%src_lw = c_null_ptr",
                      "    m%dst_t = planes(4); m%dst_p = planes(5); m%dst_q = planes(6); m%dst_lw = c_null_ptr",
                      "    m%dz = planes(7); m%lapse = -0.0065; m%fill = -1.e33",
                      "    e(1)%src = planes(8); e(1)%dst = planes(9); e(1)%adjust = c_null_ptr",
                      "    e(1)%scale = 0.0; e(1)%fill = -1.e33; e(1)%mode = NOAHMP_REGRID_NEAREST",
                      "    rc = noahmp_hip_forcing_regrid_met(plan, ncell, g, m, 1, e, c_null_ptr)",
                      "    rc = noahmp_hip_forcing_regrid_met(plan, ncell, g, m, 0, e, c_null_ptr)",
                      "  end function go", "end module regrid_met_abi_check", ""])
    f = tmp_path / "regrid_met_abi_check.f90"
    f.write_text(text)
    subprocess.check_call([tr._flang(), "-c", str(f), "-o", str(tmp_path / "regrid_met_abi_check.o"), "-J", str(tmp_path)], cwd=str(tmp_path))


# ---------------------------------------------------------------------------------------------------------------- GPU
_dev = tr._dev
POISON = 7.0


def _met_call(engine, g, plan_d, ncell, src_d, dst, dz_d, lw, entries, fill=-999.0):
    import torch
    torch.cuda.synchronize()
    met = engine.regrid_met(src_d[0], src_d[1], src_d[2], dst[0], dst[1], dst[2], dz_d, src_lw=src_d[3] if lw else None,
                            dst_lw=dst[3] if lw else None, lapse=float(LAPSE), fill=fill)
    engine.forcing_regrid_met(plan_d, ncell, g, met, entries)
    engine.stream_sync()


@pytest.mark.gpu
@pytest.mark.parametrize("ncell, n", [(256, 0), (256, 3), (1028, 32), (4, 3), (335, 3), (335, 32), (1, 0)])
def test_gpu_met_kernel_equals_np_met_on_both_paths(engine, ncell, n):
    """noahmp_hip_forcing_regrid_met against np_met over np_regrid: every input set, with and without src_lw, plain and periodic sources.
    The met call runs one column per thread whatever the alignment (1028: five workgroups, the last one ragged), while the separate
    noahmp_hip_forcing_regrid call its ordinary entries are compared with takes the four-column path at 256, 4 and 1028 aligned columns;
    the same call into destinations offset by one float must give the same bits.  Guard words around every destination stay as they
    were, and the n ordinary entries of the call equal that separate call."""
    import torch
    for name in ("plain", "periodic"):
        g = SOURCES[name]
        plan = case(name, ncell)[0]
        plan_d = _dev(plan.reshape(-1))
        r = np.random.default_rng(100 * n + ncell)
        srcs = [_dev(nasty(r, g.nx * g.ny)) for _ in range(n)]
        adjs = [_dev(nasty(r, ncell)) if f % 3 != 1 else None for f in range(n)]
        modes = [NEAR if f % 4 == 3 else BIL for f in range(n)]
        scales = [-0.0065 if f % 2 else 1.5 for f in range(n)]
        fills = [-999.0 - f for f in range(n)]
        alone = torch.full((max(n, 1), ncell), POISON, dtype=torch.float32, device="cuda")
        if n:
            tr._run(engine, g, plan_d, ncell, srcs, [alone[f] for f in range(n)], adjs, modes, scales, fills)
        alone_h = alone.cpu().numpy()
        pool = torch.full((4 + n, ncell + 8), POISON, dtype=torch.float32, device="cuda")
        for which in SETS:
            src, dz, want = reference(name, ncell, which)
            src_d = [_dev(s) for s in src]
            dz_d = _dev(dz)
            for lw in (True, False):
                for off in (0, 1):
                    pool.fill_(POISON)
                    lo = (4 + off) if ncell % 4 == 0 else off
                    dst = [pool[f, lo:lo + ncell] for f in range(4 + n)]
                    if ncell % 4 == 0:
                        assert all(d.data_ptr() % 16 == 4 * off for d in dst) and dz_d.data_ptr() % 16 == 0 and plan_d.data_ptr() % 16 == 0
                    ents = [(srcs[f], dst[4 + f], modes[f], adjs[f], scales[f], fills[f]) for f in range(n)]
                    _met_call(engine, g, plan_d, ncell, src_d, dst, dz_d, lw, ents)
                    h = pool.cpu().numpy()
                    what = "%s ncell %d n %d set %s lw=%d offset %d" % (name, ncell, n, which, lw, off)
                    for f, o in enumerate(OPERANDS[:4]):
                        if f == 3 and not lw:
                            assert (h[3] == POISON).all(), what + ": dst_lw written without src_lw"
                        else:
                            assert_same(h[f, lo:lo + ncell], want[f], what + " plane " + o)
                    for f in range(n):
                        assert_same(h[4 + f, lo:lo + ncell], alone_h[f], what + " ordinary entry %d" % f)
                    assert (h[:, :lo] == POISON).all() and (h[:, lo + ncell:] == POISON).all(), what + ": guard words"


@pytest.mark.gpu
def test_gpu_masked_source_cells_never_reach_a_valid_column(engine):
    """Cells the plan's mask dropped hold NaN in all four sources; no output of a column with valid corners is NaN."""
    import torch
    ni, nj = 64, 4
    for name in ("plain", "periodic"):
        g = SOURCES[name]
        xlat, xlon, v, plan, unf = tr.plan_case(name, ni, nj, "random", 2)
        n = ni * nj
        r = np.random.default_rng(3)
        x = physical(r, g.nx * g.ny)
        src = [np.where(v.astype(bool), x[o], F(np.nan)).astype(F) for o in OPERANDS[:4]]
        dz = physical(r, n)["dz"]
        coarse = [np_regrid(plan, g, s, BIL) for s in src]
        want = np_met(*coarse, dz)
        fl = filled(plan, g)
        assert 0 < fl.sum() < n and not any(np.isnan(w[~fl]).any() for w in want)
        dst = torch.full((4, n), POISON, dtype=torch.float32, device="cuda")
        _met_call(engine, g, _dev(plan.reshape(-1)), n, [_dev(s) for s in src], [dst[f] for f in range(4)], _dev(dz), True, [], fill=-5.0)
        h = dst.cpu().numpy()
        for f, o in enumerate(OPERANDS[:4]):
            assert not np.isnan(h[f]).any(), o
            assert_same(h[f], np.where(fl, F(-5.0), want[f]).astype(F), "%s masked, plane %s" % (name, o))


@pytest.mark.gpu
@pytest.mark.parametrize("ncell", [256, 255])
def test_gpu_hand_made_plan_out_of_range_gives_fill_in_all_four_planes(engine, ncell):
    """base negative, nx*ny and INT_MAX: fill in all four planes.  The sources have 64 spare words behind them (a value no cell holds), so
    an implementation without the check reads them and fails the comparison instead of faulting."""
    import torch
    for name in ("plain", "periodic"):
        g = SOURCES[name]
        nxny = g.nx * g.ny
        r = np.random.default_rng(ncell + 1)
        plan, _ = value_cases(r, g, ncell)
        bad = r.permutation(ncell)[:min(40, ncell)]
        for q, c in enumerate(bad):
            plan[0, c] = plan[1, c] = (-1, -(2 ** 31), nxny, 2 ** 31 - 1, nxny + 17)[q % 5]
            if q % 5 == 4:
                plan[2:, c].view(F)[:] = (1, 0, 0, 0)
        x = physical(r, nxny)
        full = [np.concatenate([x[o], np.full(64, 12345.0, F)]) for o in OPERANDS[:4]]
        dz = physical(r, ncell)["dz"]
        fl = filled(plan, g)
        assert fl[bad].all()
        want = np_met(*[np_regrid(plan, g, s, BIL) for s in full], dz)
        want = [np.where(fl, F(-77.0), w).astype(F) for w in want]
        full_d = [_dev(s) for s in full]
        dst = torch.full((4, ncell + 8), POISON, dtype=torch.float32, device="cuda")
        _met_call(engine, g, _dev(plan.reshape(-1)), ncell, [s[:nxny] for s in full_d], [dst[f, :ncell] for f in range(4)], _dev(dz), True, [],
                  fill=-77.0)
        h = dst.cpu().numpy()
        for f, o in enumerate(OPERANDS[:4]):
            assert (h[f, :ncell][bad] == F(-77.0)).all(), o
            assert_same(h[f, :ncell], want[f], "%s hand-made plan, plane %s" % (name, o))
        assert (h[:, ncell:] == POISON).all()


@pytest.mark.gpu
def test_gpu_met_refusals_launch_nothing(engine):
    """Every -105 and -107 refusal returns its code with text, and the destinations keep their poison."""
    import torch
    g = SOURCES["plain"]
    lib = engine.lib
    ncell = 256
    plan = case("plain", ncell)[0]
    plan_d = _dev(plan.reshape(-1))
    src, dz, want = reference("plain", ncell, "physical")
    src_d, dz_d = [_dev(s) for s in src], _dev(dz)
    dst = torch.full((4 + 33, ncell), POISON, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def met(**kw):
        m = engine.regrid_met(src_d[0], src_d[1], src_d[2], dst[0], dst[1], dst[2], dz_d, src_lw=src_d[3], dst_lw=dst[3], lapse=float(LAPSE),
                              fill=-999.0)
        for k, val in kw.items():
            setattr(m, k, val)
        return m

    def call(m, n, e, grid=g, p=plan_d.data_ptr(), nc=ncell):
        rc = lib.noahmp_hip_forcing_regrid_met(p, nc, C.byref(grid), C.byref(m) if m is not None else None, n, e, None)
        engine.stream_sync()
        return rc, lib.noahmp_hip_last_error().decode()
    e = engine.regrid_entries([(src_d[0], dst[4 + f], "bilinear", None, 0.0, -1.0) for f in range(32)])
    e33 = (abi.RegridEntry * 33)()
    for f in range(33):
        e33[f].src, e33[f].dst, e33[f].mode = src_d[0].data_ptr(), dst[4 + f].data_ptr(), BIL
    for n, ee in ((33, e33), (-1, e)):
        rc, msg = call(met(), n, ee)
        assert rc == -107 and "entries" in msg, (n, rc, msg)
    rc, msg = call(None, 32, e)
    assert rc == -105 and "met" in msg
    for field in ("src_t", "src_p", "src_q", "dst_t", "dst_p", "dst_q", "dz"):
        rc, msg = call(met(**{field: None}), 32, e)
        assert rc == -105 and "met" in msg, (field, rc, msg)
    rc, msg = call(met(dst_lw=None), 32, e)
    assert rc == -105 and "dst_lw" in msg
    rc, msg = call(met(), 32, e, p=None)
    assert rc == -105 and "plan" in msg
    rc, msg = call(met(), 32, e, grid=tr.source(1, 5, 0.0, 0.0, 1.0, 1.0))
    assert rc == -105 and "nx" in msg
    rc, msg = call(met(), 32, e, nc=-1)
    assert rc == -105 and "columns" in msg
    rc, msg = call(met(), 1, None)
    assert rc == -105 and "entries" in msg
    for bad, what in (("mode", 2), ("src", None), ("dst", None)):
        keep = getattr(e[5], bad)
        setattr(e[5], bad, what)
        rc, msg = call(met(), 32, e)
        assert rc == -105 and "entry 5" in msg, (bad, rc, msg)
        setattr(e[5], bad, keep)
    assert (dst.cpu().numpy() == POISON).all()
    # and the same blocks are served once nothing is wrong; src_lw = NULL with any dst_lw is no refusal
    rc, msg = call(met(src_lw=None), 0, None)
    assert rc == 0
    h = dst.cpu().numpy()
    for f in range(3):
        assert_same(h[f], want[f], "after the refusals, plane %d" % f)
    assert (h[3:] == POISON).all()
    rc, msg = call(met(), 32, e)
    assert rc == 0
    h = dst.cpu().numpy()
    assert_same(h[3], want[3], "after the refusals, lw")
    assert_same(h[4 + 31], np_regrid(plan, g, src[0], BIL, fill=-1.0), "after the refusals, entry 31")
    assert (h[4 + 32] == POISON).all()


@pytest.mark.gpu
def test_gpu_chain_with_elevation_equals_the_chain_fed_with_restated_fine_records(engine, tables):
    """Two steps of test_regrid._chain's 64 x 8 tile: coarse records through ForcingRegrid.set_elevation + record, forcing_interpolate_prep
    and noahmplsm, against the same chain fed with fine records made by np_met / np_regrid and uploaded: every INOUT and OUT array
    bit-identical.  The same through a sorted store (follow) returns the same columns at the permuted positions."""
    import torch
    from noahmp_amd.regrid import ForcingRegrid
    from tools.compare import exact_check
    g = tr.CHAIN_SRC
    r = np.random.default_rng(19)
    names = list(tr.COARSE)
    coarse = [{k: r.uniform(lo, hi, g.nx * g.ny).astype(F).reshape(g.ny, g.nx) for k, (lo, hi) in tr.COARSE.items()} for _ in range(3)]
    z_src = r.uniform(200.0, 900.0, g.nx * g.ny).astype(F).reshape(g.ny, g.nx)
    z_model = r.uniform(100.0, 1500.0, (8, 64)).astype(F)
    plan, unf = np_plan(tr.CHAIN_LAT, tr.CHAIN_LON, g)
    assert unf == 0
    z_fine = np_regrid(plan, g, z_src.ravel(), BIL)
    z_model.ravel()[:5] = z_fine[:5]                                                # some columns on the source's own terrain
    dz = z_model.ravel() - z_fine
    assert (dz[:5] == 0).all() and (dz[5:] != 0).all()
    modes = {"pcp": "nearest"}

    def restated(k):
        fine = {nm: np_regrid(plan, g, coarse[k][nm].ravel(), NEAR if nm in modes else BIL, None, 0.0, np.nan) for nm in names}
        fine["t"], fine["p"], fine["q"], fine["lw"] = np_met(fine["t"], fine["p"], fine["q"], fine["lw"], dz)
        return {nm: _dev(x.reshape(8, 64)) for nm, x in fine.items()}
    ref = tr._chain(engine, tables, restated).to_host()

    rg = ForcingRegrid(engine, _dev(tr.CHAIN_LAT), _dev(tr.CHAIN_LON), g)
    rg.set_elevation(_dev(z_model), _dev(z_src))
    assert_same(rg.dz.cpu().numpy().ravel(), dz, "dz")
    cd = [{k: _dev(v) for k, v in c.items()} for c in coarse]
    torch.cuda.synchronize()
    seen = []

    class Feed:
        def __call__(self, k):
            rec = rg.record(cd[k], modes=modes)
            seen.append(rec)
            return rec
        follow = staticmethod(rg.follow)
    got = tr._chain(engine, tables, Feed()).to_host()
    ok, lines = exact_check(ref, got)
    assert ok, "\n".join(lines)
    engine.stream_sync()
    want2 = restated(2)
    for nm in names:
        assert_same(seen[3][nm].cpu().numpy(), want2[nm].cpu().numpy(), "record 2, " + nm)
    # a record without longwave: t, p, q are still adjusted
    rec = rg.record({k: v for k, v in cd[1].items() if k != "lw"}, modes=modes)
    engine.stream_sync()
    want1 = restated(1)
    assert "lw" not in rec
    for nm in ("t", "p", "q", "u"):
        assert_same(rec[nm].cpu().numpy(), want1[nm].cpu().numpy(), "record without lw, " + nm)

    # the three refusals of the helper
    with pytest.raises(ValueError):
        rg.record({k: v for k, v in cd[0].items() if k != "p"}, modes=modes)
    with pytest.raises(ValueError):
        rg.record(cd[0], modes={"q": "nearest"})
    with pytest.raises(ValueError):
        rg.set_adjust("t", _dev(dz.reshape(8, 64)), scale=-0.0065)
    rg3 = ForcingRegrid(engine, _dev(tr.CHAIN_LAT), _dev(tr.CHAIN_LON), g)
    rg3.set_adjust("t", _dev(dz.reshape(8, 64)), scale=-0.0065)
    with pytest.raises(ValueError):
        rg3.set_elevation(_dev(z_model), _dev(z_src))

    # the sorted layout: the same columns at other positions
    rg2 = ForcingRegrid(engine, _dev(tr.CHAIN_LAT), _dev(tr.CHAIN_LON), g)
    rg2.set_elevation(_dev(z_model), _dev(z_src))

    class Feed2:
        def __call__(self, k):
            return rg2.record(cd[k], modes=modes)
        follow = staticmethod(rg2.follow)
    ds = tr._chain(engine, tables, Feed2(), sort=True)
    perm = ds.sort_perm.cpu().numpy()
    assert_same(rg2.dz.cpu().numpy().ravel(), dz[perm], "dz after follow")
    # set_elevation on a regrid that already follows the sorted store: z_model in the sorted order, the tile-order copy through the inverse
    rg4 = ForcingRegrid(engine, _dev(tr.CHAIN_LAT), _dev(tr.CHAIN_LON), g)
    rg4.follow(ds)
    rg4.set_elevation(_dev(z_model.ravel()[perm].reshape(8, 64)), _dev(z_src))
    assert_same(rg4.dz.cpu().numpy().ravel(), dz[perm], "dz of set_elevation after follow")
    assert_same(rg4.dz_tile.cpu().numpy().ravel(), dz, "tile-order dz of set_elevation after follow")
    rec4 = rg4.record(cd[2], modes=modes)
    engine.stream_sync()
    for nm in ("t", "p", "q", "lw", "pcp"):
        assert_same(rec4[nm].cpu().numpy().ravel(), want2[nm].cpu().numpy().ravel()[perm], "record after follow + set_elevation, " + nm)
    hs = ds.to_host()
    for k in ("tsk", "hfx", "tgxy", "smois", "t2mvxy"):
        x, y = np.asarray(ref.a[k]), np.asarray(hs.a[k])
        if x.ndim == 3:
            x, y = np.moveaxis(x, 1, 0).reshape(x.shape[1], -1), np.moveaxis(y, 1, 0).reshape(y.shape[1], -1)
            assert_same(y, x[:, perm], "sorted chain " + k)
        else:
            assert_same(y.ravel(), x.ravel()[perm], "sorted chain " + k)
