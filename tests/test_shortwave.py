"""Shortwave forcing on the device: zenith weighting in time, slope and aspect (noahmp_hip_forcing_cosz_mean, noahmp_hip_forcing_shortwave;
nmp_dev_shortwave.hpp).

No reference routine stands behind the calls; the contract is the text in include/noahmp_hip.h.  np_sun, np_mean and np_shortwave restate it
in numpy float32, one rounded operation per line, with glibc's own sinf / cosf called per element through ctypes (fmodf is exact, numpy's
is used).  Everything is compared with the restatement bit for bit (test_regrid.assert_same: equal bits, or both NaN): the per-column
functions compiled for the host, both kernels at every shape, and a two-step engine run through Shortwave.apply against the same run
with SWDOWN overwritten by the restated plane."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from noahmp_amd import abi
from noahmp_amd import shortwave as swmod
import test_regrid as tr
from test_regrid import F, assert_same, nasty

D = np.float64
ROOT = tr.ROOT
CSRC = tr.CSRC
SRC = os.path.join(ROOT, "tests", "host_emul", "shortwave_check.hip")
LIB = os.path.join(ROOT, "tests", "host_emul", "libshortwave_check.so")
LINEAR, ZENITH = 0, 1
DEGRAD = F(3.14159265) / F(180.0)
OPERANDS = ("sw_a", "sw_b", "mean_a", "lat", "lon", "ne", "nn", "nu")
SETS = ("physical", "nasty") + tuple("nasty_" + o for o in OPERANDS)
NCELLS_HOST = (256, 335, 1)
NCELLS_GPU = (1, 4, 255, 256, 335, 1028)
# (iday, ihour, iminute, isecond): the solstices and equinoxes, both sides of the JULIAN >= 80 test of the declination
TIMES = [(171, 18, 30, 0), (355, 6, 0, 0), (79, 23, 59, 59), (80, 0, 0, 1), (265, 12, 0, 0)]
# max_ratio, mu_min, max_terrain_ratio, solar_constant: the defaults of the helper, and caps low enough to be hit
PARS = [(10.0, 0.05, 5.0, 1361.0), (1.5, 0.2, 1.25, 1361.0)]
IDTS, IDTS2 = 1800, 10800


# ---------------------------------------------------------------------------------------------------------------- the restatement
_libm = C.CDLL("libm.so.6")
for _f in ("sinf", "cosf", "asinf"):
    getattr(_libm, _f).restype = C.c_float
    getattr(_libm, _f).argtypes = [C.c_float]


def _per_element(fn, x):
    """glibc's fn where |x| < 120, NaN for every other argument (the header's sinf / cosf)."""
    x = np.asarray(x, F)
    flat = x.ravel()
    out = np.full(flat.shape, np.nan, F)
    ok = np.abs(flat) < F(120.0)
    out[ok] = [fn(float(v)) for v in flat[ok]]
    return out.reshape(x.shape)


def sinf(x):
    return _per_element(_libm.sinf, x)


def cosf(x):
    return _per_element(_libm.cosf, x)


def max0(x):
    return np.where(x > 0, x, F(0.0)).astype(F)


def min_(a, b):
    return np.where(a < b, a, b).astype(F)


def np_suntime(t):
    """(hour_utc, sin_declin, cos_declin) of t = (iday, ihour, iminute, isecond): noahmp_hip_declination (hdrv:826-854) and hdrv:856."""
    iday, ihour, iminute, isecond = (int(v) for v in t)
    dpd = F(360.0) / F(365.0)
    julian = F(iday) + F(ihour) / F(24.0)
    obecl = F(23.5) * DEGRAD
    sinob = F(_libm.sinf(float(obecl)))
    if julian >= F(80.0):
        sxlong = (dpd * (julian - F(80.0))) * DEGRAD
    else:
        sxlong = (dpd * (julian + F(285.0))) * DEGRAD
    arg = sinob * F(_libm.sinf(float(sxlong)))
    declin = F(_libm.asinf(float(arg)))
    hour = (F(ihour) + F(iminute) / F(60.0)) + F(isecond) / F(3600.0)
    return F(hour), F(_libm.sinf(float(declin))), F(_libm.cosf(float(declin)))


def np_hrang(lon, hour):
    q = lon / F(15.0)
    t0 = hour + q
    t1 = t0 + F(24.0)
    tloc = np.fmod(t1, F(24.0)).astype(F)
    d = tloc - F(12.0)
    a = F(15.0) * d
    return a * DEGRAD


def np_sun(lat, lon, sun, trig=None):
    """(e, n, u) of the header text.  trig: (sinphi, cosphi) made once per column by the caller."""
    hour, sd, cd = (F(v) for v in sun)
    lat, lon = np.asarray(lat, F), np.asarray(lon, F)
    with np.errstate(all="ignore"):
        if trig is None:
            phi = lat * DEGRAD
            trig = sinf(phi), cosf(phi)
        sinphi, cosphi = trig
        h = np_hrang(lon, hour)
        ch, sh = cosf(h), sinf(h)
        ss = sinphi * sd
        cc = cosphi * cd
        cch = cc * ch
        u = ss + cch
        pe = cd * sh
        e = -pe
        cs = cosphi * sd
        sc = sinphi * cd
        sch = sc * ch
        n = cs - sch
    return e.astype(F), n.astype(F), u.astype(F)


def np_mean(lat, lon, suns):
    lat, lon = np.asarray(lat, F), np.asarray(lon, F)
    with np.errstate(all="ignore"):
        phi = lat * DEGRAD
        trig = sinf(phi), cosf(phi)
        acc = np.zeros(lat.shape, F)
        for sun in suns:
            acc = acc + max0(np_sun(lat, lon, sun, trig)[2])
        return (acc / F(len(suns))).astype(F)


def np_kd(kt):
    with np.errstate(all="ignore"):
        lo = F(1.0) - F(0.09) * kt
        p = F(12.336) * kt
        p = p - F(16.638)
        p = p * kt
        p = p + F(4.388)
        p = p * kt
        p = p - F(0.1604)
        p = p * kt
        p = p + F(0.9511)
        return np.where(kt <= F(0.22), lo, np.where(kt <= F(0.80), p, F(0.165))).astype(F)


def np_shortwave(x, mode, with_b, terrain, sun, par, idts=IDTS, idts2=IDTS2, parts=None):
    """noahmp_hip_forcing_shortwave over the operand dict x (OPERANDS).  parts, a dict, receives s, mu, kt, cosi and the cap arguments."""
    max_ratio, mu_min, max_tr, s0 = (F(v) for v in par)
    a = {k: np.asarray(v, F) for k, v in x.items()}
    with np.errstate(all="ignore"):
        if mode == LINEAR:
            if with_b:
                fraction = F(idts2 - idts) / F(idts2)
                one_minus = F(1.0) - fraction
                s = (a["sw_a"] * fraction) + (a["sw_b"] * one_minus)
            else:
                s = a["sw_a"].copy()
            if not terrain:
                return s.astype(F)
        e, n, u = np_sun(a["lat"], a["lon"], sun)
        mu = max0(u)
        if mode == ZENITH:
            ratio = mu / a["mean_a"]
            capped = min_(ratio, max_ratio)
            s = np.where(a["mean_a"] > 0, a["sw_a"] * capped, F(0.0)).astype(F)
            if parts is not None:
                parts.update(ratio=ratio)
        if parts is not None:
            parts.update(s=s, mu=mu, u=u)
        if not terrain:
            return s.astype(F)
        pe = e * a["ne"]
        pn = n * a["nn"]
        pu = u * a["nu"]
        pen = pe + pn
        cosi = pen + pu
        top = s0 * mu
        kt = s / top
        kd = np_kd(kt)
        rr = max0(cosi) / mu
        r = min_(rr, max_tr)
        beam = F(1.0) - kd
        br = beam * r
        f = kd + br
        keep = ((a["ne"] == 0) & (a["nn"] == 0)) | (mu < mu_min)
        if parts is not None:
            parts.update(kt=kt, cosi=cosi, rr=rr, keep=keep)
        return np.where(keep, s, s * f).astype(F)


# ---------------------------------------------------------------------------------------------------------------- the inputs
def physical(r, n):
    """Operands over the ranges of a real tile: latitudes -89..89, every longitude (so every local hour at any UTC time), slopes up to 60
    degrees of every aspect with some flat normals of either sign of zero, shortwave up to 1100 W/m2."""
    lat = r.uniform(-89.0, 89.0, n).astype(F)
    lat[:min(4, n)] = np.array([89.0, -89.0, 0.0, 66.5], F)[:min(4, n)]
    slope, asp = r.uniform(0.0, np.pi / 3, n), r.uniform(0.0, 2 * np.pi, n)
    ne, nn, nu = (np.sin(slope) * np.sin(asp)).astype(F), (np.sin(slope) * np.cos(asp)).astype(F), np.cos(slope).astype(F)
    z = r.random(n)
    flat = z < 0.08
    ne[flat], nn[flat], nu[flat] = F(0.0), F(0.0), F(1.0)
    ne[z < 0.04] = F(-0.0)
    nn[z < 0.02] = F(-0.0)
    return dict(sw_a=r.uniform(0.0, 1100.0, n).astype(F), sw_b=r.uniform(0.0, 1100.0, n).astype(F), mean_a=r.uniform(0.0, 1.0, n).astype(F),
                lat=lat, lon=r.uniform(-180.0, 180.0, n).astype(F), ne=ne, nn=nn, nu=nu)


@functools.lru_cache(maxsize=None)
def operands(ncell, which):
    r = np.random.default_rng(4000 + ncell)
    phys = physical(r, ncell)
    nas = {o: nasty(r, ncell) for o in OPERANDS}
    x = {o: (nas if which in ("nasty", "nasty_" + o) else phys)[o] for o in OPERANDS}
    if which == "physical":
        # the interval mean of the column itself for a part of the columns (polar night: exactly zero), so ZENITH sees real ratios
        m = np_mean(x["lat"], x["lon"], [np_suntime(TIMES[1]), np_suntime((355, 7, 0, 0)), np_suntime((355, 8, 0, 0))])
        x = dict(x)
        x["mean_a"] = np.where(np.arange(ncell) % 2 == 0, m, x["mean_a"]).astype(F)
    for v in x.values():
        v.setflags(write=False)
    return x


def configs():
    """(mode, with_b, terrain, time index, parameter index): every mode with and without sw_b and terrain, the times and both
    parameter sets spread over them."""
    out = []
    k = 0
    for mode, with_b in ((LINEAR, False), (LINEAR, True), (ZENITH, False), (ZENITH, True)):
        for terrain in (False, True):
            for ti in range(len(TIMES)):
                out.append((mode, with_b, terrain, ti, k % len(PARS)))
                k += 1
    return out


CONFIGS = configs()
SPECIAL_SUNS = [(F(6.0), F(0.0), F(0.0)), (F(6.0), F(-0.0), F(0.0))]       # u = +0.0 in every column: the sun exactly on the horizon


@functools.lru_cache(maxsize=None)
def reference(ncell, which, cfg):
    mode, with_b, terrain, ti, pi = cfg
    out = np_shortwave(operands(ncell, which), mode, with_b, terrain, np_suntime(TIMES[ti]), PARS[pi])
    out.setflags(write=False)
    return out


def sample_sets(nsample):
    """nsample times of a three-hour interval that starts at TIMES[0] and one that crosses midnight of day 79 / 80."""
    return [[t[1:] for t in swmod.sample_times((2001,) + start, 10800, nsample, at)]
            for start, at in (((171, 18, 0, 0), "start"), ((79, 22, 0, 0), "mid"))]


@functools.lru_cache(maxsize=None)
def mean_reference(ncell, which, nsample, k):
    x = operands(ncell, which)
    out = np_mean(x["lat"], x["lon"], [np_suntime(t) for t in sample_sets(nsample)[k]])
    out.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------------------- CPU
def build():
    deps = [SRC, os.path.join(CSRC, "nmp_dev_shortwave.hpp"), os.path.join(CSRC, "nmp_dev_forcing.hpp"), os.path.join(CSRC, "nmp_libm.hpp"),
            os.path.join(CSRC, "nmp_libm_tables.inc"), os.path.join(ROOT, "include", "noahmp_hip.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off",
                               "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), SRC, "-o", LIB])


@functools.lru_cache(maxsize=None)
def _host():
    build()
    try:
        import torch  # noqa: F401  (map torch's HIP runtime first, noahmp_amd/abi.py::load_library)
    except ImportError:
        pass
    lib = C.CDLL(LIB)
    V, Fl = C.c_void_p, C.c_float
    lib.shortwave_sun.argtypes = [C.c_long, V, V, Fl, Fl, Fl, V, V, V, V]
    lib.shortwave_forcing_cosz.argtypes = [C.c_long, V, V, Fl, Fl, Fl, V]
    lib.shortwave_mean.argtypes = [C.c_long, V, V, C.c_int, V, V]
    lib.shortwave_values.argtypes = [C.c_long] + [V] * 8 + [C.c_int] + [Fl] * 5 + [V, V]
    lib.shortwave_kd.argtypes = [C.c_long, V, V]
    for f in ("shortwave_sun", "shortwave_forcing_cosz", "shortwave_mean", "shortwave_values", "shortwave_kd"):
        getattr(lib, f).restype = None
    return lib


def _p(a):
    return a.ctypes.data if a is not None else None


def host_values(x, mode, with_b, terrain, sun, par, idts=IDTS, idts2=IDTS2):
    lib = _host()
    n = x["sw_a"].size
    fraction = F(idts2 - idts) / F(idts2) if (mode == LINEAR and with_b) else F(1.0)
    one_minus = F(1.0) - fraction
    out = np.full(n, 7.0, F)
    parv = np.array(par, F)
    a = {k: np.ascontiguousarray(v, F) for k, v in x.items()}
    lib.shortwave_values(n, _p(a["sw_a"]), _p(a["sw_b"]) if with_b else None, _p(a["mean_a"]) if mode == ZENITH else None, _p(a["lat"]),
                         _p(a["lon"]), *[(_p(a[k]) if terrain else None) for k in ("ne", "nn", "nu")], mode, float(fraction), float(one_minus),
                         float(sun[0]), float(sun[1]), float(sun[2]), _p(parv), _p(out))
    return out


def host_mean(lat, lon, suns):
    out = np.full(lat.size, 7.0, F)
    sv = np.array(suns, F).reshape(-1)
    _host().shortwave_mean(lat.size, _p(np.ascontiguousarray(lat)), _p(np.ascontiguousarray(lon)), len(suns), _p(sv), _p(out))
    return out


def host_sun(lat, lon, sun):
    o = [np.full(lat.size, 7.0, F) for _ in range(4)]
    _host().shortwave_sun(lat.size, _p(np.ascontiguousarray(lat)), _p(np.ascontiguousarray(lon)), float(sun[0]), float(sun[1]), float(sun[2]),
                          *[_p(a) for a in o])
    return o


def test_the_restated_sun_is_the_librarys_sun():
    """np_suntime against noahmp_hip_declination of the built library (host code) at every sample time the tests use."""
    lib = abi.load_library()
    times = TIMES + [(0, 0, 0, 0), (364, 23, 59, 59), (79, 23, 0, 0), (80, 0, 0, 0)] + [t for n in (1, 2, 7, 64) for s in sample_sets(n) for t in s]
    for t in times:
        sd, cd = C.c_float(0), C.c_float(0)
        lib.noahmp_hip_declination(t[0], t[1], C.byref(sd), C.byref(cd))
        hour, wsd, wcd = np_suntime(t)
        assert F(sd.value) == wsd and F(cd.value) == wcd, t


def test_the_inputs_cover_what_they_are_meant_to():
    x = operands(335, "physical")
    assert np.signbit(x["ne"][(x["ne"] == 0)]).any() and not np.signbit(x["ne"][(x["ne"] == 0)]).all()
    assert (x["mean_a"] == 0).any(), "polar night"
    seen = dict(lo=False, hi=False, shaded=False, cap_r=False, cap_t=False, night=False, kt1=False, branch79=False)
    for cfg in CONFIGS:
        mode, with_b, terrain, ti, pi = cfg
        parts = {}
        np_shortwave(x, mode, with_b, terrain, np_suntime(TIMES[ti]), PARS[pi], parts=parts)
        if mode == ZENITH:
            seen["cap_r"] |= bool((parts["ratio"][x["mean_a"] > 0] > PARS[pi][0]).any())
            seen["night"] |= bool((parts["mu"] == 0).any())
        if terrain:
            live = ~parts["keep"]
            seen["lo"] |= bool((parts["mu"] < PARS[pi][1]).any())
            seen["hi"] |= bool(live.any())
            seen["shaded"] |= bool((parts["cosi"][live] <= 0).any())
            seen["cap_t"] |= bool((parts["rr"][live] > PARS[pi][2]).any())
            seen["kt1"] |= bool((parts["kt"][live] > 1).any())
    seen["branch79"] = F(79) + F(23) / F(24) < F(80) <= F(80) + F(0) / F(24)
    assert all(seen.values()), seen


@pytest.mark.parametrize("ncell", NCELLS_HOST)
def test_host_compilation_equals_the_restatement(ncell):
    """nmp_dev_shortwave.hpp compiled for the host against np_sun / np_mean / np_shortwave: every input set and configuration."""
    for which in SETS:
        x = operands(ncell, which)
        for t in TIMES[:2]:
            sun = np_suntime(t)
            e, n, u, ua = host_sun(x["lat"], x["lon"], sun)
            we, wn, wu = np_sun(x["lat"], x["lon"], sun)
            for got, want, nm in ((e, we, "e"), (n, wn, "n"), (u, wu, "u"), (ua, wu, "u alone")):
                assert_same(got, want, "sun %s n=%d set %s time %s" % (nm, ncell, which, t))
        for cfg in CONFIGS:
            mode, with_b, terrain, ti, pi = cfg
            got = host_values(x, mode, with_b, terrain, np_suntime(TIMES[ti]), PARS[pi])
            assert_same(got, reference(ncell, which, cfg), "n=%d set %s cfg %s" % (ncell, which, cfg))
        if which in ("physical", "nasty", "nasty_lat", "nasty_lon"):
            for nsample in (1, 2, 7, 64):
                for k, times in enumerate(sample_sets(nsample)):
                    got = host_mean(x["lat"], x["lon"], [np_suntime(t) for t in times])
                    assert_same(got, mean_reference(ncell, which, nsample, k), "mean n=%d set %s nsample %d interval %d" % (ncell, which, nsample, k))


def test_host_special_suns_breakpoints_and_nasty_parameters():
    """The sun exactly on the horizon (u = +0.0 everywhere, also with mu_min = 0, where the terrain step divides by zero), kt exactly on
    both Erbs breakpoints and beyond 1, and NaN / Inf / -0.0 in each parameter in turn."""
    x = dict(operands(335, "physical"))
    for sun in SPECIAL_SUNS:
        assert (np_sun(x["lat"], x["lon"], sun)[2] == 0).all()
        for par in (PARS[0], (10.0, 0.0, 5.0, 1361.0), (10.0, -1.0, 5.0, 1361.0)):
            for mode in (LINEAR, ZENITH):
                assert_same(host_values(x, mode, True, True, sun, par), np_shortwave(x, mode, True, True, sun, par), "horizon %s %s" % (par, mode))
    # kt on the breakpoints: LINEAR without sw_b, so s = sw_a; sw_a is searched so that the float32 quotient is the breakpoint itself
    sun = np_suntime(TIMES[4])
    par = PARS[0]
    u = np_sun(x["lat"], x["lon"], sun)[2]
    top = F(par[3]) * max0(u)
    sw = x["sw_a"].copy()
    hit = {"lo": 0, "hi": 0}
    day = np.flatnonzero(u > 0.3)
    assert day.size > 40
    for q, c in enumerate(day):
        bp = F(0.22) if q % 3 == 0 else F(0.80)
        if q % 3 == 2:
            sw[c] = F(1.5) * top[c]
            continue
        cand = F(bp * top[c])
        for _ in range(4):
            cand = np.nextafter(cand, F(0))
        for _ in range(9):
            if F(cand / top[c]) == bp:
                sw[c] = cand
                hit["lo" if q % 3 == 0 else "hi"] += 1
                break
            cand = np.nextafter(cand, F(np.inf))
    assert hit["lo"] > 3 and hit["hi"] > 3, hit
    x["sw_a"] = sw
    parts = {}
    want = np_shortwave(x, LINEAR, False, True, sun, par, parts=parts)
    live = ~parts["keep"]
    assert (parts["kt"][live] == F(0.22)).any() and (parts["kt"][live] == F(0.80)).any() and (parts["kt"][live] > 1).any()
    assert_same(host_values(x, LINEAR, False, True, sun, par), want, "Erbs breakpoints")
    kt = np.concatenate([np.array([0.22, 0.80, 0.0, -0.0, 1.0, 1.2, np.nan, np.inf, -np.inf, -1.0], F), np.nextafter(F(0.22), F(1)).reshape(1),
                         np.nextafter(F(0.80), F(1)).reshape(1), np.random.default_rng(1).uniform(0, 1.2, 500).astype(F)])
    kd = np.zeros_like(kt)
    _host().shortwave_kd(kt.size, _p(kt), _p(kd))
    assert_same(kd, np_kd(kt), "kd")
    # the diffuse fraction is continuous at 0.22 to the paper's four digits and runs into 0.165 at 0.80
    assert abs(float(np_kd(np.array([0.22], F))[0]) - float(np_kd(np.nextafter(F(0.22), F(1)).reshape(1))[0])) < 2e-3
    assert abs(float(np_kd(np.array([0.80], F))[0]) - 0.165) < 1.5e-2
    x0 = operands(256, "physical")
    for bad in (np.nan, np.inf, -np.inf, -0.0, 1e-40):
        for k in range(4):
            par = list(PARS[0])
            par[k] = bad
            for mode in (LINEAR, ZENITH):
                assert_same(host_values(x0, mode, True, True, np_suntime(TIMES[0]), par), np_shortwave(x0, mode, True, True, np_suntime(TIMES[0]), par),
                            "parameter %d = %r, mode %d" % (k, bad, mode))


def test_properties():
    x = operands(335, "physical")
    r = np.random.default_rng(5)
    # one sample at `now`: the ratio is exactly 1, the output has the bits of sw_a
    for t in TIMES:
        sun = np_suntime(t)
        mean = host_mean(x["lat"], x["lon"], [sun])
        u = host_sun(x["lat"], x["lon"], sun)[2]
        assert_same(mean, max0(u), "one sample: the mean is max(u, 0)")
        y = dict(x, mean_a=mean)
        got = host_values(y, ZENITH, False, False, sun, PARS[0])
        up = mean > 0
        assert up.sum() > 50 and (~up).sum() > 50
        assert_same(got[up], x["sw_a"][up], "nsample = 1: the bits of sw_a")
        assert (got[~up] == 0).all() and not np.signbit(got[~up]).any()
    # u is forcing_cosz: the compiled function itself, and the compiled reference's COSZ of the fixture
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "golden_declin.npz")))
    for i, when in enumerate(g["when"]):
        y, mo, d, h, mi, sec = (int(v) for v in when)
        iday = sum((31, 29 if swmod.days_in_year(y) == 366 else 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31)[:mo - 1]) + d - 1
        sun = np_suntime((iday, h, mi, sec))
        assert F(iday) + F(h) / F(24.0) == g["julian%02d" % i], when
        u = host_sun(g["lat"], g["lon"], sun)[2]
        assert_same(u, g["cosz%02d" % i], "u against the reference's COSZ, %s" % (when,))
        assert_same(np_sun(g["lat"], g["lon"], sun)[2], g["cosz%02d" % i], "restated u against the reference's COSZ, %s" % (when,))
        cz = np.zeros_like(u)
        _host().shortwave_forcing_cosz(u.size, _p(g["lat"]), _p(g["lon"]), float(sun[0]), float(sun[1]), float(sun[2]), _p(cz))
        assert_same(u, cz, "u against forcing_cosz")
    # LINEAR without terrain: the bits of interp2; without sw_b: sw_a
    fraction = F(IDTS2 - IDTS) / F(IDTS2)
    want = (x["sw_a"] * fraction) + (x["sw_b"] * (F(1.0) - fraction))
    assert_same(host_values(x, LINEAR, True, False, np_suntime(TIMES[0]), PARS[0]), want, "LINEAR is interp2")
    assert_same(host_values(x, LINEAR, False, False, np_suntime(TIMES[0]), PARS[0]), x["sw_a"], "LINEAR without sw_b")
    # flat normals and low-sun columns keep the bits of s
    for mode in (LINEAR, ZENITH):
        for ti in range(len(TIMES)):
            sun = np_suntime(TIMES[ti])
            s = host_values(x, mode, True, False, sun, PARS[1])
            st = host_values(x, mode, True, True, sun, PARS[1])
            mu = max0(host_sun(x["lat"], x["lon"], sun)[2])
            keep = ((x["ne"] == 0) & (x["nn"] == 0)) | (mu < F(PARS[1][1]))
            assert keep.sum() > 20 and (~keep).sum() > 20
            assert_same(st[keep], s[keep], "flat or low sun: the bits of s")
            lit = ~keep & (s != 0)
            assert (st[lit] != s[lit]).mean() > 0.9
    # unit vector, and the geometry of a slope: facing the sun gains, facing away keeps the diffuse part only
    e, n, u, _ = host_sun(x["lat"], x["lon"], np_suntime(TIMES[0]))
    assert np.abs(e.astype(D) ** 2 + n.astype(D) ** 2 + u.astype(D) ** 2 - 1.0).max() < 1e-6
    del r


def test_zenith_weighting_conserves_the_energy_of_the_interval():
    """When the step times are the sample times and max_ratio is not hit, the float64 mean of the ZENITH outputs over the interval equals
    sw_a to relative 1e-5: at most nsample + 2 <= 66 float32 roundings of 2^-24 each, about 4e-6."""
    r = np.random.default_rng(8)
    n = 400
    x = physical(r, n)
    par = (100.0, 0.05, 5.0, 1361.0)               # the ratio is at most nsample <= 64: this cap is never hit
    for nsample, start in ((1, (2001, 171, 18, 0, 0)), (7, (2001, 171, 12, 0, 0)), (36, (2001, 79, 15, 0, 0)), (64, (2001, 355, 9, 0, 0))):
        times = [t[1:] for t in swmod.sample_times(start, 10800, nsample)]
        suns = [np_suntime(t) for t in times]
        mean = host_mean(x["lat"], x["lon"], suns)
        y = dict(x, mean_a=mean)
        parts = [dict() for _ in suns]
        outs = [np_shortwave(y, ZENITH, False, False, sun, par, parts=p) for sun, p in zip(suns, parts)]
        up = mean > 0
        assert up.sum() > 100
        for p in parts:
            assert not (p["ratio"][up] >= par[0]).any(), "the cap must not be hit by the chosen inputs"
        for sun, o in zip(suns, outs):
            assert_same(host_values(y, ZENITH, False, False, sun, par), o, "ZENITH, nsample %d" % nsample)
        avg = np.mean(np.stack(outs).astype(D), axis=0)
        dev = np.abs(avg[up] - x["sw_a"][up].astype(D)) / x["sw_a"][up].astype(D)
        print("energy conservation, nsample %d: max relative deviation %.3g" % (nsample, dev.max()))
        assert dev.max() <= 1e-5, (nsample, dev.max())
        assert (avg[~up] == 0).all()


def _f64(x, mode, with_b, terrain, sun, par):
    """The same formulas in float64 from the same float32 inputs (libm's double sin / cos); returns the output and the branch arguments."""
    a = {k: np.asarray(v, F).astype(D) for k, v in x.items()}
    max_ratio, mu_min, max_tr, s0 = (D(F(v)) for v in par)
    hour, sd, cd = (D(v) for v in sun)
    dg = D(DEGRAD)
    fraction = D(F(IDTS2 - IDTS) / F(IDTS2))
    s = a["sw_a"] * fraction + a["sw_b"] * D(F(1.0) - F(IDTS2 - IDTS) / F(IDTS2)) if with_b else a["sw_a"]
    phi = a["lat"] * dg
    h = 15.0 * (np.fmod(hour + a["lon"] / 15.0 + 24.0, 24.0) - 12.0) * dg
    u = np.sin(phi) * sd + np.cos(phi) * cd * np.cos(h)
    e = -cd * np.sin(h)
    n = np.cos(phi) * sd - np.sin(phi) * cd * np.cos(h)
    mu = np.maximum(u, 0.0)
    args = dict(u=u, mu=mu)
    if mode == ZENITH:
        ratio = mu / a["mean_a"]
        s = np.where(a["mean_a"] > 0, a["sw_a"] * np.minimum(ratio, max_ratio), 0.0)
        args["ratio_cap"] = ratio - max_ratio
    if terrain:
        cosi = e * a["ne"] + n * a["nn"] + u * a["nu"]
        with np.errstate(all="ignore"):
            kt = s / (s0 * mu)
            kd = np.where(kt <= D(F(0.22)), 1.0 - D(F(0.09)) * kt,
                          np.where(kt <= D(F(0.80)), (((D(F(12.336)) * kt - D(F(16.638))) * kt + D(F(4.388))) * kt - D(F(0.1604))) * kt + D(F(0.9511)),
                                   D(F(0.165))))
            rr = np.maximum(cosi, 0.0) / mu
            out = s * (kd + (1.0 - kd) * np.minimum(rr, max_tr))
        keep = ((a["ne"] == 0) & (a["nn"] == 0)) | (mu < mu_min)
        s = np.where(keep, s, out)
        args.update(kt22=kt - D(F(0.22)), kt80=kt - D(F(0.80)), mumin=mu - mu_min, cosi=cosi, terr_cap=rr - max_tr, keep=keep)
    return s, args


def test_every_output_agrees_with_float64():
    """Every output of the host compilation against a float64 evaluation of the same formulas over 200 000 physical draws (kt spread over
    (0, 1.2); LINEAR with terrain, ZENITH, ZENITH with terrain) and the interval mean over 20 000.
    The measure.  The float32 hour angle carries an absolute error of about ulp(24 h) * 15 * DEGRAD = 5e-7, so u does, whatever its
    size; an output proportional to mu then has the relative error 5e-7 / mu, unbounded towards the horizon, and the Erbs polynomial
    multiplies it by up to 8 (its slope in kt is steepest where kd is smallest).  So a sunlit draw is judged by its relative deviation
    times mu -- the deviation in units of u -- and a night draw (mu = 0: exact zeros, or the bits of s with terrain) by the relative
    deviation itself.  MEASURED is the largest such figure seen here (3.86e-6, LINEAR with terrain; ZENITH with terrain 3.02e-6, ZENITH
    alone 7.3e-7, the interval mean 5.4e-7; the pure relative deviation of draws with mu >= 0.05 was 5.4e-5 / 1.8e-5 / 1.3e-5 / 4.9e-6); the tolerance is five times that, so other draws do not flake, and is asserted to be
    <= 1e-4, so a wrong constant (>= 1e-3 relative on every draw with mu > 0.1) cannot pass.
    Left out, and asserted to be <= 1 % of the draws: those whose float64 kt, mu - mu_min, cosi or cap argument lies within 1e-5 of a branch
    boundary, u = 0 (the branch of max0) among them: float32 and float64 may take different sides."""
    MEASURED = 3.86e-6
    TOL = 5 * MEASURED
    assert TOL <= 1e-4
    r = np.random.default_rng(21)
    n = 200000
    x = physical(r, n)
    x["mean_a"] = r.uniform(0.05, 1.0, n).astype(F)
    sun = np_suntime(TIMES[0])
    par = PARS[0]
    # kt spread over (0, 1.2) where the sun is up: sw_a = kt * S0 * mu (ZENITH scales it by the ratio again, which keeps a wide spread)
    u64 = _f64(x, LINEAR, False, False, sun, par)[1]["mu"]
    x["sw_a"] = np.where(u64 > 0, r.uniform(0.0, 1.2, n) * 1361.0 * u64, x["sw_a"]).astype(F)
    x["sw_b"] = x["sw_a"]
    worst = {}
    left_out = 0
    total = 0

    def figures(name, got, want, mu, near):
        nonlocal left_out, total
        left_out += int(near.sum())
        total += got.size
        with np.errstate(all="ignore"):
            rel = np.where(want == 0, np.abs(got), np.abs(got - want) / np.abs(want))
        dev = np.where(mu > 0, rel * mu, rel)[~near]
        worst[name] = float(dev.max())
        print("float64 agreement %s: max deviation %.3g (pure relative, sun above 0.05: %.3g), left out %d" %
              (name, worst[name], rel[~near & (mu >= 0.05)].max(), near.sum()))
    for mode, with_b, terrain in ((LINEAR, True, True), (ZENITH, False, False), (ZENITH, False, True)):
        got = host_values(x, mode, with_b, terrain, sun, par).astype(D)
        want, a = _f64(x, mode, with_b, terrain, sun, par)
        near = np.abs(a["u"]) < 1e-5
        if mode == ZENITH:
            near |= np.abs(a["ratio_cap"]) < 1e-5
        if terrain:
            live = ~a["keep"]
            for k in ("kt22", "kt80", "cosi", "terr_cap"):
                near |= live & (np.abs(a[k]) < 1e-5)
            near |= np.abs(a["mumin"]) < 1e-5
        figures("mode %d terrain %d" % (mode, terrain), got, want, a["mu"], near)
    lat, lon = x["lat"][:20000], x["lon"][:20000]
    times = [t[1:] for t in swmod.sample_times((2001, 171, 18, 0, 0), 10800, 12)]
    suns = [np_suntime(t) for t in times]
    got = host_mean(lat, lon, suns).astype(D)
    dummy = dict(lat=lat, lon=lon, sw_a=lat, sw_b=lat, mean_a=lat, ne=lat, nn=lat, nu=lat)
    us = np.array([_f64(dummy, LINEAR, False, False, s, par)[1]["u"] for s in suns])
    want = np.mean(np.maximum(us, 0.0), axis=0)
    figures("interval mean", got, want, want, (np.abs(us) < 1e-5).any(axis=0))
    print("left out %d of %d" % (left_out, total))
    assert left_out <= 0.01 * total, (left_out, total)
    for k, v in worst.items():
        assert v <= TOL, (k, v)


def test_bindings_regenerate_identically_with_the_shortwave_calls():
    from tools import gen_abi
    for rel, text in (("include/noahmp_hip.h", gen_abi.c_header()), ("oracle/ref_harness_gen.f90", gen_abi.ref_harness()),
                      ("noahmp_amd/fortran/module_sf_noahmpdrv_hip.F90", gen_abi.fortran_shim()),
                      ("tests/fortran/shim_wrap_gen.f90", gen_abi.shim_wrap())):
        assert open(os.path.join(ROOT, rel)).read() == text, rel
    hdr = open(os.path.join(ROOT, "include", "noahmp_hip.h")).read()
    for word in ("typedef struct noahmp_sun_time {", "} noahmp_sun_time;", "typedef struct noahmp_shortwave {", "} noahmp_shortwave;",
                 "#define NOAHMP_HIP_HAS_FORCING_SHORTWAVE 1\n", "#define NOAHMP_HIP_ABI_VERSION 1\n", "#define NOAHMP_HIP_ABI_MINOR 3\n",
                 "#define NOAHMP_SW_LINEAR 0", "#define NOAHMP_SW_ZENITH 1", "#define NOAHMP_SW_MAX_SAMPLES 64\n",
                 "noahmp_hip_forcing_cosz_mean(", "noahmp_hip_forcing_shortwave(",
                 "u      = (sinphi*sin_declin) + ((cosphi*cos_declin)*cosf(hrang))", "e      = -(cos_declin*sinf(hrang))",
                 "n      = (cosphi*sin_declin) - ((sinphi*cos_declin)*cosf(hrang))", "mean[c] = acc / (float)nsample",
                 "cosi = ((e*ne) + (n*nn)) + (u*nu)", "kt   = s / (solar_constant*mu)", "r    = min(max0(cosi) / mu, max_terrain_ratio)",
                 "s    = s * (kd + ((1.0f - kd)*r))", "((((12.336f*kt - 16.638f)*kt + 4.388f)*kt - 0.1604f)*kt) + 0.9511f",
                 "Shadows", "NOT represented"):
        assert word in hdr, word
    assert "noahmp_shortwave" not in gen_abi.ref_harness() and "noahmp_sun_time" not in gen_abi.ref_harness()
    f90 = open(os.path.join(ROOT, "noahmp_amd", "fortran", "module_sf_noahmpdrv_hip.F90")).read()
    for word in ("bind(C, name='noahmp_hip_forcing_cosz_mean')", "bind(C, name='noahmp_hip_forcing_shortwave')",
                 "type, bind(C) :: noahmp_shortwave", "type, bind(C) :: noahmp_sun_time", "NOAHMP_SW_LINEAR = 0, NOAHMP_SW_ZENITH = 1"):
        assert word in f90, word
    assert "noahmp_hip_forcing_cosz_mean" in abi.EXPORTED_SYMBOLS and "noahmp_hip_forcing_shortwave" in abi.EXPORTED_SYMBOLS
    assert [n for n, _ in abi.Shortwave._fields_] == ["sw_a", "sw_b", "mean_a", "xlat", "lon", "normal_e", "normal_n", "normal_u", "swdown", "idts",
                                                      "idts2", "mode", "max_ratio", "mu_min", "max_terrain_ratio", "solar_constant"]
    assert [n for n, _ in abi.SunTime._fields_] == ["iday", "ihour", "iminute", "isecond"]
    assert abi.SW_MODE == {"linear": 0, "zenith": 1}


def test_ctypes_mirrors_match_the_compiled_header(tmp_path):
    body = ""
    want = []
    for cname, M in (("noahmp_shortwave", abi.Shortwave), ("noahmp_sun_time", abi.SunTime)):
        names = [n for n, _ in M._fields_]
        body += 'printf(" %%zu", sizeof(%s));' % cname + "".join('printf(" %%zu", offsetof(%s, %s));' % (cname, n) for n in names)
        want += [C.sizeof(M)] + [getattr(M, n).offset for n in names]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "noahmp_hip.h"\nint main(){' + body +
                   'printf(" %d %d", NOAHMP_HIP_ABI_MINOR, NOAHMP_HIP_HAS_FORCING_SHORTWAVE); return 0;}')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert out == want + [3, 1]


def test_library_exports_the_shortwave_calls():
    if not os.path.exists(abi.LIB_PATH):
        from noahmp_amd import build as b
        b.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", abi.LIB_PATH]).decode()
    assert " T noahmp_hip_forcing_cosz_mean\n" in out and " T noahmp_hip_forcing_shortwave\n" in out


@pytest.mark.skipif(tr._flang() is None, reason="no flang")
def test_generated_fortran_types_and_interfaces_compile(tmp_path):
    """The shortwave part of the generated module compiles, and a caller of both interfaces type-checks."""
    from tools import gen_abi
    text = "\n".join(["module shortwave_abi_check", "  use iso_c_binding", "  implicit none"] + gen_abi.shortwave_f90_types() + ["  interface"] +
                     gen_abi.shortwave_f90_interfaces() +
                     ["  end interface", "contains", "  function go(ncell, planes) result(rc)", "    integer(c_int64_t), value :: ncell",
                      "    type(c_ptr), intent(in) :: planes(9)", "    type(noahmp_shortwave) :: sw", "    type(noahmp_sun_time) :: t(36)",
                      "    integer(c_int) :: rc", "    integer :: k", "    do k = 1, 36",
                      "      t(k)%iday = 171; t(k)%ihour = 18 + (k-1)/12; t(k)%iminute = 5*mod(k-1, 12); t(k)%isecond = 0", "    end do",
                      "    rc = noahmp_hip_forcing_cosz_mean(planes(4), planes(5), ncell, 36, t, planes(3), c_null_ptr)",
                      "    sw%sw_a = planes(1); sw%sw_b = c_null_ptr; sw%mean_a = planes(3); sw%xlat = planes(4); sw%lon = planes(5)",
                      "    sw%normal_e = planes(6); sw%normal_n = planes(7); sw%normal_u = planes(8); sw%swdown = planes(9)",
                      "    sw%idts = 0; sw%idts2 = 0; sw%mode = NOAHMP_SW_ZENITH; sw%max_ratio = 10.0; sw%mu_min = 0.05",
                      "    sw%max_terrain_ratio = 5.0; sw%solar_constant = 1361.0",
                      "    rc = noahmp_hip_forcing_shortwave(sw, ncell, t(7), c_null_ptr)",
                      "  end function go", "end module shortwave_abi_check", ""])
    f = tmp_path / "shortwave_abi_check.f90"
    f.write_text(text)
    subprocess.check_call([tr._flang(), "-c", str(f), "-o", str(tmp_path / "shortwave_abi_check.o"), "-J", str(tmp_path)], cwd=str(tmp_path))


def test_terrain_from_height_on_a_plane():
    """z = a*x + b*y: the exact slope and aspect in the interior and at the edges (one-sided differences), with and without rotation."""
    import torch
    a, b, dx, dy = 0.25, -0.5, 100.0, 200.0
    jj, ii = np.meshgrid(np.arange(7), np.arange(9), indexing="ij")
    z = torch.from_numpy((a * dx * ii + b * dy * jj).astype(F))                      # whole numbers: the differences are exact
    e, n, u, slope, aspect = swmod.normal_from_height(z, dx, dy)
    g = np.hypot(a, b)
    want = np.array([-a, -b, 1.0]) / np.sqrt(1.0 + g * g)
    for got, w in zip((e, n, u), want):
        assert np.abs(got.numpy() - w).max() < 1e-6
    assert np.abs(slope.numpy() - np.arctan(g)).max() < 1e-6
    az = np.arctan2(-a, -b) % (2 * np.pi)                                             # downslope: towards -grad z
    assert np.abs(aspect.numpy() - az).max() < 1e-6
    # the normal of set_terrain(slope, aspect) is the same vector
    s, asp = slope.numpy().astype(D), aspect.numpy().astype(D)
    for got, w in zip((e, n, u), (np.sin(s) * np.sin(asp), np.sin(s) * np.cos(asp), np.cos(s))):
        assert np.abs(got.numpy() - w).max() < 1e-6
    # a grid whose y axis points alpha east of... rotated against true north: the gradient turns with WRF's wind rotation
    alpha = 0.3
    ca, sa = torch.full_like(z, np.cos(alpha)), torch.full_like(z, np.sin(alpha))
    e2, n2, u2, slope2, aspect2 = swmod.normal_from_height(z, dx, dy, ca, sa)
    ge, gn = a * np.cos(alpha) - b * np.sin(alpha), a * np.sin(alpha) + b * np.cos(alpha)
    assert np.abs(slope2.numpy() - np.arctan(g)).max() < 1e-6
    assert np.abs(aspect2.numpy() - (np.arctan2(-ge, -gn) % (2 * np.pi))).max() < 1e-6
    assert np.abs(e2.numpy() - (-ge / np.sqrt(1 + g * g))).max() < 1e-6 and np.abs(u2.numpy() - u.numpy()).max() < 1e-6
    # a single row or column has no gradient along the missing direction
    e3, n3, u3, _, _ = swmod.normal_from_height(z[:1], dx, dy)
    assert (n3 == 0).all() and np.abs(e3.numpy() - (-a / np.sqrt(1 + a * a))).max() < 1e-6


def test_date_arithmetic_rolls_over():
    assert swmod.time_after((2000, 365, 23, 59, 59), 1) == (2001, 0, 0, 0, 0)              # 2000 is a leap year: days 0..365
    assert swmod.time_after((2001, 364, 23, 0, 0), 7200) == (2002, 0, 1, 0, 0)
    assert swmod.time_after((2100, 364, 23, 0, 0), 3600) == (2101, 0, 0, 0, 0)              # 2100 is not
    assert swmod.sample_times((2001, 79, 22, 0, 0), 10800, 3) == [(2001, 79, 22, 0, 0), (2001, 79, 23, 0, 0), (2001, 80, 0, 0, 0)]
    assert swmod.sample_times((2001, 79, 22, 0, 0), 10800, 3, "mid") == [(2001, 79, 22, 30, 0), (2001, 79, 23, 30, 0), (2001, 80, 0, 30, 0)]
    assert len(swmod.sample_times((2001, 10, 0, 0, 0), 21600, 64)) == 64


# ---------------------------------------------------------------------------------------------------------------- GPU
_dev = tr._dev
POISON = 7.0


def _block(engine, xd, dst, mode, with_b, terrain, par, **kw):
    args = dict(sw_b=xd["sw_b"] if with_b else None, mean_a=xd["mean_a"] if mode == ZENITH else None,
                normal=(xd["ne"], xd["nn"], xd["nu"]) if terrain else None, idts=IDTS, idts2=IDTS2, mode=mode, max_ratio=par[0], mu_min=par[1],
                max_terrain_ratio=par[2], solar_constant=par[3])
    args.update(kw)
    return engine.shortwave_block(xd["sw_a"], xd["lat"], xd["lon"], dst, **args)


@pytest.mark.gpu
@pytest.mark.parametrize("ncell", NCELLS_GPU)
def test_gpu_kernels_equal_the_restatement_on_both_paths(engine, ncell):
    """Both kernels against the restatement: every input set, all modes with and without sw_b and terrain, nsample 1, 7 and 64.  With 4, 256
    and 1028 aligned columns the LINEAR calls without normals take the four-column path, else -- and into destinations offset by one
    float -- the one-column path of every other call: the same bits.  1028 columns are five workgroups of the one-column path, the last
    one ragged.  Guard words around
    every destination stay as they were."""
    import torch
    pool = torch.full((ncell + 8,), POISON, dtype=torch.float32, device="cuda")
    for which in SETS:
        x = operands(ncell, which)
        xd = {k: _dev(v) for k, v in x.items()}
        torch.cuda.synchronize()
        for off in (0, 1):
            lo = (4 + off) if ncell % 4 == 0 else off
            dst = pool[lo:lo + ncell]
            if ncell % 4 == 0:
                assert dst.data_ptr() % 16 == 4 * off and all(t.data_ptr() % 16 == 0 for t in xd.values())
            for cfg in CONFIGS:
                mode, with_b, terrain, ti, pi = cfg
                pool.fill_(POISON)
                torch.cuda.synchronize()
                engine.forcing_shortwave(_block(engine, xd, dst, mode, with_b, terrain, PARS[pi]), ncell, TIMES[ti])
                engine.stream_sync()
                h = pool.cpu().numpy()
                what = "ncell %d set %s cfg %s offset %d" % (ncell, which, cfg, off)
                assert_same(h[lo:lo + ncell], reference(ncell, which, cfg), what)
                assert (h[:lo] == POISON).all() and (h[lo + ncell:] == POISON).all(), what + ": guard words"
            if which in ("physical", "nasty", "nasty_lat", "nasty_lon"):
                for nsample in (1, 7, 64):
                    for k, times in enumerate(sample_sets(nsample)):
                        pool.fill_(POISON)
                        torch.cuda.synchronize()
                        engine.cosz_mean(xd["lat"], xd["lon"], times, dst)
                        engine.stream_sync()
                        h = pool.cpu().numpy()
                        what = "mean ncell %d set %s nsample %d interval %d offset %d" % (ncell, which, nsample, k, off)
                        assert_same(h[lo:lo + ncell], mean_reference(ncell, which, nsample, k), what)
                        assert (h[:lo] == POISON).all() and (h[lo + ncell:] == POISON).all(), what + ": guard words"


@pytest.mark.gpu
def test_gpu_refusals_launch_nothing(engine):
    """Every refusal returns its code with text, the destinations keep their poison, and the same blocks are served afterwards."""
    import torch
    lib = engine.lib
    ncell = 256
    x = operands(ncell, "physical")
    xd = {k: _dev(v) for k, v in x.items()}
    dst = torch.full((2, ncell), POISON, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    now = engine.sun_times([TIMES[0]])
    cfg = (ZENITH, False, True, 0, 0)

    def blk(**kw):
        b = _block(engine, xd, dst[0], ZENITH, True, True, PARS[0])
        for k, v in kw.items():
            setattr(b, k, v)
        return b

    def call(b, nc=ncell, t=now):
        rc = lib.noahmp_hip_forcing_shortwave(C.byref(b) if b is not None else None, nc, t, None)
        engine.stream_sync()
        return rc, lib.noahmp_hip_last_error().decode()
    for field in ("sw_a", "xlat", "lon", "swdown"):
        rc, msg = call(blk(**{field: None}))
        assert rc == -105 and "required" in msg, (field, rc, msg)
    rc, msg = call(blk(mean_a=None))
    assert rc == -105 and "mean_a" in msg
    for gone in (("normal_e",), ("normal_n",), ("normal_u",), ("normal_e", "normal_n"), ("normal_n", "normal_u"), ("normal_e", "normal_u")):
        rc, msg = call(blk(**{k: None for k in gone}))
        assert rc == -105 and "all three or none" in msg, (gone, rc, msg)
    for mode in (2, -1):
        rc, msg = call(blk(mode=mode))
        assert rc == -105 and "mode" in msg
    rc, msg = call(blk(), nc=-1)
    assert rc == -105 and "columns" in msg
    rc, msg = call(blk(), t=None)
    assert rc == -105 and "now" in msg
    rc, msg = call(None)
    assert rc == -105 and "NULL" in msg
    for idts, idts2 in ((1800, 0), (-1, 10800), (10801, 10800)):
        rc, msg = call(blk(mode=LINEAR, idts=idts, idts2=idts2))
        assert rc == -105 and "bracketing" in msg, (idts, idts2, rc, msg)

    def mean_call(nsample, times, lat=xd["lat"].data_ptr(), lon=xd["lon"].data_ptr(), out=dst[1].data_ptr(), nc=ncell):
        rc = lib.noahmp_hip_forcing_cosz_mean(lat, lon, nc, nsample, times, out, None)
        engine.stream_sync()
        return rc, lib.noahmp_hip_last_error().decode()
    t65 = engine.sun_times([TIMES[0]] * 65)
    for nsample in (0, 65, -3):
        rc, msg = mean_call(nsample, t65)
        assert rc == -107 and "samples" in msg, (nsample, rc, msg)
    rc, msg = mean_call(3, None)
    assert rc == -105 and "times" in msg
    for kw in (dict(lat=None), dict(lon=None), dict(out=None)):
        rc, msg = mean_call(3, t65, **kw)
        assert rc == -105 and "required" in msg, (kw, rc, msg)
    rc, msg = mean_call(3, t65, nc=-1)
    assert rc == -105 and "columns" in msg
    assert (dst.cpu().numpy() == POISON).all()
    # ncell == 0 returns 0 and writes nothing; then the same blocks are served
    assert call(blk(), nc=0)[0] == 0 and mean_call(3, t65, nc=0)[0] == 0
    assert (dst.cpu().numpy() == POISON).all()
    rc, msg = call(blk())
    assert rc == 0, msg
    rc, msg = mean_call(64, t65)
    assert rc == 0, msg
    h = dst.cpu().numpy()
    assert_same(h[0], reference(ncell, "physical", cfg), "after the refusals")
    assert_same(h[1], np_mean(x["lat"], x["lon"], [np_suntime(TIMES[0])] * 64), "after the refusals, the mean")
    # ZENITH does not read sw_b, idts or idts2: a block with a NULL sw_b and idts2 = 0 is no refusal
    rc, msg = call(blk(sw_b=None, idts=5, idts2=0))
    assert rc == 0, msg
    assert_same(dst.cpu().numpy()[0], reference(ncell, "physical", cfg), "ZENITH without sw_b")


CHAIN_NI, CHAIN_NJ = 64, 8
_jj, _ii = np.meshgrid(np.arange(CHAIN_NJ), np.arange(CHAIN_NI), indexing="ij")
CHAIN_LAT = (34.6 + 0.9 * _jj + 0.01 * _ii).astype(F)
CHAIN_LON = (-20.0 + 1.1 * _ii - 0.05 * _jj).astype(F)           # at 18 UTC of day 171 the terminator crosses the tile
CHAIN_START = (2000, 171, 18, 0, 0)


@pytest.mark.gpu
def test_gpu_coszin_of_forcing_prep_equals_the_single_sample_mean(engine, tables):
    """After forcing_prep at time T and cosz_mean with the single sample T on the same planes, max(COSZIN, 0) is the mean, bit for bit."""
    import torch
    from noahmp_amd import synth
    T, tb = tables
    s = synth.mixed_small(tb, ni=CHAIN_NI, nj=CHAIN_NJ)
    s.a["xlatin"][...] = CHAIN_LAT
    d = s.to_device("cuda:0")
    lon = _dev(CHAIN_LON)
    rain = torch.zeros((CHAIN_NJ, CHAIN_NI), dtype=torch.float32, device="cuda:0")
    mean = torch.full((CHAIN_NJ, CHAIN_NI), POISON, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    for t in ((171, 18, 0, 0), (171, 19, 30, 0), (79, 17, 59, 59), (355, 6, 10, 5)):
        engine.forcing_prep(d, lon, rain, *t)
        engine.cosz_mean(d.a["xlatin"], lon, [t], mean)
        engine.stream_sync()
        cz = d.a["coszin"].cpu().numpy()
        assert (cz > 0).any() and (cz <= 0).any(), t
        assert_same(mean.cpu().numpy(), max0(cz), "COSZIN at %s" % (t,))
        assert_same(cz.ravel(), np_sun(CHAIN_LAT.ravel(), CHAIN_LON.ravel(), np_suntime(t))[2], "COSZIN against the restated u at %s" % (t,))


def _sw_chain(engine, tables, recs, feed, sort=False):
    """Two steps of a 64 x 8 synth.mixed_small tile: forcing_interpolate_prep, feed(store, it, rec_a, rec_b, now) writes SWDOWN, noahmplsm."""
    import torch
    from noahmp_amd import synth
    T, tb = tables
    s = synth.mixed_small(tb, ni=CHAIN_NI, nj=CHAIN_NJ)
    s.a["xlatin"][...] = CHAIN_LAT
    synth.first_step_fixups(s)
    synth.diurnal_forcing(s, 12, t_offset=s.t_offset)
    d = s.to_device("cuda:0")
    lon = _dev(CHAIN_LON)
    rain = torch.zeros((CHAIN_NJ, CHAIN_NI), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    perm = None
    if sort:
        engine.sort_store(d)
        perm = d.sort_perm.long()
        lon = lon.reshape(-1)[perm].reshape(CHAIN_NJ, CHAIN_NI).contiguous()
        recs = [{k: v.reshape(-1)[perm].reshape(CHAIN_NJ, CHAIN_NI).contiguous() for k, v in r.items()} for r in recs]
        torch.cuda.synchronize()
    feed.start(d, perm)
    linear = []
    for it in (1, 2):
        now = (171, 18, 30 * (it - 1), 0)
        jul = engine.forcing_interpolate_prep(d, recs[0], recs[1], 1800 * (it - 1), 10800, rain, lon, *now, scale_vegfra=True,
                                              first_step=(it == 1))
        linear.append(d.a["swdown"].cpu().numpy().copy())
        feed(d, it, recs[0], recs[1], now)
        torch.cuda.synchronize()
        engine.stream_sync()
        st = engine.noahmplsm(d, it, 2000, jul)
        assert st.code == 0
    return d, linear


@pytest.mark.gpu
def test_gpu_chain_equals_the_chain_fed_with_the_restated_plane(engine, tables):
    """forcing_interpolate_prep, Shortwave.apply (ZENITH with terrain) and noahmplsm for two steps, against the same chain with SWDOWN
    overwritten by the restated plane uploaded from the host: every INOUT and OUT array bit-identical.  The sun is down over the eastern
    part of the tile: ZENITH writes exact zeros there where the linear path does not.  The same through a sorted store with follow
    returns the same columns at the permuted positions."""
    import torch
    from noahmp_amd.shortwave import Shortwave
    from tools.compare import exact_check
    r = np.random.default_rng(29)
    recs_h = [{k: r.uniform(lo, hi, (CHAIN_NJ, CHAIN_NI)).astype(F) for k, (lo, hi) in tr.COARSE.items()} for _ in range(2)]
    recs = [{k: _dev(v) for k, v in rec.items()} for rec in recs_h]
    slope = _dev(r.uniform(0.0, 0.8, (CHAIN_NJ, CHAIN_NI)).astype(F))
    aspect = _dev(r.uniform(0.0, 2 * np.pi, (CHAIN_NJ, CHAIN_NI)).astype(F))
    slope[0, :6] = 0.0                                                             # some flat columns
    par = dict(max_ratio=10.0, mu_min=0.05, max_terrain_ratio=5.0, solar_constant=1361.0)
    parv = (10.0, 0.05, 5.0, 1361.0)
    nsample = 6                                                                    # every 30 minutes: the step times are sample times
    sample_suns = [np_suntime(t[1:]) for t in swmod.sample_times(CHAIN_START, 10800, nsample)]

    class Device:
        def start(self, d, perm):
            self.sw = Shortwave(engine, _dev(CHAIN_LAT), _dev(CHAIN_LON), mode="zenith", **par)
            self.sw.set_terrain(slope, aspect)
            if perm is not None:
                self.sw.follow(d)
            self.sw.interval(CHAIN_START, 10800, nsample)

        def __call__(self, d, it, ra, rb, now):
            self.sw.apply(d, ra, rb, 1800 * (it - 1), 10800, now)
            engine.stream_sync()
    dev = Device()
    got_d, linear = _sw_chain(engine, tables, recs, dev)
    normal = [t.cpu().numpy().ravel() for t in dev.sw.normal_tile]
    assert (normal[0][:6] == 0).all() and (normal[1][:6] == 0).all()
    mean_h = np_mean(CHAIN_LAT.ravel(), CHAIN_LON.ravel(), sample_suns)
    assert_same(dev.sw.mean_a.cpu().numpy().ravel(), mean_h, "the interval mean of the helper")
    x = dict(sw_a=recs_h[0]["sw"].ravel(), sw_b=recs_h[1]["sw"].ravel(), mean_a=mean_h, lat=CHAIN_LAT.ravel(), lon=CHAIN_LON.ravel(),
             ne=normal[0], nn=normal[1], nu=normal[2])
    planes = [np_shortwave(x, ZENITH, False, True, np_suntime((171, 18, 30 * (it - 1), 0)), parv) for it in (1, 2)]
    for p, lin in zip(planes, linear):
        dark = p == 0
        assert 50 < dark.sum() < p.size - 50 and (lin.ravel()[dark] > 400).all(), "the sun is down over a part of the tile"

    class Restated:
        perm = None

        def start(self, d, perm):
            self.perm = perm.cpu().numpy() if perm is not None else None

        def __call__(self, d, it, ra, rb, now):
            p = planes[it - 1] if self.perm is None else planes[it - 1][self.perm]
            d.a["swdown"].copy_(_dev(p.reshape(CHAIN_NJ, CHAIN_NI)))
    ref_d, _ = _sw_chain(engine, tables, recs, Restated())
    assert_same(got_d.a["swdown"].cpu().numpy().ravel(), planes[1], "SWDOWN of the second step")
    ref, got = ref_d.to_host(), got_d.to_host()
    ok, lines = exact_check(ref, got)
    assert ok, "\n".join(lines)

    # the sorted layout: the same columns at other positions
    ds, _ = _sw_chain(engine, tables, recs, Device(), sort=True)
    perm = ds.sort_perm.cpu().numpy()
    assert_same(ds.a["swdown"].cpu().numpy().ravel(), planes[1][perm], "SWDOWN of the sorted chain")
    hs = ds.to_host()
    for k in ("tsk", "hfx", "tgxy", "smois", "t2mvxy", "fsaxy", "savxy", "sagxy"):
        a, b = np.asarray(ref.a[k]), np.asarray(hs.a[k])
        if a.ndim == 3:
            a, b = np.moveaxis(a, 1, 0).reshape(a.shape[1], -1), np.moveaxis(b, 1, 0).reshape(b.shape[1], -1)
            assert_same(b, a[:, perm], "sorted chain " + k)
        else:
            assert_same(b.ravel(), a.ravel()[perm], "sorted chain " + k)
    # mode "linear" of the helper without terrain leaves what forcing_interpolate_prep wrote
    lin = Shortwave(engine, _dev(CHAIN_LAT), _dev(CHAIN_LON), mode="linear")
    out = got_d.a["swdown"]
    lin.apply(got_d, recs[0], recs[1], 1800, 10800, (171, 18, 30, 0))
    engine.stream_sync()
    assert_same(out.cpu().numpy(), linear[1], "mode linear is the linear SWDOWN")
    with pytest.raises(ValueError):
        Shortwave(engine, _dev(CHAIN_LAT), _dev(CHAIN_LON), mode="zenith").apply(got_d, recs[0], recs[1], 1800, 10800, (171, 18, 30, 0))
