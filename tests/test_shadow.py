"""Cast shadows in the shortwave forcing: the terrain ray march and the lit shortwave step (noahmp_hip_forcing_shadow,
noahmp_hip_forcing_shortwave_lit; nmp_dev_shadow.hpp, nmp_dev_shortwave.hpp).

No reference routine stands behind the calls; the contract is the text in include/noahmp_hip.h.  np_ray, np_march, np_cells and np_lit restate
it in numpy float32, one rounded operation per line, on top of test_shortwave's np_sun / np_shortwave / np_kd.  Everything is compared with
the restatement bit for bit (test_regrid.assert_same: equal bits, or both NaN; exit codes as integers): the per-cell functions compiled for
the host, both kernels, and a two-step engine run through Shortwave.set_shadow / apply.  No tolerance appears anywhere.

The GPU suns.  The issue asks for latitude / longitude planes with 0.01-degree steps and times at which mu spans about 0.05 .. 0.15 over
the window; over 130 cells of 0.01 degrees mu changes by about 0.02 only, so the range is covered by three times instead -- mu at the
window's centre about 0.055 (the mu_min = 0.05 line crosses the window or lies next to it), 0.10 and 0.15, found by the restatement --
plus one noon and one night time."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from noahmp_amd import abi
import test_regrid as tr
import test_shortwave as ts
from test_regrid import F, assert_same, nasty
from test_shortwave import LINEAR, ZENITH, max0, min_, np_kd, np_shortwave, np_sun, np_suntime

ROOT = tr.ROOT
CSRC = tr.CSRC
SRC = os.path.join(ROOT, "tests", "host_emul", "shadow_check.hip")
LIB = os.path.join(ROOT, "tests", "host_emul", "libshadow_check.so")
CAST, LOW_SUN, NO_AXIS, LEFT, ABOVE, BAD_T, NSTEP = range(7)          # nmp::ShadowExit; only CAST gives lit = 0
WINDOWS = [(1, 1), (1, 7), (7, 1), (5, 3), (35, 67), (70, 130)]        # (ni, nj)
WINDOWS_GPU = [(1, 1), (5, 3), (35, 67), (70, 130)]
BIG = [(35, 67), (70, 130)]
NSTEP_TEST = 12
DX = 1000.0
AZIMUTHS = (10.0, 80.0, 135.0, 200.0, 260.0, 315.0)
ELEVATIONS = (3.0, 8.0, 20.0)
MU_MIN = 0.05
LITS = np.array([0.0, 0.25, np.nan, -0.0], F)
POISON = 7.0


# ---------------------------------------------------------------------------------------------------------------- the restatement
def np_ray(gx, gy, u, dx, dy):
    """major (0 none, 1 x, 2 y), d, t, rise of the header text, elementwise."""
    gx, gy, u = (np.asarray(v, F) for v in (gx, gy, u))
    dx, dy = F(dx), F(dy)
    with np.errstate(all="ignore"):
        ax = np.abs(gx) / dx
        ay = np.abs(gy) / dy
        xm = (ax >= ay) & (ax > 0)
        ym = ~xm & (ay > ax)
        a = np.where(xm, ax, ay).astype(F)
        d = np.where(xm, np.where(gx > 0, 1, -1), np.where(gy > 0, 1, -1)).astype(np.int64)
        qx = gx / dx
        qy = gy / dy
        t = np.where(xm, qy / a, qx / a).astype(F)
        rise = (u / a).astype(F)
    major = np.where(xm, 1, np.where(ym, 2, 0))
    return major, d, t, rise


def np_march(height, major, d, t, rise, nstep, height_max, todo=None):
    """How the march of every window cell ends (the exit codes above; -1 where todo is False), all cells advancing together step by step."""
    height = np.asarray(height, F)
    nj, ni = height.shape
    jj, ii = np.meshgrid(np.arange(nj, dtype=np.int64), np.arange(ni, dtype=np.int64), indexing="ij")
    ex = np.full((nj, ni), -9, np.int32)
    ex[major == 0] = NO_AXIS
    if todo is not None:
        ex[~todo] = -1
    xm = major == 1
    pos_m, pos_o = np.where(xm, ii, jj), np.where(xm, jj, ii)
    M, O = np.where(xm, ni, nj), np.where(xm, nj, ni)
    hmax = F(height_max)
    with np.errstate(all="ignore"):
        for k in range(1, int(nstep) + 1):
            live = ex == -9
            if not live.any():
                break
            kf = F(k)
            m = pos_m + k * d
            out = live & ((m < 0) | (m > M - 1))
            ex[out] = LEFT
            live &= ~out
            ray = (height + (kf * rise)).astype(F)
            out = live & (ray > hmax)
            ex[out] = ABOVE
            live &= ~out
            fo = (kf * t).astype(F)
            out = live & ~((fo >= -kf) & (fo <= kf))
            ex[out] = BAD_T
            live &= ~out
            jo = np.floor(fo).astype(F)
            w = (fo - jo).astype(F)
            o = pos_o + np.where(live, jo, F(0)).astype(np.int64)
            out = live & ((o < 0) | (o > O - 1))
            ex[out] = LEFT
            live &= ~out
            one = w == 0
            out = live & ~one & (o + 1 > O - 1)
            ex[out] = LEFT
            live &= ~out
            mc, oc = np.where(live, m, 0), np.where(live, o, 0)
            o1 = np.where(live & ~one, o + 1, oc)
            h0 = height[np.where(xm, oc, mc), np.where(xm, mc, oc)]
            h1 = height[np.where(xm, o1, mc), np.where(xm, mc, o1)]
            zt = np.where(one, h0, (h0 * (F(1.0) - w)) + (h1 * w)).astype(F)
            ex[live & (zt > ray)] = CAST
    ex[ex == -9] = NSTEP
    return ex


def lit_of(ex):
    return np.where(ex == CAST, F(0.0), F(1.0)).astype(F)


def np_march_dir(height, gx, gy, u, dx, dy, nstep, height_max):
    shape = np.asarray(height).shape
    gx, gy, u = (np.broadcast_to(np.asarray(v, F), shape) for v in (gx, gy, u))
    return np_march(height, *np_ray(gx, gy, u, dx, dy), nstep, height_max)


def np_cells(height, lat, lon, sun, dx, dy, nstep, mu_min, height_max, rot=None, dst_index=None, ndst=None):
    """noahmp_hip_forcing_shadow over a window: the exit codes in window order (-1: not marched) and the sun's mu."""
    height = np.asarray(height, F)
    ncell = height.size
    idx = np.arange(ncell).reshape(height.shape) if dst_index is None else np.asarray(dst_index).reshape(height.shape)
    ndst = ncell if ndst is None else ndst
    todo = (idx >= 0) & (idx < ndst)
    e, n, u = np_sun(lat, lon, sun)
    with np.errstate(all="ignore"):
        mu = max0(u)
        low = mu < F(mu_min)
        if rot is not None:
            ca, sa = (np.asarray(v, F) for v in rot)
            gx = (e * ca) + (n * sa)
            gy = (n * ca) - (e * sa)
        else:
            gx, gy = e, n
    ex = np_march(height, *np_ray(gx, gy, u, dx, dy), nstep, height_max, todo & ~low)
    ex[todo & low] = LOW_SUN
    return ex, mu


def np_lit(x, lit, mode, with_b, terrain, sun, par):
    """noahmp_hip_forcing_shortwave_lit over the operand dict x (test_shortwave.OPERANDS) and the lit plane."""
    max_ratio, mu_min, max_tr, s0 = (F(v) for v in par)
    lit = np.asarray(lit, F)
    a = {k: np.asarray(v, F) for k, v in x.items()}
    base = np_shortwave(x, mode, with_b, terrain, sun, par)
    s = np_shortwave(x, mode, with_b, False, sun, par)                       # the time stage
    e, n, u = np_sun(a["lat"], a["lon"], sun)
    with np.errstate(all="ignore"):
        mu = max0(u)
        top = s0 * mu
        kt = s / top
        kd = np_kd(kt)
        r0 = np.ones(lit.shape, F)
        if terrain:
            pe = e * a["ne"]
            pn = n * a["nn"]
            pu = u * a["nu"]
            pen = pe + pn
            cosi = pen + pu
            rr = max0(cosi) / mu
            flat = (a["ne"] == 0) & (a["nn"] == 0)
            r0 = np.where(flat, F(1.0), min_(rr, max_tr)).astype(F)
        r = r0 * lit
        beam = F(1.0) - kd
        br = beam * r
        f = kd + br
        out = np.where(mu < mu_min, s, s * f).astype(F)
    return np.where(lit == F(1.0), base, out).astype(F), dict(s=s, kd=kd, mu=mu)


# ---------------------------------------------------------------------------------------------------------------- the inputs
@functools.lru_cache(maxsize=None)
def terrain(ni, nj, centre_hill=False):
    """Gaussian hills on the grid: about one per 150 cells, sigma 1.5 .. 5 cells, 200 .. 1800 m, summed."""
    r = np.random.default_rng(7000 + 131 * ni + nj)
    nh = max(1, int(round(ni * nj / 150.0)))
    jj, ii = np.meshgrid(np.arange(nj), np.arange(ni), indexing="ij")
    z = np.zeros((nj, ni))
    hills = [(r.uniform(0, ni), r.uniform(0, nj), r.uniform(1.5, 5.0), r.uniform(200.0, 1800.0)) for _ in range(nh)]
    if centre_hill:
        hills.append((ni / 2.0 - 0.5, nj / 2.0 - 0.5, 3.0, 3000.0))          # stands on both cuts of a 2 x 2 decomposition
    for ci, cj, sg, hh in hills:
        z += hh * np.exp(-((ii - ci) ** 2 + (jj - cj) ** 2) / (2.0 * sg * sg))
    z = z.astype(F)
    z.setflags(write=False)
    return z


def direction(az, el):
    az, el = np.radians(az), np.radians(el)
    return F(np.cos(el) * np.sin(az)), F(np.cos(el) * np.cos(az)), F(np.sin(el))


@functools.lru_cache(maxsize=None)
def dir_reference(ni, nj, az, el):
    z = terrain(ni, nj)
    ex = np_march_dir(z, *direction(az, el), DX, DX, NSTEP_TEST, z.max())
    ex.setflags(write=False)
    return ex


def latlon(ni, nj):
    jj, ii = np.meshgrid(np.arange(nj), np.arange(ni), indexing="ij")
    return (39.0 + 0.01 * jj).astype(F), (-106.0 + 0.01 * ii).astype(F)


@functools.lru_cache(maxsize=None)
def sun_times():
    """(iday, ihour, iminute, isecond) of day 355 at which mu at (39.35 N, 105.65 W) is closest to 0.055, 0.10 and 0.15 in the afternoon,
    found by the restatement; one noon and one night time."""
    lat, lon = np.array([39.35], F), np.array([-105.65], F)
    best = {}
    for target in (0.055, 0.10, 0.15):
        for minute in range(19 * 60, 24 * 60):                                  # local afternoon: 12 .. 17 h
            t = (355, minute // 60, minute % 60, 0)
            mu = float(max0(np_sun(lat, lon, np_suntime(t))[2])[0])
            if target not in best or abs(mu - target) < best[target][0]:
                best[target] = (abs(mu - target), t)
    out = [best[k][1] for k in (0.055, 0.10, 0.15)]
    assert all(best[k][0] < 0.003 for k in best), best
    return out + [(171, 19, 0, 0), (355, 7, 0, 0)]                              # noon and night at 106 W


@functools.lru_cache(maxsize=None)
def cell_reference(ni, nj, ti, rot=False):
    z = terrain(ni, nj)
    lat, lon = latlon(ni, nj)
    ex, mu = np_cells(z, lat, lon, np_suntime(sun_times()[ti]), DX, DX, NSTEP_TEST, MU_MIN, z.max(), rot=rotation(ni, nj) if rot else None)
    ex.setflags(write=False)
    return ex, mu


def rotation(ni, nj):
    jj, ii = np.meshgrid(np.arange(nj), np.arange(ni), indexing="ij")
    alpha = 0.3 + 0.002 * ii - 0.001 * jj
    return np.cos(alpha).astype(F), np.sin(alpha).astype(F)


# ---------------------------------------------------------------------------------------------------------------- CPU
def build():
    deps = [SRC, os.path.join(CSRC, "nmp_dev_shadow.hpp"), os.path.join(CSRC, "nmp_dev_shortwave.hpp"), os.path.join(CSRC, "nmp_dev_forcing.hpp"),
            os.path.join(CSRC, "nmp_libm.hpp"), os.path.join(CSRC, "nmp_libm_tables.inc"), os.path.join(ROOT, "include", "noahmp_hip.h")]
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
    V, Fl, I = C.c_void_p, C.c_float, C.c_int
    lib.shadow_march_dir.argtypes = [I, I, V, V, V, V, Fl, Fl, I, Fl, I, V, V]
    lib.shadow_cells.argtypes = [I, I, V, V, V, V, V, V, C.c_long, Fl, Fl, Fl, Fl, Fl, I, Fl, Fl, V, V]
    lib.shadow_lit_values.argtypes = [C.c_long] + [V] * 9 + [I] + [Fl] * 5 + [V, V]
    for f in ("shadow_march_dir", "shadow_cells", "shadow_lit_values"):
        getattr(lib, f).restype = None
    return lib


_p = ts._p


def _c(a, dtype=F):
    return np.ascontiguousarray(a, dtype)


def host_march_dir(height, gx, gy, u, dx, dy, nstep, height_max, nf=4):
    height = _c(height)
    nj, ni = height.shape
    gx, gy, u = (_c(np.broadcast_to(np.asarray(v, F), height.shape)) for v in (gx, gy, u))
    ex = np.full(height.shape, -5, np.int32)
    lit = np.full(height.shape, POISON, F)
    _host().shadow_march_dir(ni, nj, _p(height), _p(gx), _p(gy), _p(u), float(dx), float(dy), int(nstep), float(height_max), nf, _p(ex), _p(lit))
    return ex, lit


def host_cells(height, lat, lon, sun, dx, dy, nstep, mu_min, height_max, rot=None, dst_index=None, ndst=None):
    height = _c(height)
    nj, ni = height.shape
    ndst = height.size if ndst is None else ndst
    ex = np.full(height.shape, -5, np.int32)
    lit = np.full(max(ndst, 1), POISON, F)
    keep = [_c(lat), _c(lon)] + ([_c(rot[0]), _c(rot[1])] if rot is not None else [None, None])
    idx = _c(dst_index, np.int32) if dst_index is not None else None
    _host().shadow_cells(ni, nj, _p(height), _p(keep[0]), _p(keep[1]), _p(keep[2]), _p(keep[3]), _p(idx), ndst, float(sun[0]), float(sun[1]),
                         float(sun[2]), float(dx), float(dy), int(nstep), float(mu_min), float(height_max), _p(ex), _p(lit))
    return ex, lit[:ndst]


def host_lit(x, lit, mode, with_b, terrain_, sun, par, idts=ts.IDTS, idts2=ts.IDTS2):
    n = x["sw_a"].size
    fraction = F(idts2 - idts) / F(idts2) if (mode == LINEAR and with_b) else F(1.0)
    one_minus = F(1.0) - fraction
    out = np.full(n, POISON, F)
    parv = np.array(par, F)
    a = {k: _c(v) for k, v in x.items()}
    lit = _c(lit)
    _host().shadow_lit_values(n, _p(lit), _p(a["sw_a"]), _p(a["sw_b"]) if with_b else None, _p(a["mean_a"]) if mode == ZENITH else None,
                              _p(a["lat"]), _p(a["lon"]), *[(_p(a[k]) if terrain_ else None) for k in ("ne", "nn", "nu")], mode,
                              float(fraction), float(one_minus), float(sun[0]), float(sun[1]), float(sun[2]), _p(parv), _p(out))
    return out


def same_exits(got, want, what):
    bad = got != want
    assert not bad.any(), "%s: %d of %d exits differ, first at %s: %d vs %d" % (what, bad.sum(), bad.size, tuple(np.argwhere(bad)[0]),
                                                                                 got[tuple(np.argwhere(bad)[0])], want[tuple(np.argwhere(bad)[0])])


@pytest.mark.parametrize("ni, nj", WINDOWS)
def test_host_compilation_equals_the_restatement(ni, nj):
    """shadow_ray / shadow_march compiled for the host against np_march at given directions (every azimuth and elevation; 1, 2 and 4 steps
    in flight give the same), and shadow_cell against np_cells at the real suns, with and without rotation planes."""
    z = terrain(ni, nj)
    for az in AZIMUTHS:
        for el in ELEVATIONS:
            want = dir_reference(ni, nj, az, el)
            for nf in (1, 2, 4):
                ex, lit = host_march_dir(z, *direction(az, el), DX, DX, NSTEP_TEST, z.max(), nf)
                same_exits(ex, want, "%dx%d az %g el %g nf %d" % (ni, nj, az, el, nf))
                assert_same(lit, lit_of(want), "lit %dx%d az %g el %g nf %d" % (ni, nj, az, el, nf))
    lat, lon = latlon(ni, nj)
    for ti, t in enumerate(sun_times()):
        for rot in (False, True):
            want, _ = cell_reference(ni, nj, ti, rot)
            ex, lit = host_cells(z, lat, lon, np_suntime(t), DX, DX, NSTEP_TEST, MU_MIN, z.max(), rot=rotation(ni, nj) if rot else None)
            same_exits(ex, want, "%dx%d time %s rot %d" % (ni, nj, t, rot))
            assert_same(lit.reshape(z.shape), lit_of(want), "lit %dx%d time %s rot %d" % (ni, nj, t, rot))


def test_host_ties_axes_spacing_nstep_and_nasty_operands():
    """Exact ties ax == ay in all four quadrants, gx = 0, gy = 0, both zero, dx != dy, nstep 1, and NaN / Inf / -0.0 / denormals in every
    operand one at a time."""
    ni, nj = 35, 67
    z = terrain(ni, nj)
    hmax = z.max()
    u = F(0.1)
    for gx, gy in ((0.5, 0.5), (-0.5, 0.5), (0.5, -0.5), (-0.5, -0.5), (0.0, 0.7), (0.0, -0.7), (-0.0, 0.7), (0.7, 0.0), (-0.7, 0.0), (0.7, -0.0),
                   (0.0, 0.0), (-0.0, 0.0), (0.3, 0.45), (-0.9, 0.2)):
        for dx, dy, nstep in ((DX, DX, NSTEP_TEST), (1000.0, 1500.0, NSTEP_TEST), (1500.0, 1000.0, 7), (DX, DX, 1)):
            want = np_march_dir(z, F(gx), F(gy), u, dx, dy, nstep, hmax)
            ex, lit = host_march_dir(z, F(gx), F(gy), u, dx, dy, nstep, hmax)
            same_exits(ex, want, "g (%g, %g) d (%g, %g) nstep %d" % (gx, gy, dx, dy, nstep))
            assert_same(lit, lit_of(want), "lit")
            if gx == 0 and gy == 0:
                assert (want == NO_AXIS).all()
            if abs(gx) == abs(gy) and gx != 0 and dx == dy:
                major = np_ray(F(gx), F(gy), u, dx, dy)[0]
                assert major == 1, "a tie is x-major"
    # a tie with dx != dy: ax == ay exactly
    major, d, t, rise = np_ray(F(0.5), F(0.75), u, 1000.0, 1500.0)
    assert major == 1 and t == 1 and d == 1
    r = np.random.default_rng(77)
    shape = z.shape
    gx0, gy0, u0 = (np.full(shape, v, F) for v in direction(135.0, 8.0))
    for which in ("height", "gx", "gy", "u"):
        ops = dict(height=z, gx=gx0, gy=gy0, u=u0)
        ops[which] = nasty(r, z.size).reshape(shape)
        for hm in (hmax, F(np.inf), F(np.nan)):
            want = np_march(ops["height"], *np_ray(ops["gx"], ops["gy"], ops["u"], DX, DX), NSTEP_TEST, hm)
            ex, lit = host_march_dir(ops["height"], ops["gx"], ops["gy"], ops["u"], DX, DX, NSTEP_TEST, hm)
            same_exits(ex, want, "nasty %s height_max %r" % (which, hm))
            assert_same(lit, lit_of(want), "lit, nasty %s" % which)
    lat, lon = latlon(ni, nj)
    rot = rotation(ni, nj)
    sun = np_suntime(sun_times()[1])
    for which in ("height", "lat", "lon", "cosalpha", "sinalpha"):
        ops = dict(height=z, lat=lat, lon=lon, cosalpha=rot[0], sinalpha=rot[1])
        ops[which] = nasty(r, z.size).reshape(shape)
        for mu_min in (MU_MIN, -1.0, np.nan):
            want, _ = np_cells(ops["height"], ops["lat"], ops["lon"], sun, DX, DX, NSTEP_TEST, mu_min, hmax, rot=(ops["cosalpha"], ops["sinalpha"]))
            ex, lit = host_cells(ops["height"], ops["lat"], ops["lon"], sun, DX, DX, NSTEP_TEST, mu_min, hmax, rot=(ops["cosalpha"], ops["sinalpha"]))
            same_exits(ex, want, "cells, nasty %s mu_min %r" % (which, mu_min))
            assert_same(lit.reshape(shape), lit_of(want), "cells lit, nasty %s" % which)
    # nasty sun parameters
    for bad in (np.nan, np.inf, -0.0, 1e-40):
        for k in range(3):
            s = list(sun)
            s[k] = F(bad)
            want, _ = np_cells(z, lat, lon, s, DX, DX, NSTEP_TEST, MU_MIN, hmax)
            ex, _ = host_cells(z, lat, lon, s, DX, DX, NSTEP_TEST, MU_MIN, hmax)
            same_exits(ex, want, "sun parameter %d = %r" % (k, bad))


@pytest.mark.parametrize("ni, nj", BIG)
def test_the_terrain_exercises_every_exit(ni, nj):
    """Asserted on the restatement alone: over the suns of one shape each of the four exits (shadow, over height_max, left the window,
    nstep exhausted) is taken by at least 0.5 % of the cells, and for every sun at elevation <= 8 degrees the shadowed share lies in
    [5 %, 50 %]."""
    count = np.zeros(7)
    total = 0
    for az in AZIMUTHS:
        for el in ELEVATIONS:
            ex = dir_reference(ni, nj, az, el)
            count += np.bincount(ex.ravel(), minlength=7)
            total += ex.size
            share = (ex == CAST).mean()
            print("%dx%d az %g el %g: shadowed %.1f %%" % (ni, nj, az, el, 100 * share))
            if el <= 8.0:
                assert 0.05 <= share <= 0.50, (az, el, share)
    print("exits", dict(zip(("cast", "low", "none", "left", "above", "bad_t", "nstep"), (100 * count / total).round(2))))
    for code in (CAST, ABOVE, LEFT, NSTEP):
        assert count[code] >= 0.005 * total, (code, count / total)


def test_wall():
    """A wall exactly nstep cells away shadows, at nstep + 1 it does not; a wall whose interpolated height equals the ray exactly does not
    shadow (the comparison is >), one float above it does."""
    ni, nj, nstep = 40, 3, 12
    z = np.zeros((nj, ni), F)
    z[:, 20] = 100.0
    for gx, lo, hi in ((1.0, 8, 19), (-1.0, 21, 32)):                       # rise 0.5 m per cell: the wall stands above the ray at every k <= 12
        want = np_march_dir(z, F(gx), F(0.0), F(0.5), 1.0, 1.0, nstep, 1000.0)
        ex, lit = host_march_dir(z, F(gx), F(0.0), F(0.5), 1.0, 1.0, nstep, 1000.0)
        same_exits(ex, want, "wall")
        shadowed = np.zeros((nj, ni), bool)
        shadowed[:, lo:hi + 1] = True
        assert ((ex == CAST) == shadowed).all(), "cells up to nstep away are shadowed, the cell at nstep + 1 is not"
        far = 7 if gx > 0 else 33
        assert (ex[:, far] == NSTEP).all() and (lit[:, far] == 1).all()
    # the same along j
    z = np.zeros((ni, nj), F)
    z[20, :] = 100.0
    ex, _ = host_march_dir(z, F(0.0), F(1.0), F(0.5), 1.0, 1.0, nstep, 1000.0)
    same_exits(ex, np_march_dir(z, F(0.0), F(1.0), F(0.5), 1.0, 1.0, nstep, 1000.0), "wall along j")
    assert (ex[8:20] == CAST).all() and (ex[7] == NSTEP).all() and (ex[:7] == NSTEP).all()
    # equality: t = 0.5, so at k = 1 zt = (h(m,o)*0.5) + (h(m,o+1)*0.5); ray = 0 + 1*0.5
    for top, code in ((F(1.0), NSTEP), (np.nextafter(F(1.0), F(2.0)), CAST)):
        z = np.zeros((3, 3), F)
        z[0, 1] = top
        want = np_march_dir(z, F(1.0), F(0.5), F(0.5), 1.0, 1.0, 1, 1000.0)
        ex, lit = host_march_dir(z, F(1.0), F(0.5), F(0.5), 1.0, 1.0, 1, 1000.0)
        same_exits(ex, want, "equality")
        assert ex[0, 0] == code and lit[0, 0] == (0.0 if code == CAST else 1.0), (top, ex)
    # w == 0: the second cell is never read -- a NaN there changes nothing
    z = np.zeros((3, 3), F)
    z[0, 1], z[1, 1] = 2.0, np.nan
    ex, _ = host_march_dir(z, F(1.0), F(0.0), F(0.5), 1.0, 1.0, 1, 1000.0)
    assert ex[0, 0] == CAST
    same_exits(ex, np_march_dir(z, F(1.0), F(0.0), F(0.5), 1.0, 1.0, 1, 1000.0), "w == 0")


def _cuts(ni, nj, margin):
    """The 2 x 2 decomposition: (tile slices, window slices, dst_index of the window) per part."""
    out = []
    for j0, j1 in ((0, nj // 2), (nj // 2, nj)):
        for i0, i1 in ((0, ni // 2), (ni // 2, ni)):
            wj0, wj1, wi0, wi1 = max(0, j0 - margin), min(nj, j1 + margin), max(0, i0 - margin), min(ni, i1 + margin)
            idx = np.full((wj1 - wj0, wi1 - wi0), -1, np.int32)
            idx[j0 - wj0:j1 - wj0, i0 - wi0:i1 - wi0] = np.arange((j1 - j0) * (i1 - i0), dtype=np.int32).reshape(j1 - j0, i1 - i0)
            out.append(((slice(j0, j1), slice(i0, i1)), (slice(wj0, wj1), slice(wi0, wi1)), idx))
    return out


def test_origin_independence():
    """The 70 x 130 grid cut 2 x 2 with a margin of nstep cells (none at the domain's edges) gives the whole grid's bits with the whole
    grid's height_max, restated and compiled; with margin 0 the restatement differs, because a hill stands on the cuts."""
    ni, nj = 70, 130
    z = terrain(ni, nj, True)
    lat, lon = latlon(ni, nj)
    hmax = z.max()
    for ti in (0, 1, 2):
        sun = np_suntime(sun_times()[ti])
        whole, _ = np_cells(z, lat, lon, sun, DX, DX, NSTEP_TEST, MU_MIN, hmax)
        assert 0.03 < (whole == CAST).mean() < 0.9
        differs = 0
        for margin in (NSTEP_TEST, 0):
            for tile, win, idx in _cuts(ni, nj, margin):
                ndst = int(idx.max()) + 1
                ex, _ = np_cells(z[win], lat[win], lon[win], sun, DX, DX, NSTEP_TEST, MU_MIN, hmax, dst_index=idx, ndst=ndst)
                part = ex[idx >= 0].reshape(whole[tile].shape)
                if margin:
                    same_exits(part, whole[tile], "restated part, time %d" % ti)
                    hex_, hlit = host_cells(z[win], lat[win], lon[win], sun, DX, DX, NSTEP_TEST, MU_MIN, hmax, dst_index=idx, ndst=ndst)
                    same_exits(hex_, ex, "compiled part, time %d" % ti)
                    assert_same(hlit.reshape(whole[tile].shape), lit_of(whole[tile]), "compiled part lit, time %d" % ti)
                else:
                    differs += int((lit_of(part) != lit_of(whole[tile])).sum())
        assert differs >= 1, "without a margin a shadow that crosses the cut is lost"


@pytest.mark.parametrize("ncell", ts.NCELLS_HOST)
def test_host_lit_column(ncell):
    """sw_column_lit compiled for the host: lit == 1 gives the bits of np_shortwave for every configuration and operand set; lit in
    {0, 0.25, NaN, -0.0} the restated formula; lit = 0 exactly s*kd."""
    r = np.random.default_rng(ncell)
    mixed = np.where(r.random(ncell) < 0.4, F(1.0), LITS[r.integers(0, len(LITS), ncell)]).astype(F)
    for which in ts.SETS:
        x = ts.operands(ncell, which)
        for cfg in ts.CONFIGS:
            mode, with_b, terr, ti, pi = cfg
            sun, par = np_suntime(ts.TIMES[ti]), ts.PARS[pi]
            what = "n=%d set %s cfg %s" % (ncell, which, cfg)
            assert_same(host_lit(x, np.ones(ncell, F), mode, with_b, terr, sun, par), ts.reference(ncell, which, cfg), what + " lit 1")
            want, _ = np_lit(x, mixed, mode, with_b, terr, sun, par)
            assert_same(host_lit(x, mixed, mode, with_b, terr, sun, par), want, what + " mixed lit")
            if which in ("physical", "nasty"):
                for v in LITS:
                    lit = np.full(ncell, v, F)
                    want, parts = np_lit(x, lit, mode, with_b, terr, sun, par)
                    got = host_lit(x, lit, mode, with_b, terr, sun, par)
                    assert_same(got, want, what + " lit %r" % v)
                    if v == 0 and not np.signbit(v) and which == "physical":
                        up = ~(parts["mu"] < F(par[1]))
                        with np.errstate(all="ignore"):
                            assert_same(got[up], (parts["s"] * parts["kd"]).astype(F)[up], what + ": lit 0 is s*kd")
                        assert_same(got[~up], parts["s"][~up], what + ": low sun keeps s")


def test_lit_column_flat_and_sloped_with_and_without_normals():
    """A flat floor in a cast shadow keeps its diffuse part only, with and without normals: the same bits both ways."""
    ncell = 335
    x = dict(ts.operands(ncell, "physical"))
    flat = dict(x, ne=np.zeros(ncell, F), nn=np.full(ncell, -0.0, F), nu=np.ones(ncell, F))
    sun, par = np_suntime(ts.TIMES[0]), ts.PARS[0]
    for lit in (np.zeros(ncell, F), np.full(ncell, 0.25, F)):
        a = host_lit(flat, lit, LINEAR, True, True, sun, par)
        b = host_lit(flat, lit, LINEAR, True, False, sun, par)
        assert_same(a, b, "flat normals are no normals")
        assert_same(a, np_lit(flat, lit, LINEAR, True, True, sun, par)[0], "flat, restated")
        sloped = host_lit(x, lit, LINEAR, True, True, sun, par)
        assert_same(sloped, np_lit(x, lit, LINEAR, True, True, sun, par)[0], "sloped, restated")
        assert (sloped != a).mean() > 0.2 or lit[0] == 0


def test_bindings_regenerate_identically_with_the_shadow_calls():
    from tools import gen_abi
    for rel, text in (("include/noahmp_hip.h", gen_abi.c_header()), ("oracle/ref_harness_gen.f90", gen_abi.ref_harness()),
                      ("noahmp_amd/fortran/module_sf_noahmpdrv_hip.F90", gen_abi.fortran_shim()),
                      ("tests/fortran/shim_wrap_gen.f90", gen_abi.shim_wrap())):
        assert open(os.path.join(ROOT, rel)).read() == text, rel
    hdr = open(os.path.join(ROOT, "include", "noahmp_hip.h")).read()
    for word in ("typedef struct noahmp_shadow {", "} noahmp_shadow;", "#define NOAHMP_HIP_HAS_FORCING_SHADOW 1\n", "#define NOAHMP_HIP_ABI_MINOR 3\n",
                 "noahmp_hip_forcing_shadow(const noahmp_shadow* sh, int64_t ndst, const noahmp_sun_time* now, void* stream);",
                 "noahmp_hip_forcing_shortwave_lit(const noahmp_shortwave* sw, const float* lit, int64_t ncell, const noahmp_sun_time* now,",
                 "minor is unchanged; announced by the macro and the symbols", "Earth curvature and atmospheric", "refraction are neglected, as in WRF",
                 "gx = (e*ca) + (n*sa)", "gy = (n*ca) - (e*sa)", "rise = u / a", "ray = z0 + (kf*rise)", "fo = kf*t", "jo = floorf(fo);  w = fo - jo",
                 "zt = (height(m,o)*(1.0f - w)) + (height(m,o+1)*w)", "If zt > ray: lit = +0.0f", "r  = r0*lit[c]", "s  = s * (kd + ((1.0f - kd)*r))",
                 "margin is at least nstep cells"):
        assert word in hdr, word
    assert "noahmp_shadow" not in gen_abi.ref_harness()
    f90 = open(os.path.join(ROOT, "noahmp_amd", "fortran", "module_sf_noahmpdrv_hip.F90")).read()
    for word in ("bind(C, name='noahmp_hip_forcing_shadow')", "bind(C, name='noahmp_hip_forcing_shortwave_lit')", "type, bind(C) :: noahmp_shadow"):
        assert word in f90, word
    assert "noahmp_hip_forcing_shadow" in abi.EXPORTED_SYMBOLS and "noahmp_hip_forcing_shortwave_lit" in abi.EXPORTED_SYMBOLS
    assert [n for n, _ in abi.Shadow._fields_] == ["height", "xlat", "lon", "cosalpha", "sinalpha", "dst_index", "lit", "ni", "nj", "nstep", "dx", "dy",
                                                   "mu_min", "height_max"]


def test_ctypes_mirror_matches_the_compiled_header(tmp_path):
    names = [n for n, _ in abi.Shadow._fields_]
    body = 'printf(" %zu", sizeof(noahmp_shadow));' + "".join('printf(" %%zu", offsetof(noahmp_shadow, %s));' % n for n in names)
    body += 'printf(" %zu", sizeof(noahmp_shortwave));'
    want = [C.sizeof(abi.Shadow)] + [getattr(abi.Shadow, n).offset for n in names] + [C.sizeof(abi.Shortwave)]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "noahmp_hip.h"\nint main(){' + body +
                   'printf(" %d %d %d", NOAHMP_HIP_ABI_MINOR, NOAHMP_HIP_HAS_FORCING_SHADOW, NOAHMP_SHADOW_MAX_NSTEP); return 0;}')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert out == want + [3, 1, 4096]


def test_library_exports_the_shadow_calls():
    if not os.path.exists(abi.LIB_PATH):
        from noahmp_amd import build as b
        b.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", abi.LIB_PATH]).decode()
    assert " T noahmp_hip_forcing_shadow\n" in out and " T noahmp_hip_forcing_shortwave_lit\n" in out


@pytest.mark.skipif(tr._flang() is None, reason="no flang")
def test_generated_fortran_types_and_interfaces_compile(tmp_path):
    """The shadow part of the generated module compiles on top of the shortwave part, and a caller of both interfaces type-checks."""
    from tools import gen_abi
    text = "\n".join(["module shadow_abi_check", "  use iso_c_binding", "  implicit none"] + gen_abi.shortwave_f90_types() + gen_abi.shadow_f90_types() +
                     ["  interface"] + gen_abi.shortwave_f90_interfaces() + gen_abi.shadow_f90_interfaces() +
                     ["  end interface", "contains", "  function go(ncell, planes, sw) result(rc)", "    integer(c_int64_t), value :: ncell",
                      "    type(c_ptr), intent(in) :: planes(5)", "    type(noahmp_shortwave), intent(in) :: sw", "    type(noahmp_shadow) :: sh",
                      "    type(noahmp_sun_time) :: t", "    integer(c_int) :: rc", "    t%iday = 355; t%ihour = 22; t%iminute = 30; t%isecond = 0",
                      "    sh%height = planes(1); sh%xlat = planes(2); sh%lon = planes(3); sh%cosalpha = c_null_ptr; sh%sinalpha = c_null_ptr",
                      "    sh%dst_index = planes(4); sh%lit = planes(5); sh%ni = 64; sh%nj = 8; sh%nstep = min(25, NOAHMP_SHADOW_MAX_NSTEP)",
                      "    sh%dx = 1000.0; sh%dy = 1000.0; sh%mu_min = 0.05; sh%height_max = 4400.0",
                      "    rc = noahmp_hip_forcing_shadow(sh, ncell, t, c_null_ptr)",
                      "    rc = noahmp_hip_forcing_shortwave_lit(sw, planes(5), ncell, t, c_null_ptr)",
                      "  end function go", "end module shadow_abi_check", ""])
    f = tmp_path / "shadow_abi_check.f90"
    f.write_text(text)
    subprocess.check_call([tr._flang(), "-c", str(f), "-o", str(tmp_path / "shadow_abi_check.o"), "-J", str(tmp_path)], cwd=str(tmp_path))


# ---------------------------------------------------------------------------------------------------------------- GPU
_dev = tr._dev


def _indices(ni, nj):
    """(name, dst_index or None, ndst): identity, a random permutation, and a window whose outer ring (and a few cells >= ndst) is not
    written -- those keep their own positions, so the ring's positions must keep the poison."""
    ncell = ni * nj
    r = np.random.default_rng(ni * 1000 + nj)
    ring = np.arange(ncell, dtype=np.int32).reshape(nj, ni)
    m = 2 if min(ni, nj) > 8 else (1 if min(ni, nj) > 2 else 0)
    if m:
        inner = ring[m:-m, m:-m].copy()
        ring[...] = -1
        ring[m:-m, m:-m] = inner
        ring[0, 0] = ncell                       # >= ndst: not written either
        ring[-1, -1] = 2 ** 31 - 1
    return [("identity", None, ncell), ("permutation", r.permutation(ncell).astype(np.int32).reshape(nj, ni), ncell), ("margin", ring, ncell)]


@pytest.mark.gpu
@pytest.mark.parametrize("ni, nj", WINDOWS_GPU)
def test_gpu_shadow_kernel_equals_the_restatement(engine, ni, nj):
    """noahmp_hip_forcing_shadow against np_cells: three low suns, noon and night; identity, permuted and margin dst_index; with rotation
    planes at one sun.  35 x 67 = 2345 cells end in a ragged workgroup and a ragged wave.  Destinations are offset by one float inside a
    poisoned pool; guard words and the positions of unwritten cells keep the poison."""
    import torch
    ncell = ni * nj
    z = terrain(ni, nj)
    lat, lon = latlon(ni, nj)
    rot = rotation(ni, nj)
    zd, latd, lond, cad, sad = (_dev(v) for v in (z, lat, lon, rot[0], rot[1]))
    pool = torch.full((ncell + 9,), POISON, dtype=torch.float32, device="cuda")
    dst = pool[5:5 + ncell]
    torch.cuda.synchronize()
    shares = []
    for ti, t in enumerate(sun_times()):
        for use_rot in ((False, True) if ti == 1 else (False,)):
            want_ex, mu = cell_reference(ni, nj, ti, use_rot)
            shares.append(((want_ex == CAST).mean(), (want_ex == LOW_SUN).mean()))
            for name, idx, ndst in _indices(ni, nj):
                idxd = _dev(idx) if idx is not None else None
                pool.fill_(POISON)
                torch.cuda.synchronize()
                b = engine.shadow_block(zd, latd, lond, dst, DX, DX, nstep=NSTEP_TEST, cosalpha=cad if use_rot else None, sinalpha=sad if use_rot else None,
                                        dst_index=idxd, mu_min=MU_MIN, height_max=float(z.max()))
                engine.forcing_shadow(b, ndst, t)
                engine.stream_sync()
                h = pool.cpu().numpy()
                what = "%dx%d time %s rot %d index %s" % (ni, nj, t, use_rot, name)
                want = np.full(ncell, POISON, F)
                flat_idx = np.arange(ncell) if idx is None else idx.ravel().astype(np.int64)
                ok = (flat_idx >= 0) & (flat_idx < ndst)
                want[flat_idx[ok]] = lit_of(want_ex).ravel()[ok]
                assert_same(h[5:5 + ncell], want, what)
                assert (h[:5] == POISON).all() and (h[5 + ncell:] == POISON).all(), what + ": guard words"
                if name == "margin" and not ok.all():
                    assert (h[5:5 + ncell][~ok] == POISON).all(), what + ": unwritten cells keep the poison"
    if ncell > 2000:
        assert any(0.05 < c < 0.9 for c, _ in shares[:3]), shares
        assert shares[-1][1] == 1.0 and shares[-2][0] < 0.05, "night is not marched; at noon nearly nothing is shadowed"


@pytest.mark.gpu
@pytest.mark.parametrize("ncell", ts.NCELLS_GPU)
def test_gpu_lit_kernel_equals_the_restatement(engine, ncell):
    """noahmp_hip_forcing_shortwave_lit against np_lit over every configuration and operand set, with a mixed lit plane (1, 0, 0.25, NaN,
    -0.0); with an all-ones plane it equals what noahmp_hip_forcing_shortwave writes in the same test."""
    import torch
    r = np.random.default_rng(50 + ncell)
    mixed = np.where(r.random(ncell) < 0.4, F(1.0), LITS[r.integers(0, len(LITS), ncell)]).astype(F)
    mixed_d, ones_d = _dev(mixed), _dev(np.ones(ncell, F))
    pool = torch.full((3, ncell + 9), POISON, dtype=torch.float32, device="cuda")
    dsts = [pool[k, 5:5 + ncell] for k in range(3)]
    for which in ts.SETS:
        x = ts.operands(ncell, which)
        xd = {k: _dev(v) for k, v in x.items()}
        torch.cuda.synchronize()
        for cfg in ts.CONFIGS:
            mode, with_b, terr, ti, pi = cfg
            pool.fill_(POISON)
            torch.cuda.synchronize()
            blocks = [ts._block(engine, xd, d, mode, with_b, terr, ts.PARS[pi]) for d in dsts]
            engine.forcing_shortwave_lit(blocks[0], mixed_d, ncell, ts.TIMES[ti])
            engine.forcing_shortwave_lit(blocks[1], ones_d, ncell, ts.TIMES[ti])
            engine.forcing_shortwave(blocks[2], ncell, ts.TIMES[ti])
            engine.stream_sync()
            h = pool.cpu().numpy()
            what = "ncell %d set %s cfg %s" % (ncell, which, cfg)
            want, _ = np_lit(x, mixed, mode, with_b, terr, np_suntime(ts.TIMES[ti]), ts.PARS[pi])
            assert_same(h[0, 5:5 + ncell], want, what + " mixed lit")
            assert_same(h[1, 5:5 + ncell], h[2, 5:5 + ncell], what + ": all ones is the unshaded call")
            assert_same(h[2, 5:5 + ncell], ts.reference(ncell, which, cfg), what + ": the unshaded call")
            assert (h[:, :5] == POISON).all() and (h[:, 5 + ncell:] == POISON).all(), what + ": guard words"


@pytest.mark.gpu
def test_gpu_refusals_launch_nothing(engine):
    """Every refusal returns -105 with text, the destinations keep their poison, and the same blocks are served afterwards."""
    import torch
    lib = engine.lib
    ni, nj = 35, 67
    ncell = ni * nj
    z = terrain(ni, nj)
    lat, lon = latlon(ni, nj)
    rot = rotation(ni, nj)
    zd, latd, lond, cad, sad = (_dev(v) for v in (z, lat, lon, rot[0], rot[1]))
    dst = torch.full((2, ncell), POISON, dtype=torch.float32, device="cuda")
    x = ts.operands(256, "physical")
    xd = {k: _dev(v) for k, v in x.items()}
    ones = _dev(np.ones(256, F))
    torch.cuda.synchronize()
    t = sun_times()[1]
    now = engine.sun_times([t])

    def blk(**kw):
        b = engine.shadow_block(zd, latd, lond, dst[0], DX, DX, nstep=NSTEP_TEST, cosalpha=cad, sinalpha=sad, mu_min=MU_MIN, height_max=float(z.max()))
        for k, v in kw.items():
            setattr(b, k, v)
        return b

    def call(b, ndst=ncell, when=now):
        rc = lib.noahmp_hip_forcing_shadow(C.byref(b) if b is not None else None, ndst, when, None)
        engine.stream_sync()
        return rc, lib.noahmp_hip_last_error().decode()
    for field in ("height", "xlat", "lon", "lit"):
        rc, msg = call(blk(**{field: None}))
        assert rc == -105 and "required" in msg, (field, rc, msg)
    for field in ("cosalpha", "sinalpha"):
        rc, msg = call(blk(**{field: None}))
        assert rc == -105 and "both or none" in msg, (field, rc, msg)
    for kw, word in ((dict(nstep=0), "nstep"), (dict(nstep=4097), "nstep"), (dict(nstep=-3), "nstep"), (dict(dx=0.0), "dx"), (dict(dx=-1.0), "dx"),
                     (dict(dx=float("nan")), "dx"), (dict(dy=float("inf")), "dy"), (dict(dy=0.0), "dy"), (dict(ni=-1), "ni"), (dict(nj=-1), "nj"),
                     (dict(ni=65536, nj=32768), "ni")):
        rc, msg = call(blk(**kw))
        assert rc == -105 and word in msg, (kw, rc, msg)
    for ndst in (-1, 2 ** 31):
        rc, msg = call(blk(), ndst=ndst)
        assert rc == -105 and "ndst" in msg, (ndst, rc, msg)
    rc, msg = call(blk(), when=None)
    assert rc == -105 and "now" in msg
    rc, msg = call(None)
    assert rc == -105 and "NULL" in msg
    # the lit call: a NULL plane, and the refusals of the unshaded call
    swb = ts._block(engine, xd, dst[1][:256], ZENITH, False, True, ts.PARS[0])

    def lit_call(b, lit=ones.data_ptr(), nc=256, when=now):
        rc = lib.noahmp_hip_forcing_shortwave_lit(C.byref(b) if b is not None else None, lit, nc, when, None)
        engine.stream_sync()
        return rc, lib.noahmp_hip_last_error().decode()
    rc, msg = lit_call(swb, lit=None)
    assert rc == -105 and "lit" in msg
    rc, msg = lit_call(None)
    assert rc == -105 and "NULL" in msg
    rc, msg = lit_call(swb, when=None)
    assert rc == -105 and "now" in msg
    rc, msg = lit_call(swb, nc=-1)
    assert rc == -105 and "columns" in msg
    for field, word in (("sw_a", "required"), ("swdown", "required"), ("mean_a", "mean_a"), ("normal_n", "all three or none")):
        b = ts._block(engine, xd, dst[1][:256], ZENITH, False, True, ts.PARS[0])
        setattr(b, field, None)
        rc, msg = lit_call(b)
        assert rc == -105 and word in msg, (field, rc, msg)
    b = ts._block(engine, xd, dst[1][:256], ZENITH, False, True, ts.PARS[0])
    b.mode = 2
    rc, msg = lit_call(b)
    assert rc == -105 and "mode" in msg
    assert (dst.cpu().numpy() == POISON).all()
    # empty calls return 0 and write nothing
    assert call(blk(), ndst=0)[0] == 0 and call(blk(ni=0))[0] == 0 and call(blk(nj=0))[0] == 0 and lit_call(swb, nc=0)[0] == 0
    assert (dst.cpu().numpy() == POISON).all()
    # the same blocks are served afterwards
    rc, msg = call(blk())
    assert rc == 0, msg
    rc, msg = lit_call(swb)
    assert rc == 0, msg
    h = dst.cpu().numpy()
    assert_same(h[0], lit_of(cell_reference(ni, nj, 1, True)[0]).ravel(), "after the refusals")
    assert_same(h[1][:256], np_shortwave(x, ZENITH, False, True, np_suntime(t), ts.PARS[0]), "after the refusals, the lit call")
    assert (h[1][256:] == POISON).all()


@pytest.mark.gpu
def test_gpu_chain_with_cast_shadows(engine, tables):
    """forcing_interpolate_prep, Shortwave.apply with set_shadow (ZENITH with terrain normals, a window with a margin), noahmplsm for two
    steps: the store's SWDOWN equals the restatement fed with the restated lit plane; the sorted store after follow() holds the tile-order
    result permuted; with every=2 the second step reuses the first step's plane."""
    import torch
    from noahmp_amd import shortwave as swmod
    from noahmp_amd.shortwave import Shortwave
    NI, NJ, MARGIN = ts.CHAIN_NI, ts.CHAIN_NJ, 3
    r = np.random.default_rng(31)
    recs_h = [{k: r.uniform(lo, hi, (NJ, NI)).astype(F) for k, (lo, hi) in tr.COARSE.items()} for _ in range(2)]
    recs = [{k: _dev(v) for k, v in rec.items()} for rec in recs_h]
    # a window with a margin of 3 cells along j and none along i; ridges across the tile, the sun low in the west over its western part
    jj, ii = np.meshgrid(np.arange(NJ + 2 * MARGIN), np.arange(NI), indexing="ij")
    height = (900.0 + 700.0 * np.sin(ii * 0.9) * np.cos(jj * 0.7)).astype(F)
    dx = dy = 1000.0
    nstep = 5
    par = dict(max_ratio=10.0, mu_min=0.05, max_terrain_ratio=5.0, solar_constant=1361.0)
    parv = (10.0, 0.05, 5.0, 1361.0)
    start = ts.CHAIN_START
    steps = [(171, 18, 30 * (it - 1), 0) for it in (1, 2)]                       # at 18 UTC the terminator crosses the tile: a low sun west of it
    nsample = 6
    sample_suns = [np_suntime(t[1:]) for t in swmod.sample_times(start, 10800, nsample)]
    heightd = _dev(height)

    class Device:
        def __init__(self, every):
            self.every = every

        def start(self, d, perm):
            self.sw = Shortwave(engine, _dev(ts.CHAIN_LAT), _dev(ts.CHAIN_LON), mode="zenith", **par)
            self.sw.terrain_from_height(heightd[MARGIN:MARGIN + NJ], dx, dy)
            self.sw.set_shadow(heightd, dx, dy, nstep=nstep, origin=(0, MARGIN), every=self.every)
            if perm is not None:
                self.sw.follow(d)
            self.sw.interval(start, 10800, nsample)
            self.planes = []

        def __call__(self, d, it, ra, rb, now):
            self.sw.apply(d, ra, rb, 1800 * (it - 1), 10800, steps[it - 1])
            engine.stream_sync()
            self.planes.append(d.a["swdown"].cpu().numpy().ravel().copy())
            self.lits = getattr(self, "lits", []) + [self.sw.lit.cpu().numpy().ravel().copy()]

    def chain(feed, sort=False):
        return ts._sw_chain(engine, tables, recs, feed, sort=sort)
    dev = Device(1)
    chain(dev)
    normal = [t.cpu().numpy().ravel() for t in dev.sw.normal_tile]
    mean_h = ts.np_mean(ts.CHAIN_LAT.ravel(), ts.CHAIN_LON.ravel(), sample_suns)
    x = dict(sw_a=recs_h[0]["sw"].ravel(), sw_b=recs_h[1]["sw"].ravel(), mean_a=mean_h, lat=ts.CHAIN_LAT.ravel(), lon=ts.CHAIN_LON.ravel(),
             ne=normal[0], nn=normal[1], nu=normal[2])
    latw, lonw = np.zeros_like(height), np.zeros_like(height)
    latw[MARGIN:MARGIN + NJ], lonw[MARGIN:MARGIN + NJ] = ts.CHAIN_LAT, ts.CHAIN_LON
    idx = np.full(height.shape, -1, np.int32)
    idx[MARGIN:MARGIN + NJ] = np.arange(NI * NJ, dtype=np.int32).reshape(NJ, NI)
    lits, planes = [], []
    for t in steps:
        ex, _ = np_cells(height, latw, lonw, np_suntime(t), dx, dy, nstep, 0.05, height.max(), dst_index=idx, ndst=NI * NJ)
        lits.append(lit_of(ex[MARGIN:MARGIN + NJ]).ravel())
        planes.append(np_lit(x, lits[-1], ZENITH, False, True, np_suntime(t), parv)[0])
    assert all(20 < (l == 0).sum() < l.size - 20 for l in lits), [(l == 0).sum() for l in lits]
    assert (lits[0] != lits[1]).any(), "the shadows move between the steps"
    unshaded = np_shortwave(x, ZENITH, False, True, np_suntime(steps[1]), parv)
    assert (unshaded != planes[1]).sum() > 20
    for it in (0, 1):
        assert_same(dev.lits[it], lits[it], "the lit plane of step %d" % (it + 1))
        assert_same(dev.planes[it], planes[it], "SWDOWN of step %d" % (it + 1))
    # the sorted layout: the same columns at other positions
    devs = Device(1)
    ds, _ = chain(devs, sort=True)
    perm = ds.sort_perm.cpu().numpy()
    assert (perm != np.arange(perm.size)).any()
    for it in (0, 1):
        assert_same(devs.lits[it], lits[it][perm], "the lit plane of the sorted chain, step %d" % (it + 1))
        assert_same(devs.planes[it], planes[it][perm], "SWDOWN of the sorted chain, step %d" % (it + 1))
    # every = 2: the second step reuses the first plane
    dev2 = Device(2)
    chain(dev2)
    assert_same(dev2.lits[1], lits[0], "every = 2: the plane of step 1 at step 2")
    assert_same(dev2.planes[1], np_lit(x, lits[0], ZENITH, False, True, np_suntime(steps[1]), parv)[0], "every = 2: SWDOWN of step 2")
    # without set_shadow nothing changes
    plain = Shortwave(engine, _dev(ts.CHAIN_LAT), _dev(ts.CHAIN_LON), mode="zenith", **par)
    assert plain.shadow is None and plain.lit is None
    torch.cuda.synchronize()
