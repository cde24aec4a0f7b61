"""Sky-view factor in the radiation forcing: the horizon scan and the per-step radiation call (noahmp_hip_skyview,
noahmp_hip_forcing_radiation_sky; nmp_dev_skyview.hpp, nmp_dev_shortwave.hpp).

No reference routine stands behind the calls; the contract is the text in include/noahmp_hip.h.  np_sky_scan, np_skyview and
np_radiation_sky restate it in numpy float32, one rounded operation per line, on top of test_shadow's np_ray / np_lit and test_shortwave's
np_sun / np_kd.  Everything is compared with the restatement bit for bit (test_regrid.assert_same: equal bits, or both NaN): the per-cell
functions compiled for the host with 1, 2 and 4 steps in flight, both kernels, and two engine steps through Shortwave.set_shadow /
set_skyview / apply.  A tolerance appears in the two analytic checks only (a tilted plane, a cone pit); where it comes from is said there."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from noahmp_amd import abi
import test_regrid as tr
import test_shadow as tsh
import test_shortwave as ts
from test_regrid import F, assert_same, nasty
from test_shadow import np_lit, np_ray
from test_shortwave import LINEAR, ZENITH, max0, min_, np_sun, np_suntime

ROOT = tr.ROOT
CSRC = tr.CSRC
SRC = os.path.join(ROOT, "tests", "host_emul", "skyview_check.hip")
LIB = os.path.join(ROOT, "tests", "host_emul", "libskyview_check.so")
WINDOWS = tsh.WINDOWS
WINDOWS_GPU = [(1, 1), (5, 3), (35, 67), (70, 130)]
NSTEP_TEST = 12
NDIRS = (1, 4, 8, 16, 64)
NDIRS_GPU = (1, 8, 16, 64)
DX, DY = 1000.0, 1500.0                                                  # dx != dy
POISON = 7.0
ONE = np.array([1.0], F).view(np.uint32)[0]                              # 0x3F800000
EPS = 2.0 ** -24
SIGMA = 5.67e-8


# ---------------------------------------------------------------------------------------------------------------- the restatement
def directions(ndir):
    """(float32) sin / cos (2 pi q / ndir), made in float64: the table of the Python layer."""
    a = 2.0 * np.pi * np.arange(ndir, dtype=np.float64) / ndir
    return np.sin(a).astype(F), np.cos(a).astype(F)


def np_sky_scan(height, gx, gy, dx, dy, nstep):
    """One direction of the header text over a window: smax of every cell, and (major, L2) of the direction."""
    height = np.asarray(height, F)
    nj, ni = height.shape
    major, d, t, _ = np_ray(F(gx), F(gy), F(0.0), dx, dy)
    major, d, t = int(major), int(d), F(t)
    smax = np.zeros((nj, ni), F)
    if major == 0:
        return smax, 0, F(0.0)
    xm = major == 1
    sp, so = (F(dx), F(dy)) if xm else (F(dy), F(dx))
    with np.errstate(all="ignore"):
        td = F(t * so)
        td2 = F(td * td)
        sp2 = F(sp * sp)
        L2 = F(sp2 + td2)
    jj, ii = np.meshgrid(np.arange(nj, dtype=np.int64), np.arange(ni, dtype=np.int64), indexing="ij")
    pos_m, pos_o = (ii, jj) if xm else (jj, ii)
    M, O = (ni, nj) if xm else (nj, ni)
    live = np.ones((nj, ni), bool)
    with np.errstate(all="ignore"):
        for k in range(1, int(nstep) + 1):
            kf = F(k)
            m = pos_m + k * d
            live &= (m >= 0) & (m <= M - 1)
            fo = F(kf * t)
            if not (fo >= -kf and fo <= kf):
                break
            jo = np.floor(fo)
            w = F(fo - jo)
            o = pos_o + int(jo)
            live &= (o >= 0) & (o <= O - 1)
            one = w == 0
            if not one:
                live &= o + 1 <= O - 1
            if not live.any():
                break
            mc, oc = np.where(live, m, 0), np.where(live, o, 0)
            h0 = height[(oc, mc) if xm else (mc, oc)]
            if one:
                zt = h0
            else:
                o1 = np.where(live, o + 1, 0)
                h1 = height[(o1, mc) if xm else (mc, o1)]
                zt = ((h0 * F(F(1.0) - w)) + (h1 * w)).astype(F)
            dz = (zt - height).astype(F)
            s = (dz / kf).astype(F)
            up = live & (s > smax)
            smax[up] = s[up]
    return smax, major, L2


def np_skyview(height, dir_x, dir_y, dx, dy, nstep, dst_index=None, ndst=None):
    """noahmp_hip_skyview over a window: svf in WINDOW order, smax per direction, and the mask of the written cells."""
    height = np.asarray(height, F)
    ncell = height.size
    idx = np.arange(ncell).reshape(height.shape) if dst_index is None else np.asarray(dst_index).reshape(height.shape)
    todo = (idx >= 0) & (idx < (ncell if ndst is None else ndst))
    acc = np.zeros(height.shape, F)
    smaxes = []
    with np.errstate(all="ignore"):
        for gx, gy in zip(dir_x, dir_y):
            smax, major, L2 = np_sky_scan(height, gx, gy, dx, dy, nstep)
            smaxes.append(smax)
            if major == 0:
                term = np.ones(height.shape, F)
            else:
                s2 = smax * smax
                den = L2 + s2
                term = np.where(smax == 0, F(1.0), L2 / den).astype(F)
            acc = (acc + term).astype(F)
        svf = (acc / F(len(dir_x))).astype(F)
    return svf, np.array(smaxes, F).reshape((len(dir_x),) + height.shape), todo


def np_radiation_sky(x, svf, lit, albedo, glw, tsurf, emiss, sigma, mode, with_b, terrain, sun, par):
    """noahmp_hip_forcing_radiation_sky over the operand dict x (test_shortwave.OPERANDS): (swdown, glw or None).  lit None = 1; albedo and
    emiss are planes or constants."""
    max_ratio, mu_min, max_tr, s0 = (F(v) for v in par)
    v = np.asarray(svf, F)
    n = v.size
    l = np.ones(n, F) if lit is None else np.asarray(lit, F)
    al = np.broadcast_to(np.asarray(albedo, F), (n,))
    a = {k: np.asarray(q, F) for k, q in x.items()}
    base, parts = np_lit(x, l, mode, with_b, terrain, sun, par)
    s, kd, mu = parts["s"], parts["kd"], parts["mu"]
    e, nn_, u = np_sun(a["lat"], a["lon"], sun)
    with np.errstate(all="ignore"):
        r0 = np.ones(n, F)
        if terrain:
            pe = e * a["ne"]
            pn = nn_ * a["nn"]
            pu = u * a["nu"]
            pen = pe + pn
            cosi = pen + pu
            rr = max0(cosi) / mu
            flat = (a["ne"] == 0) & (a["nn"] == 0)
            r0 = np.where(flat, F(1.0), min_(rr, max_tr)).astype(F)
        r = r0 * l
        dif = kd * v
        beam = F(1.0) - kd
        br = beam * r
        f0 = np.where(mu < mu_min, v, dif + br).astype(F)
        o = F(1.0) - v
        refl = al * o
        f = f0 + refl
        out = (s * f).astype(F)
        sw = np.where(v == F(1.0), base, out).astype(F)
        if glw is None:
            return sw, None
        g, T = np.asarray(glw, F), np.asarray(tsurf, F)
        em = np.broadcast_to(np.asarray(emiss, F), (n,))
        t2 = T * T
        t4 = t2 * t2
        b = F(sigma) * t4
        eb = em * b
        upw = o * eb
        dn = v * g
        lw = np.where(v == F(1.0), g, dn + upw).astype(F)
    return sw, lw


# ---------------------------------------------------------------------------------------------------------------- the inputs
def hand_table():
    """A zero vector, a NaN, axis-parallel directions of both signs, the exact diagonal ax == ay for dx != dy (both signs), and two
    ordinary directions."""
    gx = np.array([0.0, np.nan, 1.0, -1.0, 0.0, -0.0, DX / 2000.0, -DX / 2000.0, 0.3, -0.9, 0.5], F)
    gy = np.array([-0.0, 0.5, 0.0, -0.0, 1.0, -1.0, DY / 2000.0, DY / 2000.0, 0.45, 0.2, np.nan], F)
    return gx, gy


@functools.lru_cache(maxsize=None)
def scan_reference(ni, nj, ndir, kind="hills"):
    """(svf, smax, todo) of the restatement; kind: hills = test_shadow.terrain, nasty = the same with NaN / Inf / denormal words, hand =
    the hand-made table on the hills."""
    z = terrain_of(ni, nj, kind)
    dxs = hand_table() if kind == "hand" else directions(ndir)
    out = np_skyview(z, dxs[0], dxs[1], DX, DY, NSTEP_TEST)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def terrain_of(ni, nj, kind="hills"):
    z = tsh.terrain(ni, nj)
    if kind == "nasty":
        r = np.random.default_rng(ni * 7 + nj)
        bad = nasty(r, z.size).reshape(z.shape)
        z = np.where(r.random(z.shape) < 0.15, bad, z).astype(F)
        z.setflags(write=False)
    return z


def sky_planes(ncell, which):
    """svf (1.0 in about a third of the columns), lit, albedo, glw, tsurf, emiss of ncell columns: physical, nasty, or mixed."""
    r = np.random.default_rng(900 + ncell + len(which))
    phys = dict(svf=np.where(r.random(ncell) < 0.35, F(1.0), r.uniform(0.3, 1.0, ncell)).astype(F),
                lit=np.where(r.random(ncell) < 0.4, F(1.0), tsh.LITS[r.integers(0, len(tsh.LITS), ncell)]).astype(F),
                albedo=r.uniform(0.05, 0.9, ncell).astype(F), glw=r.uniform(150.0, 450.0, ncell).astype(F),
                tsurf=r.uniform(230.0, 320.0, ncell).astype(F), emiss=r.uniform(0.85, 1.0, ncell).astype(F))
    if which == "physical":
        return phys
    nas = {k: nasty(r, ncell) for k in phys}
    nas["svf"] = np.where(r.random(ncell) < 0.2, F(1.0), nas["svf"]).astype(F)
    if which == "nasty":
        return nas
    pick = {k: r.random(ncell) < 0.5 for k in phys}
    return {k: np.where(pick[k], phys[k], nas[k]).astype(F) for k in phys}


def sky_options():
    """(lit, albedo plane, glw, emiss plane): every combination of the optional planes."""
    return [(a, b, c, d) for a in (False, True) for b in (False, True) for c in (False, True) for d in (False, True) if c or not d]


ALBEDO_CONST, EMISS_CONST = 0.23, 0.96


def restated_radiation(x, y, opt, cfg):
    mode, with_b, terr, ti, pi = cfg
    use_lit, use_alb, use_glw, use_em = opt
    return np_radiation_sky(x, y["svf"], y["lit"] if use_lit else None, y["albedo"] if use_alb else ALBEDO_CONST, y["glw"] if use_glw else None,
                            y["tsurf"], y["emiss"] if use_em else EMISS_CONST, SIGMA, mode, with_b, terr, np_suntime(ts.TIMES[ti]), ts.PARS[pi])


# ---------------------------------------------------------------------------------------------------------------- CPU
def build():
    deps = [SRC, os.path.join(CSRC, "nmp_dev_skyview.hpp"), os.path.join(CSRC, "nmp_dev_shadow.hpp"), os.path.join(CSRC, "nmp_dev_shortwave.hpp"),
            os.path.join(CSRC, "nmp_dev_forcing.hpp"), os.path.join(CSRC, "nmp_libm.hpp"), os.path.join(CSRC, "nmp_libm_tables.inc"),
            os.path.join(ROOT, "include", "noahmp_hip.h")]
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
    lib.skyview_cells.argtypes = [I, I, V, V, C.c_long, I, I, V, V, Fl, Fl, I, V, V]
    lib.skyview_radiation_values.argtypes = [C.c_long] + [V] * 15 + [I] + [Fl] * 5 + [V, V]
    lib.skyview_cells.restype = lib.skyview_radiation_values.restype = None
    return lib


_p = ts._p


def _c(a, dtype=F):
    return np.ascontiguousarray(a, dtype)


def host_skyview(height, dir_x, dir_y, dx, dy, nstep, nf, dst_index=None, ndst=None):
    height = _c(height)
    nj, ni = height.shape
    ndst = height.size if ndst is None else ndst
    dir_x, dir_y = _c(dir_x), _c(dir_y)
    smax = np.full((dir_x.size, nj, ni), POISON, F)
    svf = np.full(max(ndst, 1), POISON, F)
    idx = _c(dst_index, np.int32) if dst_index is not None else None
    _host().skyview_cells(ni, nj, _p(height), _p(idx), ndst, int(nstep), dir_x.size, _p(dir_x), _p(dir_y), float(dx), float(dy), nf, _p(smax), _p(svf))
    return svf[:ndst], smax


def host_radiation(x, y, opt, cfg, idts=ts.IDTS, idts2=ts.IDTS2):
    mode, with_b, terr, ti, pi = cfg
    use_lit, use_alb, use_glw, use_em = opt
    sun, par = np_suntime(ts.TIMES[ti]), ts.PARS[pi]
    n = x["sw_a"].size
    fraction = F(idts2 - idts) / F(idts2) if (mode == LINEAR and with_b) else F(1.0)
    one_minus = F(1.0) - fraction
    out = np.full(n, POISON, F)
    parv, skyv = np.array(par, F), np.array([ALBEDO_CONST, EMISS_CONST, SIGMA], F)
    a = {k: _c(v) for k, v in x.items()}
    b = {k: _c(v).copy() for k, v in y.items()}
    _host().skyview_radiation_values(n, _p(b["svf"]), _p(b["lit"]) if use_lit else None, _p(b["albedo"]) if use_alb else None,
                                     _p(b["glw"]) if use_glw else None, _p(b["tsurf"]), _p(b["emiss"]) if use_em else None, _p(skyv), _p(a["sw_a"]),
                                     _p(a["sw_b"]) if with_b else None, _p(a["mean_a"]) if mode == ZENITH else None, _p(a["lat"]), _p(a["lon"]),
                                     *[(_p(a[k]) if terr else None) for k in ("ne", "nn", "nu")], mode, float(fraction), float(one_minus),
                                     float(sun[0]), float(sun[1]), float(sun[2]), _p(parv), _p(out))
    return out, b["glw"]


def _check_window(svf, smax, want, what):
    wsvf, wsmax, todo = want
    for q in range(wsmax.shape[0]):
        assert_same(smax[q][todo], wsmax[q][todo], what + ": smax of direction %d" % q)
        assert (smax[q][~todo] == POISON).all(), what + ": a cell that is not scanned"
    return wsvf


@pytest.mark.parametrize("ni, nj", WINDOWS)
def test_host_scan_equals_the_restatement(ni, nj):
    """sky_dir / sky_scan / sky_cell compiled for the host against np_skyview: per-direction smax and the factor, for ndir 1 .. 64, 1, 2 and
    4 steps in flight, dx != dy, the hand-made table (zero, NaN, axis-parallel, the exact diagonal), terrain with NaN / Inf / denormal
    words, and a dst_index with margin cells and a permutation."""
    cases = [("hills", n) for n in NDIRS] + [("hand", 0), ("nasty", 16)]
    for kind, ndir in cases:
        z = terrain_of(ni, nj, kind)
        dxs = hand_table() if kind == "hand" else directions(ndir)
        want = scan_reference(ni, nj, ndir, kind)
        for nf in (1, 2, 4):
            what = "%dx%d %s ndir %d nf %d" % (ni, nj, kind, ndir, nf)
            svf, smax = host_skyview(z, dxs[0], dxs[1], DX, DY, NSTEP_TEST, nf)
            assert_same(svf.reshape(z.shape), _check_window(svf, smax, want, what), what)
    # the diagonal of the hand-made table is an exact tie, and a tie is x-major
    major, d, t, _ = np_ray(F(DX / 2000.0), F(DY / 2000.0), F(0.0), DX, DY)
    assert major == 1 and t == 1 and d == 1
    z = terrain_of(ni, nj)
    dxs = directions(16)
    for name, idx, ndst in tsh._indices(ni, nj)[1:]:
        wsvf, wsmax, todo = np_skyview(z, dxs[0], dxs[1], DX, DY, NSTEP_TEST, dst_index=idx, ndst=ndst)
        svf, smax = host_skyview(z, dxs[0], dxs[1], DX, DY, NSTEP_TEST, 2, dst_index=idx, ndst=ndst)
        _check_window(svf, smax, (wsvf, wsmax, todo), "%dx%d index %s" % (ni, nj, name))
        full = np.full(ndst, POISON, F)
        full[idx[todo].astype(np.int64)] = wsvf[todo]
        assert_same(svf, full, "%dx%d index %s: through dst_index, unwritten positions keep the poison" % (ni, nj, name))
        assert_same(wsvf[todo], scan_reference(ni, nj, 16)[0][todo], "a cell's factor does not depend on where it is written")


def test_the_terrain_closes_a_part_of_the_sky():
    """Asserted on the restatement alone: on the hills the factor lies in (0, 1], a good share of the cells sees less than the hemisphere,
    and every direction of the hand-made table that has no axis gives smax = 0."""
    svf, smax, _ = scan_reference(70, 130, 16)
    assert (svf > 0.2).all() and (svf <= 1).all() and 0.1 < (svf < 0.99).mean(), ((svf < 0.99).mean(), svf.min())
    _, smax, _ = scan_reference(70, 130, 0, "hand")
    assert (smax[0] == 0).all() and (smax[1] == 0).all() and (smax[-1] == 0).all() and (smax[2] > 0).any()


def test_flat_terrain_gives_one_exactly():
    """Every word is 0x3F800000, whatever ndir, the height of the plain and the number of steps in flight."""
    for ni, nj in ((35, 67), (5, 3), (1, 1)):
        for level in (0.0, -0.0, 1234.5):
            z = np.full((nj, ni), level, F)
            for ndir in NDIRS + (3, 7, 49):
                dxs = directions(ndir)
                want, _, _ = np_skyview(z, dxs[0], dxs[1], DX, DY, NSTEP_TEST)
                assert (want.view(np.uint32) == ONE).all()
                for nf in (1, 2, 4):
                    svf, _ = host_skyview(z, dxs[0], dxs[1], DX, DY, NSTEP_TEST, nf)
                    assert (svf.view(np.uint32) == ONE).all(), (ni, nj, level, ndir, nf)


def relief(ni, nj):
    r = np.random.default_rng(12)
    jj, ii = np.meshgrid(np.arange(nj), np.arange(ni), indexing="ij")
    return (1500.0 + 600.0 * np.sin(ii * 0.45) * np.cos(jj * 0.38) + r.uniform(-40.0, 40.0, (nj, ni))).astype(F)


def test_decomposition():
    """A 44 x 40 window cut 2 x 2: with a margin of nstep cells (none at the domain's edges) no cell differs from the undecomposed run,
    restated and compiled; with margin 0 some do, so the test can fail (the restatement gave 0 and 613 differing cells)."""
    ni, nj, nstep, ndir = 44, 40, 6, 16
    z = relief(ni, nj)
    dxs = directions(ndir)
    whole, _, _ = np_skyview(z, dxs[0], dxs[1], DX, DX, nstep)
    differs = {nstep: 0, 0: 0}
    for margin in differs:
        for tile, win, idx in tsh._cuts(ni, nj, margin):
            ndst = int(idx.max()) + 1
            svf, _, todo = np_skyview(z[win], dxs[0], dxs[1], DX, DX, nstep, dst_index=idx, ndst=ndst)
            part = svf[todo].reshape(whole[tile].shape)
            differs[margin] += int((part.view(np.uint32) != whole[tile].view(np.uint32)).sum())
            for nf in (1, 4):
                got, _ = host_skyview(z[win], dxs[0], dxs[1], DX, DX, nstep, nf, dst_index=idx, ndst=ndst)
                assert_same(got.reshape(part.shape), part, "compiled part, margin %d nf %d" % (margin, nf))
    print("differing cells: margin %d: %d, margin 0: %d" % (nstep, differs[nstep], differs[0]))
    assert differs[nstep] == 0
    assert differs[0] > 0


def test_tilted_plane():
    """z = a*x: the interpolation is exact on it, so a cell at least nstep from every edge has the float64 value of
    mean_q 1 / (1 + (a*gx_q)^2) over the upslope directions (gx of the unit direction) and 1 for the others.  Bound (12 + ndir) * 2^-24
    relative, counted from the text: at most 12 rounded operations per term, ndir - 1 additions, one division."""
    ni, nj, nstep, dx = 31, 31, 12, 1000.0
    jj, ii = np.meshgrid(np.arange(nj), np.arange(ni), indexing="ij")
    for a in (0.3, 0.05, 1.0):
        z = (a * dx * ii).astype(F)
        for ndir in (16, 8, 64):
            gx, gy = directions(ndir)
            ux = gx.astype(np.float64) / np.hypot(gx.astype(np.float64), gy.astype(np.float64))
            want = np.mean(np.where(ux > 0, 1.0 / (1.0 + (float(F(a)) * ux) ** 2), 1.0))
            svf, _, _ = np_skyview(z, gx, gy, dx, dx, nstep)
            for nf in (1, 2, 4):
                got, _ = host_skyview(z, gx, gy, dx, dx, nstep, nf)
                assert_same(got.reshape(z.shape), svf, "plane a %g ndir %d nf %d" % (a, ndir, nf))
            inner = svf[nstep:nj - nstep, nstep:ni - nstep].astype(np.float64)
            err = np.abs(inner / want - 1.0).max()
            print("a %g ndir %d: %.2f * 2^-24 (bound %d)" % (a, ndir, err / EPS, 12 + ndir))
            assert err <= (12 + ndir) * EPS, (a, ndir, err / EPS)


def test_cone_pit():
    """The centre cell of a cone pit of slope tan(beta): 1 / (1 + (1.08 tan beta)^2) <= svf <= (1 / (1 + tan^2 beta)) * (1 + ndir * 2^-24).
    Linear interpolation between two cells of a cone overestimates the radius by at most ((1 + sqrt 2) / 2) / sqrt 1.25 = 1.0797 (at k = 1,
    fo = 0.5); axis-parallel directions are exact.  (The restatement gives 0.7867 in [0.7742, 0.8] for tan beta = 0.5.)"""
    n, nstep, dx, ndir = 27, 12, 1000.0, 16
    jj, ii = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    c = n // 2
    gx, gy = directions(ndir)
    for tanb in (0.5, 0.1, 1.5):
        z = (tanb * dx * np.hypot(ii - c, jj - c)).astype(F)
        svf, _, _ = np_skyview(z, gx, gy, dx, dx, nstep)
        got, _ = host_skyview(z, gx, gy, dx, dx, nstep, 2)
        assert_same(got.reshape(z.shape), svf, "cone %g" % tanb)
        v = float(svf[c, c])
        lo, hi = 1.0 / (1.0 + (1.08 * tanb) ** 2), (1.0 / (1.0 + tanb ** 2)) * (1.0 + ndir * EPS)
        print("tan beta %g: svf %.4f in [%.4f, %.4f]" % (tanb, v, lo, hi))
        assert lo <= v <= hi, (tanb, lo, v, hi)


@pytest.mark.parametrize("ncell", ts.NCELLS_HOST)
def test_host_sky_column(ncell):
    """sw_column_sky / lw_column_sky compiled for the host against np_radiation_sky: physical, NaN / Inf / denormal and mixed operands, both
    modes, with and without normals, every combination of lit, albedo / emiss planes and glw; the configurations' times put mu on both
    sides of mu_min."""
    options = sky_options()
    sides = set()
    for which in ("physical", "nasty", "mixed"):
        y = sky_planes(ncell, which)
        for xset in (("physical", "nasty") if which != "mixed" else ("physical", "nasty_lat", "nasty_sw_a")):
            x = ts.operands(ncell, xset)
            for ci, cfg in enumerate(ts.CONFIGS):
                for opt in (options if ci % 5 == 0 else [options[(ci + len(xset)) % len(options)]]):
                    what = "n=%d sky %s set %s cfg %s opt %s" % (ncell, which, xset, cfg, opt)
                    sw, lw = restated_radiation(x, y, opt, cfg)
                    got_sw, got_lw = host_radiation(x, y, opt, cfg)
                    assert_same(got_sw, sw, what)
                    if opt[2]:
                        assert_same(got_lw, lw, what + ": glw")
                        keep = y["svf"] == 1
                        assert_same(got_lw[keep], y["glw"][keep], what + ": an open sky keeps glw")
                    else:
                        assert_same(got_lw, y["glw"], what + ": glw is not touched without the longwave group")
                if which == "physical" and xset == "physical" and ncell > 1:
                    mu = max0(np_sun(x["lat"], x["lon"], np_suntime(ts.TIMES[cfg[3]]))[2])
                    low = mu < F(ts.PARS[cfg[4]][1])
                    sides.add((bool(low.any()), bool((~low).any())))
    assert ncell == 1 or (True, True) in sides


@pytest.mark.parametrize("ncell", ts.NCELLS_HOST)
def test_host_sky_column_with_an_open_sky_is_the_lit_call(ncell):
    """svf == 1.0f everywhere: swdown has the bits of the restated lit call for lit in {1, 0, 0.25, NaN, -0} whatever albedo holds, and
    glw is untouched."""
    for which in ("physical", "nasty"):
        x = ts.operands(ncell, which)
        y = dict(sky_planes(ncell, which), svf=np.ones(ncell, F))
        for cfg in ts.CONFIGS:
            mode, with_b, terr, ti, pi = cfg
            for v in (1.0, 0.0, 0.25, np.nan, -0.0):
                lit = np.full(ncell, v, F)
                want, _ = np_lit(x, lit, mode, with_b, terr, np_suntime(ts.TIMES[ti]), ts.PARS[pi])
                for opt in ((True, True, True, True), (True, False, True, False)):
                    got_sw, got_lw = host_radiation(x, dict(y, lit=lit), opt, cfg)
                    what = "n=%d set %s cfg %s lit %r opt %s" % (ncell, which, cfg, v, opt)
                    assert_same(got_sw, want, what)
                    assert_same(got_lw, y["glw"], what + ": glw")
            # no lit plane at all: the unshaded call
            got_sw, _ = host_radiation(x, y, (False, True, False, False), cfg)
            assert_same(got_sw, ts.reference(ncell, which, cfg), "n=%d set %s cfg %s: no lit plane" % (ncell, which, cfg))


def _sky_block(svf=1, lit=0, albedo=0, glw=0, tsurf=0, emiss=0):
    b = abi.Sky()
    b.svf, b.lit, b.albedo, b.glw, b.tsurf, b.emiss = (v or None for v in (svf, lit, albedo, glw, tsurf, emiss))
    b.albedo_const, b.emiss_const, b.sigma = ALBEDO_CONST, EMISS_CONST, SIGMA
    return b


def test_refusals_write_nothing():
    """Every refusal returns -105 with text before anything is launched or read: the planes here are host memory that the calls must not
    touch, and they keep their poison.  Empty calls are served where a device is present (the GPU tests)."""
    lib = abi.load_library()
    ni, nj = 5, 3
    z = np.full((nj, ni), POISON, F)
    out = np.full(ni * nj, POISON, F)
    gx, gy = directions(8)

    def blk(**kw):
        b = abi.Skyview()
        b.height, b.svf, b.dir_x, b.dir_y = z.ctypes.data, out.ctypes.data, gx.ctypes.data, gy.ctypes.data
        b.dst_index = None
        b.ni, b.nj, b.nstep, b.ndir, b.dx, b.dy = ni, nj, NSTEP_TEST, 8, DX, DY
        for k, v in kw.items():
            setattr(b, k, v)
        return b

    def call(b, ndst=ni * nj):
        rc = lib.noahmp_hip_skyview(C.byref(b) if b is not None else None, ndst, None)
        return rc, lib.noahmp_hip_last_error().decode()
    rc, msg = call(None)
    assert rc == -105 and "NULL" in msg and "noahmp_hip_skyview" in msg
    for field in ("height", "svf", "dir_x", "dir_y"):
        rc, msg = call(blk(**{field: None}))
        assert rc == -105 and "required" in msg, (field, rc, msg)
    for kw, word in ((dict(ndir=0), "ndir"), (dict(ndir=65), "ndir"), (dict(ndir=-1), "ndir"), (dict(nstep=0), "nstep"),
                     (dict(nstep=abi.SHADOW_MAX_STEPS + 1), "nstep"), (dict(dx=0.0), "dx"), (dict(dx=-1.0), "dx"), (dict(dx=float("nan")), "dx"),
                     (dict(dy=float("inf")), "dy"), (dict(dy=0.0), "dy"), (dict(ni=-1), "ni"), (dict(nj=-1), "nj"), (dict(ni=65536, nj=32768), "ni")):
        rc, msg = call(blk(**kw))
        assert rc == -105 and word in msg, (kw, rc, msg)
    for ndst in (-1, 2 ** 31):
        rc, msg = call(blk(), ndst=ndst)
        assert rc == -105 and "ndst" in msg, (ndst, rc, msg)
    # the radiation call: its own refusals, and those of the shortwave calls
    n = 16
    planes = {k: np.full(n, POISON, F) for k in ("sw_a", "mean_a", "lat", "lon", "ne", "nn", "nu", "swdown", "svf", "glw", "tsurf")}
    now = (abi.SunTime * 1)()
    now[0].iday, now[0].ihour = 171, 18

    def swb(**kw):
        b = abi.Shortwave()
        b.sw_a, b.mean_a, b.xlat, b.lon, b.swdown = (planes[k].ctypes.data for k in ("sw_a", "mean_a", "lat", "lon", "swdown"))
        b.normal_e, b.normal_n, b.normal_u = (planes[k].ctypes.data for k in ("ne", "nn", "nu"))
        b.mode, b.max_ratio, b.mu_min, b.max_terrain_ratio, b.solar_constant = ZENITH, 10.0, 0.05, 5.0, 1361.0
        for k, v in kw.items():
            setattr(b, k, v)
        return b

    def sky_call(b, y, nc=n, when=now):
        rc = lib.noahmp_hip_forcing_radiation_sky(C.byref(b) if b is not None else None, C.byref(y) if y is not None else None, nc, when, None)
        return rc, lib.noahmp_hip_last_error().decode()
    good = _sky_block(svf=planes["svf"].ctypes.data, glw=planes["glw"].ctypes.data, tsurf=planes["tsurf"].ctypes.data)
    for y, word in ((None, "sky"), (_sky_block(svf=0), "svf"), (_sky_block(svf=planes["svf"].ctypes.data, glw=planes["glw"].ctypes.data), "tsurf")):
        rc, msg = sky_call(swb(), y)
        assert rc == -105 and word in msg and "noahmp_hip_forcing_radiation_sky" in msg, (word, rc, msg)
    rc, msg = sky_call(None, good)
    assert rc == -105 and "NULL" in msg
    rc, msg = sky_call(swb(), good, when=None)
    assert rc == -105 and "now" in msg
    for nc in (-1, 2 ** 31):
        rc, msg = sky_call(swb(), good, nc=nc)
        assert rc == -105 and "columns" in msg
    for kw, word in ((dict(sw_a=None), "required"), (dict(swdown=None), "required"), (dict(xlat=None), "required"), (dict(mean_a=None), "mean_a"),
                     (dict(normal_n=None), "all three or none"), (dict(mode=2), "mode")):
        rc, msg = sky_call(swb(**kw), good)
        assert rc == -105 and word in msg, (kw, rc, msg)
    assert (z == POISON).all() and (out == POISON).all() and all((p == POISON).all() for p in planes.values())


def test_bindings_regenerate_identically_with_the_skyview_calls():
    from tools import gen_abi
    for rel, text in (("include/noahmp_hip.h", gen_abi.c_header()), ("oracle/ref_harness_gen.f90", gen_abi.ref_harness()),
                      ("noahmp_amd/fortran/module_sf_noahmpdrv_hip.F90", gen_abi.fortran_shim()),
                      ("tests/fortran/shim_wrap_gen.f90", gen_abi.shim_wrap())):
        assert open(os.path.join(ROOT, rel)).read() == text, rel
    hdr = open(os.path.join(ROOT, "include", "noahmp_hip.h")).read()
    for word in ("typedef struct noahmp_skyview {", "} noahmp_skyview;", "typedef struct noahmp_sky {", "} noahmp_sky;",
                 "#define NOAHMP_HIP_HAS_FORCING_SKYVIEW 1\n", "#define NOAHMP_SKYVIEW_MAX_NDIR 64\n", "#define NOAHMP_HIP_ABI_MINOR 3\n",
                 "noahmp_hip_skyview(const noahmp_skyview* sv, int64_t ndst, void* stream);",
                 "noahmp_hip_forcing_radiation_sky(const noahmp_shortwave* sw, const noahmp_sky* sky, int64_t ncell, const noahmp_sun_time* now,",
                 "ENDS THE SCAN OF THIS DIRECTION", "dz = zt - z0;  s = dz / kf;  if s > smax: smax = s",
                 "td = t*so;  td2 = td*td;  sp2 = sp*sp;  L2 = sp2 + td2;  s2 = smax*smax;  den = L2 + s2;  term = L2 / den",
                 "svf[dst_index[c]] = acc / (float)ndir", "r = r0*l;  dif = kd*v;  beam = 1.0f - kd;  br = beam*r;  f0 = dif + br",
                 "o = 1.0f - v;  refl = al*o;  f = f0 + refl;  swdown[c] = s*f",
                 "t2 = T*T;  t4 = t2*t2;  b = sigma*t4;  eb = e*b;  up = o*eb;  dn = v*g;  glw[c] = dn + up", "OWN horizontal global flux",
                 "margin is at least nstep cells"):
        assert word in hdr, word
    assert "sky-view factor and terrain-reflected light are NOT represented" not in hdr
    assert "noahmp_sky" not in gen_abi.ref_harness()
    f90 = open(os.path.join(ROOT, "noahmp_amd", "fortran", "module_sf_noahmpdrv_hip.F90")).read()
    for word in ("bind(C, name='noahmp_hip_skyview')", "bind(C, name='noahmp_hip_forcing_radiation_sky')", "type, bind(C) :: noahmp_skyview",
                 "type, bind(C) :: noahmp_sky ", "NOAHMP_SKYVIEW_MAX_NDIR = 64"):
        assert word in f90, word
    assert "noahmp_hip_skyview" in abi.EXPORTED_SYMBOLS and "noahmp_hip_forcing_radiation_sky" in abi.EXPORTED_SYMBOLS
    assert [n for n, _ in abi.Skyview._fields_] == ["height", "dst_index", "svf", "ni", "nj", "nstep", "ndir", "dx", "dy", "dir_x", "dir_y"]
    assert [n for n, _ in abi.Sky._fields_] == ["svf", "lit", "albedo", "albedo_const", "glw", "tsurf", "emiss", "emiss_const", "sigma"]


def test_ctypes_mirrors_match_the_compiled_header(tmp_path):
    body, want = "", []
    for cname, cls in (("noahmp_skyview", abi.Skyview), ("noahmp_sky", abi.Sky)):
        names = [n for n, _ in cls._fields_]
        body += 'printf(" %%zu", sizeof(%s));' % cname + "".join('printf(" %%zu", offsetof(%s, %s));' % (cname, n) for n in names)
        want += [C.sizeof(cls)] + [getattr(cls, n).offset for n in names]
    body += 'printf(" %zu", sizeof(noahmp_shortwave));'
    want += [C.sizeof(abi.Shortwave)]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "noahmp_hip.h"\nint main(){' + body +
                   'printf(" %d %d %d", NOAHMP_HIP_ABI_MINOR, NOAHMP_HIP_HAS_FORCING_SKYVIEW, NOAHMP_SKYVIEW_MAX_NDIR); return 0;}')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert out == want + [3, 1, 64]


def test_library_exports_the_skyview_calls():
    if not os.path.exists(abi.LIB_PATH):
        from noahmp_amd import build as b
        b.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", abi.LIB_PATH]).decode()
    assert " T noahmp_hip_skyview\n" in out and " T noahmp_hip_forcing_radiation_sky\n" in out


@pytest.mark.skipif(tr._flang() is None, reason="no flang")
def test_generated_fortran_types_and_interfaces_compile(tmp_path):
    """The sky-view part of the generated module compiles on top of the shortwave part, and a caller of both interfaces type-checks."""
    from tools import gen_abi
    text = "\n".join(["module skyview_abi_check", "  use iso_c_binding", "  implicit none"] + gen_abi.shortwave_f90_types() +
                     gen_abi.skyview_f90_types() + ["  interface"] + gen_abi.shortwave_f90_interfaces() + gen_abi.skyview_f90_interfaces() +
                     ["  end interface", "contains", "  function go(ncell, planes, sw) result(rc)", "    integer(c_int64_t), value :: ncell",
                      "    type(c_ptr), intent(in) :: planes(6)", "    type(noahmp_shortwave), intent(in) :: sw", "    type(noahmp_skyview) :: sv",
                      "    type(noahmp_sky) :: sky", "    type(noahmp_sun_time) :: t", "    integer(c_int) :: rc",
                      "    real(c_float), target :: gx(16), gy(16)", "    gx = 0.0; gy = 1.0",
                      "    t%iday = 355; t%ihour = 22; t%iminute = 30; t%isecond = 0",
                      "    sv%height = planes(1); sv%dst_index = c_null_ptr; sv%svf = planes(2); sv%ni = 64; sv%nj = 8; sv%nstep = 25",
                      "    sv%ndir = min(16, NOAHMP_SKYVIEW_MAX_NDIR); sv%dx = 1000.0; sv%dy = 1000.0; sv%dir_x = c_loc(gx); sv%dir_y = c_loc(gy)",
                      "    rc = noahmp_hip_skyview(sv, ncell, c_null_ptr)",
                      "    sky%svf = planes(2); sky%lit = planes(3); sky%albedo = c_null_ptr; sky%glw = planes(4); sky%tsurf = planes(5)",
                      "    sky%emiss = planes(6); sky%albedo_const = 0.2; sky%emiss_const = 0.95; sky%sigma = 5.67e-8",
                      "    rc = noahmp_hip_forcing_radiation_sky(sw, sky, ncell, t, c_null_ptr)",
                      "  end function go", "end module skyview_abi_check", ""])
    f = tmp_path / "skyview_abi_check.f90"
    f.write_text(text)
    subprocess.check_call([tr._flang(), "-c", str(f), "-o", str(tmp_path / "skyview_abi_check.o"), "-J", str(tmp_path)], cwd=str(tmp_path))


# ---------------------------------------------------------------------------------------------------------------- GPU
_dev = tr._dev


@pytest.mark.gpu
@pytest.mark.parametrize("ni, nj", WINDOWS_GPU)
def test_gpu_scan_kernel_equals_the_restatement(engine, ni, nj):
    """noahmp_hip_skyview against np_skyview: ndir 1 / 8 / 16 / 64 and the hand-made table; identity, permuted and margin dst_index (the
    margin's positions keep the poison); the nasty terrain.  35 x 67 = 2345 cells end in a ragged workgroup and a ragged wave.
    Destinations are offset by one float inside a poisoned pool whose guard words keep the poison."""
    import torch
    ncell = ni * nj
    pool = torch.full((ncell + 9,), POISON, dtype=torch.float32, device="cuda")
    dst = pool[5:5 + ncell]
    torch.cuda.synchronize()
    cases = [("hills", n) for n in NDIRS_GPU] + [("hand", 0), ("nasty", 16)]
    for kind, ndir in cases:
        z = terrain_of(ni, nj, kind)
        zd = _dev(z)
        dxs = hand_table() if kind == "hand" else directions(ndir)
        wsvf, _, _ = scan_reference(ni, nj, ndir, kind)
        for name, idx, ndst in (tsh._indices(ni, nj) if ndir in (0, 16) else tsh._indices(ni, nj)[:1]):
            idxd = _dev(idx) if idx is not None else None
            pool.fill_(POISON)
            torch.cuda.synchronize()
            b = engine.skyview_block(zd, dst, DX, DY, nstep=NSTEP_TEST, dst_index=idxd, dir_x=dxs[0], dir_y=dxs[1])
            engine.skyview(b, ndst)
            engine.stream_sync()
            h = pool.cpu().numpy()
            what = "%dx%d %s ndir %d index %s" % (ni, nj, kind, ndir, name)
            want = np.full(ncell, POISON, F)
            flat_idx = np.arange(ncell) if idx is None else idx.ravel().astype(np.int64)
            ok = (flat_idx >= 0) & (flat_idx < ndst)
            want[flat_idx[ok]] = wsvf.ravel()[ok]
            assert_same(h[5:5 + ncell], want, what)
            assert (h[:5] == POISON).all() and (h[5 + ncell:] == POISON).all(), what + ": guard words"
            if name == "margin" and not ok.all():
                assert (h[5:5 + ncell][~ok] == POISON).all(), what + ": unwritten cells keep the poison"
    # the table of the Python layer is the table of the tests
    gx, gy = engine.skyview_directions(16)
    assert_same(gx, directions(16)[0], "dir_x")
    assert_same(gy, directions(16)[1], "dir_y")
    # empty calls return 0 and write nothing
    pool.fill_(POISON)
    torch.cuda.synchronize()
    zd = _dev(terrain_of(ni, nj))
    engine.skyview(engine.skyview_block(zd, dst, DX, DY, nstep=NSTEP_TEST, ndir=8), 0)
    engine.stream_sync()
    assert (pool.cpu().numpy() == POISON).all()


@pytest.mark.gpu
def test_gpu_scan_of_a_cut_window_equals_the_whole(engine):
    """70 x 130 cut 2 x 2 with a margin of nstep = 12 cells: every part has the bits of the undecomposed launch and of the restatement."""
    import torch
    ni, nj, ndir = 70, 130, 16
    z = terrain_of(ni, nj)
    gx, gy = directions(ndir)
    whole = torch.full((nj, ni), POISON, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    engine.skyview(engine.skyview_block(_dev(z), whole, DX, DY, nstep=NSTEP_TEST, ndir=ndir), ni * nj)
    engine.stream_sync()
    whole_h = whole.cpu().numpy()
    assert_same(whole_h, scan_reference(ni, nj, ndir)[0], "the whole window")
    for tile, win, idx in tsh._cuts(ni, nj, NSTEP_TEST):
        ndst = int(idx.max()) + 1
        part = torch.full((ndst,), POISON, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        engine.skyview(engine.skyview_block(_dev(z[win]), part, DX, DY, nstep=NSTEP_TEST, ndir=ndir, dst_index=_dev(idx)), ndst)
        engine.stream_sync()
        assert_same(part.cpu().numpy().reshape(whole_h[tile].shape), whole_h[tile], "part %s" % (tile,))


@pytest.mark.gpu
@pytest.mark.parametrize("ncell", (1, 63, 64, 65, 9100))
def test_gpu_radiation_kernel_equals_the_restatement(engine, ncell):
    """noahmp_hip_forcing_radiation_sky against np_radiation_sky for every combination of the optional planes, physical and nasty
    operands, the configurations of test_shortwave spread over them; with an all-ones svf it equals noahmp_hip_forcing_shortwave_lit run
    here on the same planes, word for word, and glw is unchanged."""
    import torch
    options = sky_options()
    ones_d = _dev(np.ones(ncell, F))
    pool = torch.full((4, ncell + 9), POISON, dtype=torch.float32, device="cuda")
    sw_dst, glw_dst, sw_one, sw_lit = (pool[k, 5:5 + ncell] for k in range(4))
    k = 0
    for which in ("physical", "nasty"):
        x, y = ts.operands(ncell, which), sky_planes(ncell, which)
        xd, yd = {n: _dev(v) for n, v in x.items()}, {n: _dev(v) for n, v in y.items()}
        torch.cuda.synchronize()
        for opt in options:
            use_lit, use_alb, use_glw, use_em = opt
            for cfg in ts.CONFIGS[k % 5::5]:
                k += 1
                mode, with_b, terr, ti, pi = cfg
                what = "ncell %d set %s cfg %s opt %s" % (ncell, which, cfg, opt)
                pool.fill_(POISON)
                glw_dst.copy_(yd["glw"])
                torch.cuda.synchronize()

                def sky(svf, glw):
                    return engine.sky_block(svf, lit=yd["lit"] if use_lit else None, albedo=yd["albedo"] if use_alb else ALBEDO_CONST,
                                            glw=glw if use_glw else None, tsurf=yd["tsurf"] if use_glw else None,
                                            emiss=yd["emiss"] if use_em else EMISS_CONST, sigma=SIGMA)
                engine.forcing_radiation_sky(ts._block(engine, xd, sw_dst, mode, with_b, terr, ts.PARS[pi]), sky(yd["svf"], glw_dst), ncell, ts.TIMES[ti])
                engine.stream_sync()
                h = pool.cpu().numpy()
                sw, lw = restated_radiation(x, y, opt, cfg)
                assert_same(h[0, 5:5 + ncell], sw, what)
                assert_same(h[1, 5:5 + ncell], lw if use_glw else y["glw"], what + ": glw")
                # an open sky everywhere
                glw_dst.copy_(yd["glw"])
                torch.cuda.synchronize()
                engine.forcing_radiation_sky(ts._block(engine, xd, sw_one, mode, with_b, terr, ts.PARS[pi]), sky(ones_d, glw_dst), ncell, ts.TIMES[ti])
                engine.forcing_shortwave_lit(ts._block(engine, xd, sw_lit, mode, with_b, terr, ts.PARS[pi]), yd["lit"] if use_lit else ones_d, ncell,
                                             ts.TIMES[ti])
                engine.stream_sync()
                h = pool.cpu().numpy()
                assert_same(h[2, 5:5 + ncell], h[3, 5:5 + ncell], what + ": all ones is the lit call")
                assert_same(h[1, 5:5 + ncell], y["glw"], what + ": all ones keeps glw")
                assert (h[:, :5] == POISON).all() and (h[:, 5 + ncell:] == POISON).all(), what + ": guard words"


VAL_NI, VAL_NJ, VAL_MARGIN, VAL_NSTEP = 35, 67, 4, 6


def _valley(flat=False):
    """The window of the engine runs: valleys along j, 8 cells from ridge to ridge and 1800 m deep, with side valleys; the tile plus a
    margin of 4 cells along i."""
    jj, ii = np.meshgrid(np.arange(VAL_NJ), np.arange(VAL_NI + 2 * VAL_MARGIN), indexing="ij")
    if flat:
        return np.full(ii.shape, 800.0, F)
    return (600.0 + 900.0 * (1.0 - np.cos(2.0 * np.pi * ii / 8.0)) + 250.0 * np.sin(jj * 0.5) * np.cos(ii * 0.8)).astype(F)


def _valley_latlon():
    jj, ii = np.meshgrid(np.arange(VAL_NJ), np.arange(VAL_NI), indexing="ij")
    return (38.0 + 0.009 * jj).astype(F), (-1.5 + 0.0115 * ii).astype(F)


VAL_STEPS = [(355, 15, 30, 0), (355, 16, 0, 0)]                                   # a winter afternoon at 1.5 W: mu about 0.2 and 0.12, in the south-west
VAL_START = (2000, 355, 15, 30, 0)
VAL_PAR = dict(max_ratio=10.0, mu_min=0.05, max_terrain_ratio=5.0, solar_constant=1361.0)
VAL_PARV = (10.0, 0.05, 5.0, 1361.0)


def _valley_run(engine, tables, recs, height, sort, skyview, grab):
    """Two engine steps of the 35 x 67 tile: forcing_interpolate_prep, Shortwave.apply (ZENITH, terrain normals, set_shadow and -- with
    skyview -- set_skyview from the store's planes), noahmplsm.  grab(store, sw, it) runs after apply() and before the step."""
    import torch
    from noahmp_amd import synth
    from noahmp_amd.shortwave import Shortwave
    T, tb = tables
    lat, lon_h = _valley_latlon()
    s = synth.mixed_small(tb, ni=VAL_NI, nj=VAL_NJ)
    s.a["xlatin"][...] = lat
    synth.first_step_fixups(s)
    synth.diurnal_forcing(s, 12, t_offset=s.t_offset)
    d = s.to_device("cuda:0")
    lon = _dev(lon_h)
    rain = torch.zeros((VAL_NJ, VAL_NI), dtype=torch.float32, device="cuda:0")
    heightd = _dev(height)
    torch.cuda.synchronize()
    sw = Shortwave(engine, _dev(lat), _dev(lon_h), mode="zenith", **VAL_PAR)
    sw.terrain_from_height(heightd[:, VAL_MARGIN:VAL_MARGIN + VAL_NI], DX, DX)
    sw.set_shadow(heightd, DX, DX, nstep=VAL_NSTEP, origin=(VAL_MARGIN, 0))
    if skyview:
        sw.set_skyview(heightd, DX, DX, nstep=VAL_NSTEP, ndir=16, origin=(VAL_MARGIN, 0))
    if sort:
        engine.sort_store(d)
        perm = d.sort_perm.long()
        lon = lon.reshape(-1)[perm].reshape(VAL_NJ, VAL_NI).contiguous()
        recs = [{k: v.reshape(-1)[perm].reshape(VAL_NJ, VAL_NI).contiguous() for k, v in r.items()} for r in recs]
        torch.cuda.synchronize()
        sw.follow(d)
    sw.interval(VAL_START, 10800, 6)
    for it in (1, 2):
        now = VAL_STEPS[it - 1]
        jul = engine.forcing_interpolate_prep(d, recs[0], recs[1], 1800 * (it - 1), 10800, rain, lon, *now, scale_vegfra=True, first_step=(it == 1))
        engine.stream_sync()
        before = {k: d.a[k].cpu().numpy().ravel().copy() for k in ("albedo", "emiss", "tsk", "glw")}
        sw.apply(d, recs[0], recs[1], 1800 * (it - 1), 10800, now)
        engine.stream_sync()
        torch.cuda.synchronize()
        grab(d, sw, it, before)
        st = engine.noahmplsm(d, it, 2000, jul)
        assert st.code == 0
    return d, sw


def _valley_records():
    r = np.random.default_rng(41)
    recs_h = [{k: r.uniform(lo, hi, (VAL_NJ, VAL_NI)).astype(F) for k, (lo, hi) in tr.COARSE.items()} for _ in range(2)]
    return recs_h, [{k: _dev(v) for k, v in rec.items()} for rec in recs_h]


@pytest.mark.gpu
def test_gpu_engine_run_in_a_valley(engine, tables):
    """Two engine steps through set_shadow + set_skyview + apply on a 35 x 67 tile with a valley: swdown and glw of the store equal the
    restatement chained on the store's own albedo / emiss / tsk (read before apply) and the restated lit and sky-view planes; the run on
    a sorted store after follow(), returned to tile order, equals the unsorted one."""
    from noahmp_amd import shortwave as swmod
    height = _valley()
    recs_h, recs = _valley_records()
    lat, lon = _valley_latlon()
    seen = {}

    def grabber(tag):
        def grab(d, sw, it, before):
            seen[tag, it] = dict(before, swdown=d.a["swdown"].cpu().numpy().ravel().copy(), glw_after=d.a["glw"].cpu().numpy().ravel().copy(),
                                 svf=sw.svf.cpu().numpy().ravel().copy(), lit=sw.lit.cpu().numpy().ravel().copy())
        return grab
    d, sw = _valley_run(engine, tables, recs, height, False, True, grabber("tile"))
    normal = [t.cpu().numpy().ravel() for t in sw.normal_tile]
    gx, gy = directions(16)
    idx = np.full(height.shape, -1, np.int32)
    idx[:, VAL_MARGIN:VAL_MARGIN + VAL_NI] = np.arange(VAL_NI * VAL_NJ, dtype=np.int32).reshape(VAL_NJ, VAL_NI)
    wsvf, _, todo = np_skyview(height, gx, gy, DX, DX, VAL_NSTEP, dst_index=idx, ndst=VAL_NI * VAL_NJ)
    svf = wsvf[todo]
    assert 0.5 < (svf < 0.97).mean() and svf.min() > 0.3, ((svf < 0.97).mean(), svf.min())
    sample_suns = [np_suntime(t[1:]) for t in swmod.sample_times(VAL_START, 10800, 6)]
    mean_h = ts.np_mean(lat.ravel(), lon.ravel(), sample_suns)
    x = dict(sw_a=recs_h[0]["sw"].ravel(), sw_b=recs_h[1]["sw"].ravel(), mean_a=mean_h, lat=lat.ravel(), lon=lon.ravel(),
             ne=normal[0], nn=normal[1], nu=normal[2])
    latw, lonw = np.zeros_like(height), np.zeros_like(height)
    latw[:, VAL_MARGIN:VAL_MARGIN + VAL_NI], lonw[:, VAL_MARGIN:VAL_MARGIN + VAL_NI] = lat, lon
    shadowed = 0
    for it in (1, 2):
        t = VAL_STEPS[it - 1]
        g = seen["tile", it]
        ex, _ = tsh.np_cells(height, latw, lonw, np_suntime(t), DX, DX, VAL_NSTEP, 0.05, height.max(), dst_index=idx, ndst=VAL_NI * VAL_NJ)
        lit = tsh.lit_of(ex[:, VAL_MARGIN:VAL_MARGIN + VAL_NI]).ravel()
        shadowed += int((lit == 0).sum())
        assert_same(g["svf"], svf, "the sky-view plane, step %d" % it)
        assert_same(g["lit"], lit, "the lit plane, step %d" % it)
        sw_want, lw_want = np_radiation_sky(x, svf, lit, g["albedo"], g["glw"], g["tsk"], g["emiss"], 5.67e-8, ZENITH, False, True, np_suntime(t),
                                            VAL_PARV)
        assert_same(g["swdown"], sw_want, "SWDOWN of step %d" % it)
        assert_same(g["glw_after"], lw_want, "GLW of step %d" % it)
        assert (g["glw_after"] != g["glw"]).mean() > 0.5 and (sw_want > 0).any()
        plain, _ = np_lit(x, lit, ZENITH, False, True, np_suntime(t), VAL_PARV)
        assert (plain != sw_want).mean() > 0.3, "the sky view changes the shortwave"
    assert shadowed > 20
    assert (seen["tile", 1]["albedo"] != seen["tile", 2]["albedo"]).any() or (seen["tile", 1]["tsk"] != seen["tile", 2]["tsk"]).any(), \
        "the second step reads what the first step wrote"
    ds, sws = _valley_run(engine, tables, recs, height, True, True, grabber("sorted"))
    perm = ds.sort_perm.cpu().numpy()
    assert (perm != np.arange(perm.size)).any()
    for it in (1, 2):
        for k in ("svf", "lit", "swdown", "glw_after"):
            assert_same(seen["sorted", it][k], seen["tile", it][k][perm], "%s of the sorted run, step %d" % (k, it))
        for k in ("albedo", "emiss", "tsk", "glw"):
            assert_same(seen["sorted", it][k], seen["tile", it][k][perm], "%s of the store before step %d, sorted run" % (k, it))


@pytest.mark.gpu
def test_gpu_engine_run_on_flat_terrain(engine, tables):
    """The same two steps on flat terrain: every array of the store is bit-identical to the run without set_skyview."""
    from tools.compare import exact_check
    height = _valley(flat=True)
    _, recs = _valley_records()
    svfs = []
    with_sky, sw = _valley_run(engine, tables, recs, height, False, True, lambda d, s, it, before: svfs.append(s.svf.cpu().numpy()))
    without, _ = _valley_run(engine, tables, recs, height, False, False, lambda *a: None)
    assert all((v.view(np.uint32) == ONE).all() for v in svfs)
    ok, lines = exact_check(without.to_host(), with_sky.to_host())
    assert ok, "\n".join(lines)
    assert_same(with_sky.a["swdown"].cpu().numpy(), without.a["swdown"].cpu().numpy(), "SWDOWN")
    assert_same(with_sky.a["glw"].cpu().numpy(), without.a["glw"].cpu().numpy(), "GLW")
