"""Terrain-adjusted wind in the forcing: slope and curvature of the terrain and the MicroMet weighting and turning of a record's wind
(noahmp_hip_wind_terrain, noahmp_hip_forcing_wind; nmp_dev_wind.hpp).

No reference routine stands behind the calls; the contract is the text in include/noahmp_hip.h.  np_wind_terrain and np_forcing_wind restate
it in numpy float32, one rounded operation per line, with glibc's atanf / sinf / cosf through ctypes.  Everything is compared with the
restatement bit for bit (test_regrid.assert_same: equal bits, or both NaN): the per-cell functions compiled for the host, both kernels, and
two engine steps through WindTerrain.set_terrain / record.  A tolerance appears only where the restatement is held against MicroMet as
published in float64 and in the analytic checks; where each comes from is said there."""
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
import test_skyview as tsv
from test_regrid import F, assert_same, nasty

ROOT = tr.ROOT
CSRC = tr.CSRC
SRC = os.path.join(ROOT, "tests", "host_emul", "wind_check.hip")
LIB = os.path.join(ROOT, "tests", "host_emul", "libwind_check.so")
WINDOWS = tsh.WINDOWS
WINDOWS_GPU = tsh.WINDOWS_GPU
NCURVS = (1, 3, 64)
DX, DY = 1000.0, 1500.0                                                  # dx != dy
POISON = 7.0
EPS = 2.0 ** -24
GAMMA_S, GAMMA_C = 0.58, 0.42
TURN = 1

_libm = C.CDLL("libm.so.6")
_libm.atanf.restype = C.c_float
_libm.atanf.argtypes = [C.c_float]


def atanf(x):
    """glibc's atanf, element by element (every argument, NaN and Inf included)."""
    x = np.asarray(x, F)
    return np.array([_libm.atanf(float(v)) for v in x.ravel()], F).reshape(x.shape)


# ---------------------------------------------------------------------------------------------------------------- the restatement
def _curv_term(z, a, b, den):
    s = a + b
    h = F(0.5) * s
    n = z - h
    return (n / den).astype(F)


def np_wind_terrain(height, dx, dy, ncurv, rot=None, dst_index=None, ndst=None):
    """noahmp_hip_wind_terrain over a window: sx, sy, curv in WINDOW order and the mask of the written cells."""
    z = np.asarray(height, F)
    nj, ni = z.shape
    ncell = z.size
    idx = np.arange(ncell).reshape(z.shape) if dst_index is None else np.asarray(dst_index).reshape(z.shape)
    todo = (idx >= 0) & (idx < (ncell if ndst is None else ndst))
    dx, dy = F(dx), F(dy)
    jj, ii = np.meshgrid(np.arange(nj, dtype=np.int64), np.arange(ni, dtype=np.int64), indexing="ij")
    ie, iw = np.minimum(ii + 1, ni - 1), np.maximum(ii - 1, 0)
    jn, js = np.minimum(jj + 1, nj - 1), np.maximum(jj - 1, 0)
    with np.errstate(all="ignore"):
        dzx = z[jj, ie] - z[jj, iw]
        lenx = (ie - iw).astype(F) * dx
        gx = np.where(ie == iw, F(0.0), dzx / lenx).astype(F)
        dzy = z[jn, ii] - z[js, ii]
        leny = (jn - js).astype(F) * dy
        gy = np.where(jn == js, F(0.0), dzy / leny).astype(F)
        if rot is not None:
            ca, sa = (np.asarray(t, F) for t in rot)
            p1 = gx * ca
            p2 = gy * sa
            p3 = gy * ca
            p4 = gx * sa
            ge = p1 - p2
            gn = p3 + p4
        else:
            ge, gn = gx, gy
        ge2 = ge * ge
        gn2 = gn * gn
        g2 = ge2 + gn2
        g = np.sqrt(g2)
        beta = atanf(g)
        q = beta / g
        sx = np.where(g == 0, F(0.0), ge * q).astype(F)
        sy = np.where(g == 0, F(0.0), gn * q).astype(F)
        E, W = np.minimum(ii + ncurv, ni - 1), np.maximum(ii - ncurv, 0)
        N, S = np.minimum(jj + ncurv, nj - 1), np.maximum(jj - ncurv, 0)
        nc = F(ncurv)
        lx = F(nc * dx)
        ly = F(nc * dy)
        dx2 = F(dx * dx)
        dy2 = F(dy * dy)
        d2 = F(dx2 + dy2)
        d = F(nc * np.sqrt(d2))
        t1 = _curv_term(z, z[jj, W], z[jj, E], F(F(2.0) * lx))
        t2 = _curv_term(z, z[S, ii], z[N, ii], F(F(2.0) * ly))
        t3 = _curv_term(z, z[S, W], z[N, E], F(F(2.0) * d))
        t4 = _curv_term(z, z[N, W], z[S, E], F(F(2.0) * d))
        t12 = t1 + t2
        t123 = t12 + t3
        t1234 = t123 + t4
        curv = (F(0.25) * t1234).astype(F)
    assert sx.dtype == F and sy.dtype == F and curv.dtype == F
    return sx, sy, curv, todo


def _clamp_half(x):
    x = np.where(x < F(-0.5), F(-0.5), x).astype(F)
    return np.where(x > F(0.5), F(0.5), x).astype(F)


def np_forcing_wind(u, v, sx, sy, curv, slope_max, curv_max, gamma_s=GAMMA_S, gamma_c=GAMMA_C, flags=TURN):
    """noahmp_hip_forcing_wind over planes: (u', v', parts); parts holds keep (the columns that keep their bits), ww and td."""
    u, v, sx, sy, curv = (np.asarray(t, F).ravel() for t in (u, v, sx, sy, curv))
    slope_max, curv_max, gamma_s, gamma_c = F(slope_max), F(curv_max), F(gamma_s), F(gamma_c)
    with np.errstate(all="ignore"):
        flat = (sx == 0) & (sy == 0) & (curv == 0)
        uu = u * u
        vv = v * v
        W2 = uu + vv
        W = np.sqrt(W2)
        keep = flat | (W == 0)
        d1 = u * sx
        d2 = v * sy
        dot = d1 + d2
        r = dot / W
        ds = F(slope_max + slope_max)
        os_ = _clamp_half(r / ds)
        dc = F(curv_max + curv_max)
        oc = _clamp_half(curv / dc)
        a = gamma_s * os_
        b = gamma_c * oc
        wa = F(1.0) + a
        ww = wa + b
        td = np.zeros_like(u)
        if not (flags & TURN):
            un = ww * u
            vn = ww * v
        else:
            sx2 = sx * sx
            sy2 = sy * sy
            b2 = sx2 + sy2
            c1 = sx * v
            c2 = sy * u
            cr = c1 - c2
            n = F(2.0) * dot
            n = n * cr
            m = W2 * b2
            s2 = np.where(b2 == 0, F(0.0), n / m).astype(F)
            h = F(-0.5) * os_
            td = h * s2
            ct, st = ts.cosf(td), ts.sinf(td)
            uc = u * ct
            vs = v * st
            vc = v * ct
            us = u * st
            ur = uc + vs
            vr = vc - us
            un = ww * ur
            vn = ww * vr
    un, vn = np.where(keep, u, un), np.where(keep, v, vn)
    assert un.dtype == F and vn.dtype == F and ww.dtype == F and td.dtype == F
    return un, vn, dict(keep=keep, ww=ww, td=td, os=os_, oc=oc)


def window_maxima(sx, sy, curv):
    """The defaults of the Python layer: the maxima of sqrt(sx^2 + sy^2) and of |curv| over the window."""
    return float(np.sqrt(sx * sx + sy * sy).max()), float(np.abs(curv).max())


# ---------------------------------------------------------------------------------------------------------------- the inputs
terrain_of = tsv.terrain_of                                            # kind: hills = test_shadow.terrain, nasty = with NaN / Inf / denormal words


@functools.lru_cache(maxsize=None)
def terrain_reference(ni, nj, ncurv, kind="hills", rot=False):
    out = np_wind_terrain(terrain_of(ni, nj, kind), DX, DY, ncurv, rot=tsh.rotation(ni, nj) if rot else None)
    for a in out:
        a.setflags(write=False)
    return out


def terrain_cases():
    """(kind, ncurv, rot): the three lengths with and without rotation planes on the hills, the nasty terrain with and without them."""
    return [("hills", n, r) for n in NCURVS for r in (False, True)] + [("nasty", 3, False), ("nasty", 1, True)]


def wind_operands(ncell, which):
    """u, v, sx, sy, curv of ncell columns: physical (about a sixth of the columns on flat ground, a few calm), nasty, or mixed."""
    r = np.random.default_rng(1700 + ncell + len(which))
    ang, beta = r.uniform(0.0, 2.0 * np.pi, ncell), r.uniform(0.0, 0.9, ncell)
    phys = dict(u=r.uniform(-12.0, 12.0, ncell).astype(F), v=r.uniform(-12.0, 12.0, ncell).astype(F), sx=(beta * np.cos(ang)).astype(F),
                sy=(beta * np.sin(ang)).astype(F), curv=r.uniform(-0.05, 0.05, ncell).astype(F))
    flat = r.random(ncell) < 0.17
    for k in ("sx", "sy", "curv"):
        phys[k][flat] = r.choice(np.array([0.0, -0.0], F), int(flat.sum()))
    calm = r.random(ncell) < 0.05
    phys["u"][calm] = r.choice(np.array([0.0, -0.0], F), int(calm.sum()))
    phys["v"][calm] = r.choice(np.array([0.0, -0.0], F), int(calm.sum()))
    if which == "physical":
        return phys
    nas = {k: nasty(r, ncell) for k in phys}
    if which == "nasty":
        return nas
    pick = {k: r.random(ncell) < 0.5 for k in phys}
    return {k: np.where(pick[k], phys[k], nas[k]).astype(F) for k in phys}


MAXIMA = ((0.9, 0.05), (0.009, 0.0005))                                  # about the operands' own maxima, and a hundred times too small


# ---------------------------------------------------------------------------------------------------------------- CPU
def build():
    deps = [SRC, os.path.join(CSRC, "nmp_dev_wind.hpp"), os.path.join(CSRC, "nmp_libm.hpp"), os.path.join(CSRC, "nmp_libm_tables.inc"),
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
    lib.wind_terrain_cells.argtypes = [I, I, V, V, V, V, C.c_long, I, Fl, Fl, V, V, V]
    lib.wind_columns.argtypes = [C.c_long, V, V, V, V, V, Fl, Fl, Fl, Fl, I, V]
    lib.wind_terrain_cells.restype = lib.wind_columns.restype = None
    return lib


_p = ts._p


def _c(a, dtype=F):
    return np.ascontiguousarray(a, dtype)


def host_wind_terrain(height, dx, dy, ncurv, rot=None, dst_index=None, ndst=None):
    height = _c(height)
    nj, ni = height.shape
    ndst = height.size if ndst is None else ndst
    out = [np.full(max(ndst, 1), POISON, F) for _ in range(3)]
    idx = _c(dst_index, np.int32) if dst_index is not None else None
    ca, sa = (_c(rot[0]), _c(rot[1])) if rot is not None else (None, None)
    _host().wind_terrain_cells(ni, nj, _p(height), _p(ca), _p(sa), _p(idx), ndst, int(ncurv), float(dx), float(dy), *[_p(o) for o in out])
    return [o[:ndst] for o in out]


def host_wind_columns(x, slope_max, curv_max, flags, gamma_s=GAMMA_S, gamma_c=GAMMA_C):
    a = {k: _c(t).ravel().copy() for k, t in x.items()}
    n = a["u"].size
    changed = np.zeros(n, np.uint8)
    _host().wind_columns(n, _p(a["u"]), _p(a["v"]), _p(a["sx"]), _p(a["sy"]), _p(a["curv"]), float(slope_max), float(curv_max), float(gamma_s),
                         float(gamma_c), int(flags), _p(changed))
    return a["u"], a["v"], changed.astype(bool)


def _through(idx, todo, ndst, plane):
    full = np.full(ndst, POISON, F)
    full[idx[todo].astype(np.int64)] = plane[todo]
    return full


@pytest.mark.parametrize("ni, nj", WINDOWS)
def test_host_terrain_equals_the_restatement(ni, nj):
    """wind_terrain_cell compiled for the host against np_wind_terrain: ncurv 1 / 3 / 64 (64 clamps every neighbour in every window here),
    dx != dy, with and without rotation planes, terrain with NaN / Inf / denormal words, and identity, permuted and margin dst_index
    (unwritten positions keep the poison)."""
    for kind, ncurv, rot in terrain_cases():
        z = terrain_of(ni, nj, kind)
        want = terrain_reference(ni, nj, ncurv, kind, rot)
        got = host_wind_terrain(z, DX, DY, ncurv, rot=tsh.rotation(ni, nj) if rot else None)
        for name, g, w in zip(("sx", "sy", "curv"), got, want):
            assert_same(g.reshape(z.shape), w, "%dx%d %s ncurv %d rot %s: %s" % (ni, nj, kind, ncurv, rot, name))
    if (ni, nj) == (1, 1):
        for ncurv in NCURVS:
            assert all((p.view(np.uint32) == 0).all() for p in terrain_reference(1, 1, ncurv)[:3]), "a 1 x 1 window gives three zeros"
    z = terrain_of(ni, nj)
    rot = tsh.rotation(ni, nj)
    for name, idx, ndst in tsh._indices(ni, nj)[1:]:
        *planes, todo = np_wind_terrain(z, DX, DY, 3, rot=rot, dst_index=idx, ndst=ndst)
        got = host_wind_terrain(z, DX, DY, 3, rot=rot, dst_index=idx, ndst=ndst)
        for pname, g, w in zip(("sx", "sy", "curv"), got, planes):
            assert_same(g, _through(idx, todo, ndst, w), "%dx%d index %s: %s through dst_index, unwritten positions keep the poison" % (ni, nj, name, pname))
            assert_same(w[todo], terrain_reference(ni, nj, 3, "hills", True)[("sx", "sy", "curv").index(pname)][todo],
                        "a cell's value does not depend on where it is written")


@pytest.mark.parametrize("ncell", ts.NCELLS_HOST)
def test_host_column_equals_the_restatement(ncell):
    """wind_column compiled for the host against np_forcing_wind: physical, NaN / Inf / denormal and mixed operands, both flag values, the
    operands' own maxima and maxima a hundred times too small (every ww of the physical columns still lies in [0.5, 1.5]).  The column
    function reports a change exactly where the restatement does not keep the bits."""
    for which in ("physical", "nasty", "mixed"):
        x = wind_operands(ncell, which)
        for smax, cmax in MAXIMA:
            for flags in (0, TURN):
                what = "n=%d %s maxima %g %g flags %d" % (ncell, which, smax, cmax, flags)
                un, vn, parts = np_forcing_wind(x["u"], x["v"], x["sx"], x["sy"], x["curv"], smax, cmax, flags=flags)
                gu, gv, changed = host_wind_columns(x, smax, cmax, flags)
                assert_same(gu, un, what + ": u")
                assert_same(gv, vn, what + ": v")
                assert (changed == ~parts["keep"]).all(), what
                assert_same(gu[parts["keep"]], x["u"][parts["keep"]], what + ": kept u")
                assert_same(gv[parts["keep"]], x["v"][parts["keep"]], what + ": kept v")
                if which == "physical":
                    ww = parts["ww"][~parts["keep"]]
                    assert (ww >= F(0.5)).all() and (ww <= F(1.5)).all(), (what, ww.min(), ww.max())
                    assert (np.abs(parts["td"][~parts["keep"]]) <= 0.25 * (1 + 16 * EPS)).all()     # 0.5 * 0.5 * |sin|, and s2's roundings
        if which == "physical" and ncell > 1:
            _, _, parts = np_forcing_wind(x["u"], x["v"], x["sx"], x["sy"], x["curv"], *MAXIMA[1])
            ww = parts["ww"][~parts["keep"]]
            assert (ww == F(0.5)).any() or (ww == F(1.5)).any() or (np.abs(parts["os"]) == 0.5).any(), "too small maxima reach the clamp"
            assert parts["keep"].any() and (~parts["keep"]).any()


def test_columns_on_flat_ground_and_calm_columns_keep_their_bits():
    """All-zero terrain planes (+0 and -0) keep the bits of any wind, NaN, Inf and -0 included; a wind of speed zero keeps its bits on any
    terrain."""
    winds = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 3.5, -1e-40, 1e30], F)
    u, v = (t.ravel() for t in np.meshgrid(winds, winds))
    n = u.size
    for zero in (0.0, -0.0):
        x = dict(u=u, v=v, sx=np.full(n, zero, F), sy=np.full(n, -zero, F), curv=np.full(n, zero, F))
        for flags in (0, TURN):
            gu, gv, changed = host_wind_columns(x, 0.5, 0.01, flags)
            assert_same(gu, u, "u on flat ground")
            assert_same(gv, v, "v on flat ground")
            assert not changed.any()
            un, vn, _ = np_forcing_wind(u, v, x["sx"], x["sy"], x["curv"], 0.5, 0.01, flags=flags)
            assert_same(un, u, "restated u on flat ground")
            assert_same(vn, v, "restated v on flat ground")
    calm = np.array([0.0, -0.0], F)
    u, v = (t.ravel() for t in np.meshgrid(calm, calm))
    x = dict(u=u, v=v, sx=np.full(4, 0.3, F), sy=np.full(4, -0.2, F), curv=np.full(4, 0.01, F))
    for flags in (0, TURN):
        gu, gv, changed = host_wind_columns(x, 0.5, 0.01, flags)
        assert_same(gu, u, "calm u")
        assert_same(gv, v, "calm v")
        assert not changed.any()


def test_flat_terrain_gives_zero_words_and_changes_no_record():
    """Every word of the three planes is 0x00000000 whatever the level of the plain, ncurv and the rotation; a record adjusted with them
    is bit-identical to the record."""
    for ni, nj in ((35, 67), (5, 3), (1, 1)):
        for level in (0.0, -0.0, 1234.5):
            z = np.full((nj, ni), level, F)
            for ncurv in NCURVS:
                for rot in (None, tsh.rotation(ni, nj), (-tsh.rotation(ni, nj)[0], tsh.rotation(ni, nj)[1])):
                    *want, _ = np_wind_terrain(z, DX, DY, ncurv, rot=rot)
                    got = host_wind_terrain(z, DX, DY, ncurv, rot=rot)
                    for w, g in zip(want, got):
                        assert (w.view(np.uint32) == 0).all() and (g.view(np.uint32) == 0).all(), (ni, nj, level, ncurv)
            x = wind_operands(ni * nj, "mixed")
            x = dict(x, sx=got[0], sy=got[1], curv=got[2])
            for flags in (0, TURN):
                gu, gv, _ = host_wind_columns(x, 1.0, 1.0, flags)
                assert_same(gu, x["u"], "u")
                assert_same(gv, x["v"], "v")


def test_decomposition():
    """The 2 x 2 cut of the 35 x 67 and 70 x 130 hills with ncurv = 3: with a margin of 3 cells (none at the domain's edges) no word of the
    three planes differs from the whole window's, restated and compiled; with margin 0 some do, so the test can fail (the restatement
    gave 0 differing words at margin 3, and 964 and 1939 at margin 0)."""
    ncurv = 3
    for ni, nj in tsh.BIG:
        z = tsh.terrain(ni, nj)
        whole = np_wind_terrain(z, DX, DY, ncurv)[:3]
        differs = {ncurv: 0, 0: 0}
        for margin in differs:
            for tile, win, idx in tsh._cuts(ni, nj, margin):
                ndst = int(idx.max()) + 1
                *planes, todo = np_wind_terrain(z[win], DX, DY, ncurv, dst_index=idx, ndst=ndst)
                got = host_wind_terrain(z[win], DX, DY, ncurv, dst_index=idx, ndst=ndst)
                for w, p, g in zip(whole, planes, got):
                    part = p[todo].reshape(w[tile].shape)
                    differs[margin] += int((part.view(np.uint32) != w[tile].view(np.uint32)).sum())
                    assert_same(g.reshape(part.shape), part, "compiled part, margin %d" % margin)
        print("%d x %d: differing words: margin %d: %d, margin 0: %d" % (ni, nj, ncurv, differs[ncurv], differs[0]))
        assert differs[ncurv] == 0
        assert differs[0] > 0


def _micromet64(z, dx, dy, ncurv, u, v, gamma_s, gamma_c):
    """MicroMet as published (Liston and Elder 2006, eqs. 12-20) in float64 from the float32 inputs, the angles taken through atan2, with
    the issue's one difference: the maxima are those of the slope angle and of |curv| over the window, not of Omega_s per step.  Gradients
    and curvature with the clamped neighbours of the header text."""
    z = z.astype(np.float64)
    nj, ni = z.shape
    jj, ii = np.meshgrid(np.arange(nj), np.arange(ni), indexing="ij")
    ie, iw, jn, js = np.minimum(ii + 1, ni - 1), np.maximum(ii - 1, 0), np.minimum(jj + 1, nj - 1), np.maximum(jj - 1, 0)
    gx = (z[jj, ie] - z[jj, iw]) / ((ie - iw) * dx)
    gy = (z[jn, ii] - z[js, ii]) / ((jn - js) * dy)
    beta = np.arctan(np.hypot(gx, gy))
    xi = 1.5 * np.pi - np.arctan2(gy, gx)                                  # the aspect
    E, W, N, S = np.minimum(ii + ncurv, ni - 1), np.maximum(ii - ncurv, 0), np.minimum(jj + ncurv, nj - 1), np.maximum(jj - ncurv, 0)
    d = ncurv * np.hypot(dx, dy)
    curv = 0.25 * ((z - 0.5 * (z[jj, W] + z[jj, E])) / (2 * ncurv * dx) + (z - 0.5 * (z[S, ii] + z[N, ii])) / (2 * ncurv * dy) +
                   (z - 0.5 * (z[S, W] + z[N, E])) / (2 * d) + (z - 0.5 * (z[N, W] + z[S, E])) / (2 * d))
    u, v = u.astype(np.float64), v.astype(np.float64)
    speed = np.hypot(u, v)
    theta = np.arctan2(-u, -v)                                             # the direction the wind comes from: u = -W sin, v = -W cos
    os_ = np.clip(beta * np.cos(theta - xi) / (2 * beta.max()), -0.5, 0.5)
    oc = np.clip(curv / (2 * np.abs(curv).max()), -0.5, 0.5)
    ww = 1.0 + gamma_s * os_ + gamma_c * oc
    td = -0.5 * os_ * np.sin(2.0 * (xi - theta))
    speed2, theta2 = speed * ww, theta + td
    return -speed2 * np.sin(theta2), -speed2 * np.cos(theta2), beta.max(), np.abs(curv).max()


# Where the bound of test_against_micromet_as_published comes from, counted from the rounded operations of the header text in units of
# 2^-24 relative to the speed W.  A rounding contributes at most one unit relative to its own result; atanf, sinf and cosf count one each.
#   The slope vector: dz is exact to one unit, len, the quotient: 3 per component; g2 (3, entering g by half), g, beta, q, ge*q: the
#     vector carries at most 3 + 1.5 + 4 < 9 units of beta.
#   Omega_s: W2 (3, by half into W), dot (two products and a sum, relative to |u||sx| + |v||sy| <= 1.42 W beta: 3 * 1.42 + the 9 of the slope
#     vector), r, os (ds is a doubling: exact): below 17 units of a number of at most 0.5, so gamma_s * 0.5 * 17 < 5 units of ww.
#   Omega_c: the sum a + b of two heights below 4096 m (asserted) is rounded by at most 8192 units of a metre, over 2 L >= 6000 m and over
#     2 curv_max >= 0.1 (asserted): below 14 units of oc per term, a quarter of four of them; the other roundings of a term, the three sums,
#     the quarter and the division stay relative to numbers of at most curv_max: 7 units of 0.5.  gamma_c * (14 + 3.5) < 8 units of ww.
#   ww: a, b and two sums: 4.  The turn: td <= 0.25 carries the 17 units of os and those of s2 (dot as above, cr likewise, n, m with W2 and
#     b2, the quotient: below 40), so 0.25 * 57 < 15 units of an angle, which is an error relative to the speed; ct, st, four products, two
#     sums and the product with ww: 9.
#   In all 5 + 8 + 4 + 15 + 9 = 41, asserted as 41.  (The float64 side's own error is below 2^-45.)
MICROMET_BOUND = 41


@pytest.mark.parametrize("ni, nj", tsh.BIG)
def test_against_micromet_as_published(ni, nj):
    """The restatement's u', v' on the hills, winds uniform in [-8, 8], maxima from the window, against float64 MicroMet with explicit
    angles, relative to the speed; the bound is counted above (the restatement measured 2.9 and 3.3 * 2^-24).  Asserted on the restatement
    alone so that the inputs cannot hide a no-op: more than a tenth of the columns have |ww - 1| > 0.05, ww stays in [0.5, 1.5], and some
    |td| exceeds 0.1."""
    ncurv = 3
    z = tsh.terrain(ni, nj)
    r = np.random.default_rng(ni + nj)
    u, v = (r.uniform(-8.0, 8.0, z.shape).astype(F) for _ in range(2))
    sx, sy, curv, _ = np_wind_terrain(z, DX, DY, ncurv)
    smax, cmax = window_maxima(sx, sy, curv)
    un, vn, parts = np_forcing_wind(u, v, sx, sy, curv, smax, cmax)
    u64, v64, smax64, cmax64 = _micromet64(z, DX, DY, ncurv, u, v, GAMMA_S, GAMMA_C)
    assert abs(smax / smax64 - 1) < 16 * EPS and abs(cmax / cmax64 - 1) < 1e-4
    assert float(z.max()) < 4096.0 and cmax >= 0.05, (z.max(), cmax)             # what the counted bound assumes
    speed = np.hypot(u.astype(np.float64), v.astype(np.float64)).ravel()
    err = np.maximum(np.abs(un - u64.ravel()), np.abs(vn - v64.ravel())) / speed
    ww, td = parts["ww"], parts["td"]
    share = float((np.abs(ww - 1) > 0.05).mean())
    print("%d x %d: %.2f * 2^-24 relative to the speed (bound %d); |ww - 1| > 0.05 in %.2f of the columns; td %.2f .. %.2f"
          % (ni, nj, err.max() / EPS, MICROMET_BOUND, share, td.min(), td.max()))
    assert err.max() <= MICROMET_BOUND * EPS, err.max() / EPS
    assert share > 0.1
    assert (ww >= F(0.5)).all() and (ww <= F(1.5)).all()
    assert np.abs(td).max() > 0.1
    gu, gv, _ = host_wind_columns(dict(u=u, v=v, sx=sx, sy=sy, curv=curv), smax, cmax, TURN)
    assert_same(gu, un, "compiled u")
    assert_same(gv, vn, "compiled v")


def test_tilted_plane():
    """z = a*dx*i (50 i, 300 i, 1000 i: exact in float32): interior cells have sx = atan(a), sy = 0 within 9 * 2^-24 relative (the quotient
    1; g2 1, entering g by half; g 1: 2.5 on g; atanf's own 1 on top of them: 3.5 on beta; q = beta / g: 3.5 + 2.5 + 1 = 7; ge*q: 7 + 1
    + 1 = 9), and curv is 0 within the rounding of a*dx*i: 4 terms of one unit of the largest height over 2 L.  With slope_max = atan(a) wind straight upslope gets ww = 1 + 0.5 gamma_s and downslope 1 - 0.5 gamma_s
    within 4 * 2^-24 (r, os, a, the sum) plus the slope's; cross-slope wind gets ww = 1 and no turn exactly; wind at 45 degrees is turned
    away from the upslope direction."""
    ni, nj, dx = 31, 31, 1000.0
    jj, ii = np.meshgrid(np.arange(nj), np.arange(ni), indexing="ij")
    for a in (0.05, 0.3, 1.0):
        z = (a * dx * ii).astype(F)
        for ncurv in (1, 3):
            sx, sy, curv, _ = np_wind_terrain(z, dx, dx, ncurv)
            got = host_wind_terrain(z, dx, dx, ncurv)
            for g, w in zip(got, (sx, sy, curv)):
                assert_same(g.reshape(z.shape), w, "plane a %g ncurv %d" % (a, ncurv))
            inner = (slice(ncurv, nj - ncurv), slice(ncurv, ni - ncurv))
            want = np.arctan(a)
            err = np.abs(sx[inner].astype(np.float64) / want - 1).max()
            cerr = np.abs(curv[inner]).max()
            cbound = 4 * (float(z.max()) * EPS) / (2 * ncurv * dx)
            print("a %g ncurv %d: sx %.2f * 2^-24 (bound 9), |curv| %.3g (bound %.3g)" % (a, ncurv, err / EPS, cerr, cbound))
            assert err <= 9 * EPS
            assert (sy[inner] == 0).all()
            assert cerr <= cbound
        # the column function on an exact slope vector: beta along +x, no curvature
        beta = F(want)
        one = lambda u, v, flags=TURN: np_forcing_wind([u], [v], [beta], [0.0], [0.0], beta, 1.0, flags=flags)      # noqa: E731
        un, vn, p = one(5.0, 0.0)
        assert abs(float(p["ww"][0]) - (1 + 0.5 * GAMMA_S)) <= 4 * EPS and vn[0] == 0 and abs(un[0] / 5.0 - (1 + 0.5 * GAMMA_S)) <= 6 * EPS
        un, vn, p = one(-5.0, 0.0)
        assert abs(float(p["ww"][0]) - (1 - 0.5 * GAMMA_S)) <= 4 * EPS and vn[0] == 0
        for flags in (0, TURN):
            un, vn, p = one(0.0, 5.0, flags)
            assert p["ww"][0] == 1 and p["td"][0] == 0 and un[0] == 0 and vn[0] == F(5.0)
        un, vn, p = one(3.0, 3.0)                                         # blowing to the north-east, upslope is east
        assert p["td"][0] != 0 and vn[0] / un[0] > 1.0, "turned away from the upslope direction (towards north)"
        un, vn, p = one(3.0, -3.0)
        assert vn[0] / un[0] < -1.0, "turned away from the upslope direction (towards south)"
        gu, gv, _ = host_wind_columns(dict(u=[3.0], v=[3.0], sx=[beta], sy=[0.0], curv=[0.0]), beta, 1.0, TURN)
        un, vn, _ = one(3.0, 3.0)
        assert_same(gu, un, "compiled")
        assert_same(gv, vn, "compiled")


def test_gaussian_hill():
    """curv > 0 on the crest of a Gaussian hill and < 0 at its foot; the slope vector points uphill, towards the crest."""
    n, dx, ncurv = 41, 1000.0, 3
    jj, ii = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    c = n // 2
    z = (800.0 * np.exp(-((ii - c) ** 2 + (jj - c) ** 2) / (2.0 * 4.0 ** 2))).astype(F)
    sx, sy, curv, _ = np_wind_terrain(z, dx, dx, ncurv)
    assert curv[c, c] > 0 and curv[c, c] == curv.max()
    assert curv[c, c + 8] < 0 and curv[c + 8, c] < 0 and curv[c - 6, c - 6] < 0
    assert sx[c, c + 5] < 0 and sx[c, c - 5] > 0 and sy[c + 5, c] < 0 and sy[c - 5, c] > 0
    assert sx[c, c] == 0 and sy[c, c] == 0
    for g, w in zip(host_wind_terrain(z, dx, dx, ncurv), (sx, sy, curv)):
        assert_same(g.reshape(z.shape), w, "hill")


def _terrain_block(z, out, **kw):
    b = abi.WindTerrain()
    b.height, b.sx, b.sy, b.curv = z.ctypes.data, out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data
    b.cosalpha = b.sinalpha = b.dst_index = None
    b.nj, b.ni = z.shape
    b.ncurv, b.dx, b.dy = 3, DX, DY
    for k, v in kw.items():
        setattr(b, k, v)
    return b


def _wind_block(planes, **kw):
    b = abi.Wind()
    for k in ("u", "v", "sx", "sy", "curv"):
        setattr(b, k, planes[k].ctypes.data)
    b.slope_max, b.curv_max, b.gamma_s, b.gamma_c, b.flags = 0.5, 0.01, GAMMA_S, GAMMA_C, TURN
    for k, v in kw.items():
        setattr(b, k, v)
    return b


def test_refusals_write_nothing():
    """Every refusal returns -105 with text before anything is launched or read: the planes here are host memory that the calls must not
    touch, and they keep their poison.  Empty calls are served where a device is present (the GPU tests)."""
    lib = abi.load_library()
    ni, nj = 5, 3
    z = np.full((nj, ni), POISON, F)
    out = [np.full(ni * nj, POISON, F) for _ in range(3)]
    rotp = np.full((nj, ni), POISON, F)

    def call(b, ndst=ni * nj):
        rc = lib.noahmp_hip_wind_terrain(C.byref(b) if b is not None else None, ndst, None)
        return rc, lib.noahmp_hip_last_error().decode()
    rc, msg = call(None)
    assert rc == -105 and "NULL" in msg and "noahmp_hip_wind_terrain" in msg
    for field in ("height", "sx", "sy", "curv"):
        rc, msg = call(_terrain_block(z, out, **{field: None}))
        assert rc == -105 and "required" in msg, (field, rc, msg)
    for kw in (dict(cosalpha=rotp.ctypes.data), dict(sinalpha=rotp.ctypes.data)):
        rc, msg = call(_terrain_block(z, out, **kw))
        assert rc == -105 and "both or none" in msg, (kw, rc, msg)
    for kw, word in ((dict(ncurv=0), "ncurv"), (dict(ncurv=65), "ncurv"), (dict(ncurv=-1), "ncurv"), (dict(dx=0.0), "dx"), (dict(dx=-1.0), "dx"),
                     (dict(dx=float("nan")), "dx"), (dict(dy=float("inf")), "dy"), (dict(dy=0.0), "dy"), (dict(ni=-1), "ni"), (dict(nj=-1), "nj"),
                     (dict(ni=65536, nj=32768), "ni")):
        rc, msg = call(_terrain_block(z, out, **kw))
        assert rc == -105 and word in msg, (kw, rc, msg)
    for ndst in (-1, 2 ** 31):
        rc, msg = call(_terrain_block(z, out), ndst=ndst)
        assert rc == -105 and "ndst" in msg, (ndst, rc, msg)
    n = 16
    planes = {k: np.full(n, POISON, F) for k in ("u", "v", "sx", "sy", "curv")}

    def wcall(b, nc=n):
        rc = lib.noahmp_hip_forcing_wind(C.byref(b) if b is not None else None, nc, None)
        return rc, lib.noahmp_hip_last_error().decode()
    rc, msg = wcall(None)
    assert rc == -105 and "NULL" in msg and "noahmp_hip_forcing_wind" in msg
    for field in ("u", "v", "sx", "sy", "curv"):
        rc, msg = wcall(_wind_block(planes, **{field: None}))
        assert rc == -105 and "required" in msg, (field, rc, msg)
    for field in ("slope_max", "curv_max"):
        for bad in (0.0, -0.5, float("nan"), float("inf")):
            rc, msg = wcall(_wind_block(planes, **{field: bad}))
            assert rc == -105 and field in msg, (field, bad, rc, msg)
    for nc in (-1, 2 ** 31):
        rc, msg = wcall(_wind_block(planes), nc=nc)
        assert rc == -105 and "ncell" in msg
    assert (z == POISON).all() and all((o == POISON).all() for o in out) and all((p == POISON).all() for p in planes.values())


HEADER_LINES = (
    "typedef struct noahmp_wind_terrain {", "} noahmp_wind_terrain;", "typedef struct noahmp_wind {", "} noahmp_wind;",
    "#define NOAHMP_HIP_HAS_FORCING_WIND 1\n", "#define NOAHMP_WIND_MAX_NCURV 64\n", "#define NOAHMP_HIP_ABI_MINOR 3\n", "#define NOAHMP_WIND_TURN ",
    "noahmp_hip_wind_terrain(const noahmp_wind_terrain* wt, int64_t ndst, void* stream);",
    "noahmp_hip_forcing_wind(const noahmp_wind* w, int64_t ncell, void* stream);",
    "ie = min(i+1, ni-1);  iw = max(i-1, 0);  jn = min(j+1, nj-1);  js = max(j-1, 0)",
    "gx = (ie == iw) ? 0 : (z[j][ie] - z[j][iw]) / ((float)(ie-iw) * dx)",
    "gy = (jn == js) ? 0 : (z[jn][i] - z[js][i]) / ((float)(jn-js) * dy)",
    "ge = gx*ca - gy*sa;  gn = gy*ca + gx*sa",
    "g2 = ge*ge + gn*gn;  g = sqrtf(g2);  beta = atanf(g);  q = beta / g",
    "sx = (g == 0) ? 0 : ge*q;  sy = (g == 0) ? 0 : gn*q",
    "E = min(i+ncurv, ni-1);  W = max(i-ncurv, 0);  N = min(j+ncurv, nj-1);  S = max(j-ncurv, 0)",
    "lx = (float)ncurv*dx;  ly = (float)ncurv*dy;  d2 = dx*dx + dy*dy;  d = (float)ncurv * sqrtf(d2)",
    "t1 = (z - 0.5f*(z[j][W] + z[j][E])) / (2.0f*lx)", "t2 = (z - 0.5f*(z[S][i] + z[N][i])) / (2.0f*ly)",
    "t3 = (z - 0.5f*(z[S][W] + z[N][E])) / (2.0f*d)", "t4 = (z - 0.5f*(z[N][W] + z[S][E])) / (2.0f*d)",
    "curv = 0.25f * (((t1 + t2) + t3) + t4)",
    "If sx == 0 && sy == 0 && curv == 0: the column keeps its bits.", "W2 = u*u + v*v;  W = sqrtf(W2).  If W == 0: the column keeps its bits.",
    "dot = u*sx + v*sy;  r = dot / W;  ds = slope_max + slope_max;  os = r / ds;", "dc = curv_max + curv_max;  oc = curv / dc;",
    "a = gamma_s*os;  b = gamma_c*oc;  ww = (1.0f + a) + b", "u[c] = ww*u;  v[c] = ww*v",
    "b2 = sx*sx + sy*sy;  cr = sx*v - sy*u;  n = 2.0f*dot;  n = n*cr;  m = W2*b2",
    "s2 = (b2 == 0) ? 0 : n / m;  h = -0.5f*os;  td = h*s2",
    "ct = cosf(td);  st = sinf(td);  u[c] = ww*(u*ct + v*st);  v[c] = ww*(v*ct - u*st)",
    "DELIBERATE DIFFERENCE FROM MICROMET", "within max(1, ncurv) of its own", "CLAMPED INTO THE WINDOW")


def test_bindings_regenerate_identically_with_the_wind_calls():
    from tools import gen_abi
    for rel, text in (("include/noahmp_hip.h", gen_abi.c_header()), ("oracle/ref_harness_gen.f90", gen_abi.ref_harness()),
                      ("noahmp_amd/fortran/module_sf_noahmpdrv_hip.F90", gen_abi.fortran_shim()),
                      ("tests/fortran/shim_wrap_gen.f90", gen_abi.shim_wrap())):
        assert open(os.path.join(ROOT, rel)).read() == text, rel
    hdr = open(os.path.join(ROOT, "include", "noahmp_hip.h")).read()
    for word in HEADER_LINES:
        assert word in hdr, word
    assert "".join(gen_abi.wind_header()) != "" and "\n".join(gen_abi.wind_header()) in hdr
    assert "noahmp_wind" not in gen_abi.ref_harness()
    f90 = open(os.path.join(ROOT, "noahmp_amd", "fortran", "module_sf_noahmpdrv_hip.F90")).read()
    for word in ("bind(C, name='noahmp_hip_wind_terrain')", "bind(C, name='noahmp_hip_forcing_wind')", "type, bind(C) :: noahmp_wind_terrain",
                 "type, bind(C) :: noahmp_wind ", "NOAHMP_WIND_MAX_NCURV = 64", "NOAHMP_WIND_TURN = 1"):
        assert word in f90, word
    assert "noahmp_hip_wind_terrain" in abi.EXPORTED_SYMBOLS and "noahmp_hip_forcing_wind" in abi.EXPORTED_SYMBOLS
    assert [n for n, _ in abi.WindTerrain._fields_] == ["height", "cosalpha", "sinalpha", "dst_index", "sx", "sy", "curv", "ni", "nj", "ncurv", "dx", "dy"]
    assert [n for n, _ in abi.Wind._fields_] == ["u", "v", "sx", "sy", "curv", "slope_max", "curv_max", "gamma_s", "gamma_c", "flags"]
    assert abi.WIND_FLAG == {"turn": 1}


def test_ctypes_mirrors_match_the_compiled_header(tmp_path):
    body, want = "", []
    for cname, cls in (("noahmp_wind_terrain", abi.WindTerrain), ("noahmp_wind", abi.Wind)):
        names = [n for n, _ in cls._fields_]
        body += 'printf(" %%zu", sizeof(%s));' % cname + "".join('printf(" %%zu", offsetof(%s, %s));' % (cname, n) for n in names)
        want += [C.sizeof(cls)] + [getattr(cls, n).offset for n in names]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "noahmp_hip.h"\nint main(){' + body +
                   'printf(" %d %d %d %d", NOAHMP_HIP_ABI_MINOR, NOAHMP_HIP_HAS_FORCING_WIND, NOAHMP_WIND_MAX_NCURV, NOAHMP_WIND_TURN); return 0;}')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert out == want + [3, 1, 64, 1]


def test_library_exports_the_wind_calls():
    if not os.path.exists(abi.LIB_PATH):
        from noahmp_amd import build as b
        b.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", abi.LIB_PATH]).decode()
    assert " T noahmp_hip_wind_terrain\n" in out and " T noahmp_hip_forcing_wind\n" in out


@pytest.mark.skipif(tr._flang() is None, reason="no flang")
def test_generated_fortran_types_and_interfaces_compile(tmp_path):
    """The wind part of the generated module compiles, and a caller of both interfaces type-checks."""
    from tools import gen_abi
    text = "\n".join(["module wind_abi_check", "  use iso_c_binding", "  implicit none"] + gen_abi.wind_f90_types() + ["  interface"] +
                     gen_abi.wind_f90_interfaces() +
                     ["  end interface", "contains", "  function go(ncell, planes) result(rc)", "    integer(c_int64_t), value :: ncell",
                      "    type(c_ptr), intent(in) :: planes(6)", "    type(noahmp_wind_terrain) :: wt", "    type(noahmp_wind) :: w",
                      "    integer(c_int) :: rc",
                      "    wt%height = planes(1); wt%cosalpha = c_null_ptr; wt%sinalpha = c_null_ptr; wt%dst_index = c_null_ptr",
                      "    wt%sx = planes(2); wt%sy = planes(3); wt%curv = planes(4); wt%ni = 64; wt%nj = 8",
                      "    wt%ncurv = min(3, NOAHMP_WIND_MAX_NCURV); wt%dx = 1000.0; wt%dy = 1000.0",
                      "    rc = noahmp_hip_wind_terrain(wt, ncell, c_null_ptr)",
                      "    w%u = planes(5); w%v = planes(6); w%sx = planes(2); w%sy = planes(3); w%curv = planes(4)",
                      "    w%slope_max = 0.6; w%curv_max = 0.02; w%gamma_s = 0.58; w%gamma_c = 0.42; w%flags = NOAHMP_WIND_TURN",
                      "    rc = noahmp_hip_forcing_wind(w, ncell, c_null_ptr)",
                      "  end function go", "end module wind_abi_check", ""])
    f = tmp_path / "wind_abi_check.f90"
    f.write_text(text)
    subprocess.check_call([tr._flang(), "-c", str(f), "-o", str(tmp_path / "wind_abi_check.o"), "-J", str(tmp_path)], cwd=str(tmp_path))


# ---------------------------------------------------------------------------------------------------------------- GPU
_dev = tr._dev
PAD = 5                                                                 # destinations start at an odd offset inside the pool


@pytest.mark.gpu
@pytest.mark.parametrize("ni, nj", WINDOWS_GPU)
def test_gpu_terrain_kernel_equals_the_restatement(engine, ni, nj):
    """noahmp_hip_wind_terrain against np_wind_terrain: ncurv 1 / 3 / 64, with and without rotation, the nasty terrain; identity, permuted
    and margin dst_index (the margin's positions keep the poison).  35 x 67 = 2345 cells end in a ragged workgroup and a ragged wave.
    Destinations are offset by five floats inside a poisoned pool whose guard words keep the poison.  Empty calls write nothing."""
    import torch
    ncell = ni * nj
    pool = torch.full((3, ncell + 9), POISON, dtype=torch.float32, device="cuda")
    dst = [pool[k, PAD:PAD + ncell] for k in range(3)]
    torch.cuda.synchronize()
    rotd = tuple(_dev(t) for t in tsh.rotation(ni, nj))
    for kind, ncurv, rot in terrain_cases():
        zd = _dev(terrain_of(ni, nj, kind))
        want = terrain_reference(ni, nj, ncurv, kind, rot)[:3]
        for name, idx, ndst in (tsh._indices(ni, nj) if ncurv == 3 else tsh._indices(ni, nj)[:1]):
            idxd = _dev(idx) if idx is not None else None
            pool.fill_(POISON)
            torch.cuda.synchronize()
            b = engine.wind_terrain_block(zd, *dst, DX, DY, ncurv=ncurv, cosalpha=rotd[0] if rot else None, sinalpha=rotd[1] if rot else None,
                                          dst_index=idxd)
            engine.wind_terrain(b, ndst)
            engine.stream_sync()
            h = pool.cpu().numpy()
            what = "%dx%d %s ncurv %d rot %s index %s" % (ni, nj, kind, ncurv, rot, name)
            flat_idx = np.arange(ncell) if idx is None else idx.ravel().astype(np.int64)
            ok = (flat_idx >= 0) & (flat_idx < ndst)
            for k, pname in enumerate(("sx", "sy", "curv")):
                w = np.full(ncell, POISON, F)
                w[flat_idx[ok]] = want[k].ravel()[ok]
                assert_same(h[k, PAD:PAD + ncell], w, what + ": " + pname)
            assert (h[:, :PAD] == POISON).all() and (h[:, PAD + ncell:] == POISON).all(), what + ": guard words"
    pool.fill_(POISON)
    torch.cuda.synchronize()
    zd = _dev(terrain_of(ni, nj))
    engine.wind_terrain(engine.wind_terrain_block(zd, *dst, DX, DY, ncurv=3), 0)
    b = engine.wind_terrain_block(zd, *dst, DX, DY, ncurv=3)
    b.nj = 0                                                             # an empty window
    engine.wind_terrain(b, ncell)
    engine.stream_sync()
    assert (pool.cpu().numpy() == POISON).all()


@pytest.mark.gpu
def test_gpu_terrain_of_a_cut_window_equals_the_whole(engine):
    """70 x 130 cut 2 x 2 with a margin of ncurv = 3 cells: every part has the bits of the undecomposed launch and of the restatement."""
    import torch
    ni, nj, ncurv = 70, 130, 3
    z = terrain_of(ni, nj)
    whole = [torch.full((nj, ni), POISON, dtype=torch.float32, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()
    engine.wind_terrain(engine.wind_terrain_block(_dev(z), *whole, DX, DY, ncurv=ncurv), ni * nj)
    engine.stream_sync()
    whole_h = [t.cpu().numpy() for t in whole]
    for g, w in zip(whole_h, terrain_reference(ni, nj, ncurv)[:3]):
        assert_same(g, w, "the whole window")
    for tile, win, idx in tsh._cuts(ni, nj, ncurv):
        ndst = int(idx.max()) + 1
        part = [torch.full((ndst,), POISON, dtype=torch.float32, device="cuda") for _ in range(3)]
        torch.cuda.synchronize()
        engine.wind_terrain(engine.wind_terrain_block(_dev(z[win]), *part, DX, DY, ncurv=ncurv, dst_index=_dev(idx)), ndst)
        engine.stream_sync()
        for p, w in zip(part, whole_h):
            assert_same(p.cpu().numpy().reshape(w[tile].shape), w[tile], "part %s" % (tile,))


@pytest.mark.gpu
@pytest.mark.parametrize("ncell", (1, 63, 64, 65, 9100))
def test_gpu_wind_kernel_equals_the_restatement(engine, ncell):
    """noahmp_hip_forcing_wind against np_forcing_wind: physical and nasty operands, both flag values, both pairs of maxima; u and v sit
    at an odd offset inside a poisoned pool whose guard words keep the poison; the terrain planes are not written.  An empty call writes
    nothing."""
    import torch
    pool = torch.full((2, ncell + 9), POISON, dtype=torch.float32, device="cuda")
    ud, vd = pool[0, PAD:PAD + ncell], pool[1, PAD:PAD + ncell]
    for which in ("physical", "nasty"):
        x = wind_operands(ncell, which)
        xd = {k: _dev(t) for k, t in x.items()}
        for smax, cmax in MAXIMA:
            for flags in (0, TURN):
                what = "ncell %d %s maxima %g %g flags %d" % (ncell, which, smax, cmax, flags)
                pool.fill_(POISON)
                ud.copy_(xd["u"])
                vd.copy_(xd["v"])
                torch.cuda.synchronize()
                engine.forcing_wind(engine.wind_block(ud, vd, xd["sx"], xd["sy"], xd["curv"], smax, cmax, gamma_s=GAMMA_S, gamma_c=GAMMA_C,
                                                      turn=bool(flags)), ncell)
                engine.stream_sync()
                h = pool.cpu().numpy()
                un, vn, _ = np_forcing_wind(x["u"], x["v"], x["sx"], x["sy"], x["curv"], smax, cmax, flags=flags)
                assert_same(h[0, PAD:PAD + ncell], un, what + ": u")
                assert_same(h[1, PAD:PAD + ncell], vn, what + ": v")
                assert (h[:, :PAD] == POISON).all() and (h[:, PAD + ncell:] == POISON).all(), what + ": guard words"
        for k in ("sx", "sy", "curv"):
            assert_same(xd[k].cpu().numpy(), x[k], "the terrain planes are read only")
    pool.fill_(POISON)
    torch.cuda.synchronize()
    engine.forcing_wind(engine.wind_block(ud, vd, xd["sx"], xd["sy"], xd["curv"], 0.5, 0.01), 0)
    engine.stream_sync()
    assert (pool.cpu().numpy() == POISON).all()


@pytest.mark.gpu
def test_gpu_refusals_launch_nothing(engine):
    """The refusals with device planes: -105, text, and every plane keeps its poison."""
    import torch
    lib = engine.lib
    ni, nj = 5, 3
    planes = torch.full((9, ni * nj), POISON, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ptr = [planes[k].data_ptr() for k in range(9)]

    def tb(**kw):
        b = abi.WindTerrain()
        b.height, b.sx, b.sy, b.curv = ptr[0], ptr[1], ptr[2], ptr[3]
        b.ni, b.nj, b.ncurv, b.dx, b.dy = ni, nj, 3, DX, DY
        for k, v in kw.items():
            setattr(b, k, v)
        return b

    def wb(**kw):
        b = abi.Wind()
        b.u, b.v, b.sx, b.sy, b.curv = ptr[4], ptr[5], ptr[6], ptr[7], ptr[8]
        b.slope_max, b.curv_max, b.gamma_s, b.gamma_c, b.flags = 0.5, 0.01, GAMMA_S, GAMMA_C, TURN
        for k, v in kw.items():
            setattr(b, k, v)
        return b
    for kw in (dict(height=None), dict(curv=None), dict(cosalpha=ptr[0]), dict(ncurv=0), dict(ncurv=65), dict(dx=0.0), dict(dy=float("nan")),
               dict(ni=-1), dict(ni=65536, nj=32768)):
        assert lib.noahmp_hip_wind_terrain(C.byref(tb(**kw)), ni * nj, None) == -105, kw
        assert "noahmp_hip_wind_terrain" in lib.noahmp_hip_last_error().decode()
    assert lib.noahmp_hip_wind_terrain(C.byref(tb()), -1, None) == -105
    assert lib.noahmp_hip_wind_terrain(None, ni * nj, None) == -105
    for kw in (dict(u=None), dict(sy=None), dict(slope_max=0.0), dict(curv_max=float("inf")), dict(curv_max=-1.0)):
        assert lib.noahmp_hip_forcing_wind(C.byref(wb(**kw)), ni * nj, None) == -105, kw
        assert "noahmp_hip_forcing_wind" in lib.noahmp_hip_last_error().decode()
    assert lib.noahmp_hip_forcing_wind(C.byref(wb()), 2 ** 31, None) == -105
    assert lib.noahmp_hip_forcing_wind(None, ni * nj, None) == -105
    engine.stream_sync()
    torch.cuda.synchronize()
    assert (planes.cpu().numpy() == POISON).all()


VAL_NI, VAL_NJ, VAL_MARGIN, VAL_NCURV = tsv.VAL_NI, tsv.VAL_NJ, tsv.VAL_MARGIN, 3
VAL_STEPS = tsv.VAL_STEPS


def _wind_run(engine, tables, recs_h, height, sort, wind, seen):
    """Two engine steps of the 35 x 67 valley tile: WindTerrain.set_terrain (before the sort) and record() on both records (with wind),
    forcing_interpolate_prep, noahmplsm.  seen[it] receives level 1 of u_phy / v_phy after the interpolation of step it."""
    import torch
    from noahmp_amd import synth
    from noahmp_amd.wind import WindTerrain
    T, tb = tables
    lat, lon_h = tsv._valley_latlon()
    s = synth.mixed_small(tb, ni=VAL_NI, nj=VAL_NJ)
    s.a["xlatin"][...] = lat
    synth.first_step_fixups(s)
    synth.diurnal_forcing(s, 12, t_offset=s.t_offset)
    d = s.to_device("cuda:0")
    lon = _dev(lon_h)
    rain = torch.zeros((VAL_NJ, VAL_NI), dtype=torch.float32, device="cuda:0")
    recs = [{k: _dev(v) for k, v in rec.items()} for rec in recs_h]           # fresh copies: record() works in place
    torch.cuda.synchronize()
    wt = None
    if wind:
        wt = WindTerrain(engine, VAL_NI, VAL_NJ)
        wt.set_terrain(_dev(height), DX, DX, ncurv=VAL_NCURV, origin=(VAL_MARGIN, 0))
    if sort:
        engine.sort_store(d)
        perm = d.sort_perm.long()
        lon = lon.reshape(-1)[perm].reshape(VAL_NJ, VAL_NI).contiguous()
        recs = [{k: v.reshape(-1)[perm].reshape(VAL_NJ, VAL_NI).contiguous() for k, v in r.items()} for r in recs]
        torch.cuda.synchronize()
        if wind:
            wt.follow(d)
    if wind:
        for rec in recs:
            wt.record(rec)
        engine.stream_sync()
    for it in (1, 2):
        now = VAL_STEPS[it - 1]
        jul = engine.forcing_interpolate_prep(d, recs[0], recs[1], 1800 * (it - 1), 10800, rain, lon, *now, scale_vegfra=True, first_step=(it == 1))
        engine.stream_sync()
        seen[it] = {k: d.a[k].cpu().numpy()[:, 0, :].ravel().copy() for k in ("u_phy", "v_phy")}
        st = engine.noahmplsm(d, it, 2000, jul)
        assert st.code == 0
    return d, wt, recs


@pytest.mark.gpu
def test_gpu_engine_run_in_a_valley(engine, tables):
    """Two engine steps on the 35 x 67 valley tile (margin 4 along i, ncurv 3): level 1 of the store's u_phy / v_phy equals the reference's
    linear interpolation (netcdf_io:1369-1403: a*f + b*(1 - f), rounded products) of the restated adjusted records, bit for bit; the run
    on a sorted store after follow(), returned to tile order, equals the unsorted one."""
    height = tsv._valley()
    recs_h, _ = tsv._valley_records()
    seen, seen_sorted = {}, {}
    d, wt, recs = _wind_run(engine, tables, recs_h, height, False, True, seen)
    idx = np.full(height.shape, -1, np.int32)
    idx[:, VAL_MARGIN:VAL_MARGIN + VAL_NI] = np.arange(VAL_NI * VAL_NJ, dtype=np.int32).reshape(VAL_NJ, VAL_NI)
    sx, sy, curv, todo = np_wind_terrain(height, DX, DX, VAL_NCURV, dst_index=idx, ndst=VAL_NI * VAL_NJ)
    for k, (g, w) in enumerate(zip(wt.planes_tile, (sx, sy, curv))):
        assert_same(g.cpu().numpy().ravel(), w[todo], "plane %d of set_terrain" % k)
    smax, cmax = window_maxima(sx, sy, curv)                             # the defaults: over the WINDOW, margin included
    assert abs(wt.slope_max / smax - 1) <= 4 * EPS and abs(wt.curv_max / cmax - 1) <= 4 * EPS, (wt.slope_max, smax, wt.curv_max, cmax)
    adj = []
    changed = 0
    for k, rec in enumerate(recs_h):
        un, vn, parts = np_forcing_wind(rec["u"], rec["v"], sx[todo], sy[todo], curv[todo], wt.slope_max, wt.curv_max)
        assert_same(recs[k]["u"].cpu().numpy().ravel(), un, "u of record %d after record()" % k)
        assert_same(recs[k]["v"].cpu().numpy().ravel(), vn, "v of record %d after record()" % k)
        changed += int((un != rec["u"].ravel()).sum())
        assert (np.abs(parts["ww"] - 1) > 0.05).mean() > 0.3 and np.abs(parts["td"]).max() > 0.02, "the valley adjusts the wind"
        adj.append((un, vn))
    assert changed > VAL_NI * VAL_NJ
    for it in (1, 2):
        f = F(10800 - 1800 * (it - 1)) / F(10800)
        g = F(1.0) - f
        assert_same(seen[it]["u_phy"], adj[0][0] * f + adj[1][0] * g, "u_phy of step %d" % it)
        assert_same(seen[it]["v_phy"], adj[0][1] * f + adj[1][1] * g, "v_phy of step %d" % it)
    ds, wts, _ = _wind_run(engine, tables, recs_h, height, True, True, seen_sorted)
    perm = ds.sort_perm.cpu().numpy()
    assert (perm != np.arange(perm.size)).any()
    for it in (1, 2):
        for k in ("u_phy", "v_phy"):
            assert_same(seen_sorted[it][k], seen[it][k][perm], "%s of the sorted run, step %d" % (k, it))
    for g, w in zip(wts.planes, wt.planes_tile):
        assert_same(g.cpu().numpy().ravel(), w.cpu().numpy().ravel()[perm], "follow() permutes the planes")


@pytest.mark.gpu
def test_gpu_engine_run_on_flat_terrain(engine, tables):
    """The same two steps on the flat valley: every array of the store is bit-identical to the run without WindTerrain."""
    from tools.compare import exact_check
    height = tsv._valley(flat=True)
    recs_h, _ = tsv._valley_records()
    a, b = {}, {}
    with_wind, wt, _ = _wind_run(engine, tables, recs_h, height, False, True, a)
    without, _, _ = _wind_run(engine, tables, recs_h, height, False, False, b)
    assert all((t.cpu().numpy().view(np.uint32) == 0).all() for t in wt.planes_tile)
    ok, lines = exact_check(without.to_host(), with_wind.to_host())
    assert ok, "\n".join(lines)
    for it in (1, 2):
        for k in ("u_phy", "v_phy"):
            assert_same(a[it][k], b[it][k], k)
