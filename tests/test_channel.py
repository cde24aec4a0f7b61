"""Kinematic-wave routing with Manning friction on the D8 network (noahmp_hip_flow_channel, noahmp_hip_route_kinematic;
nmp_dev_channel.hpp; routing.ChannelFlow).

No reference routine stands behind the calls; the contract is the text in include/noahmp_hip.h.  np_flow_channel and np_route_kinematic
restate it in numpy, one rounded float32 operation per line, with glibc's own powf called per element through ctypes.  Everything is
compared with the restatement bit for bit (test_regrid.assert_same: equal bits, or both NaN): the per-cell functions compiled for the
host, both kernels, and engine runs through ChannelFlow.  diag[0] holds float32 bits and is compared as a float (a NaN is a NaN whatever
its payload); diag[1] is compared as a word.  A tolerance appears only in the budget check; where it comes from is counted there."""
import ctypes as C
import functools
import json
import os
import subprocess

import numpy as np
import pytest

from noahmp_amd import abi
import test_regrid as tr
import test_routing as trt
import test_shadow as tsh
import test_skyview as tsv
from test_regrid import F, assert_same, nasty
from test_routing import CUT, DX, DY, EPS, POISON, U32, WINDOWS, neighbour, np_flow_dir, np_inmask, np_inverse_distances, np_slopes

ROOT = tr.ROOT
CSRC = tr.CSRC
SRC = os.path.join(ROOT, "tests", "host_emul", "channel_check.hip")
LIB = os.path.join(ROOT, "tests", "host_emul", "libchannel_check.so")
HEADER = os.path.join(ROOT, "include", "noahmp_hip.h")
REFUSAL_FIXTURE = os.path.join(ROOT, "tests", "golden", "channel_refusal_text.json")
SMIN = 1e-4
DT = 600.0                                                               # seconds per call of the bit-for-bit runs
SCALE = float(F(F(DT) * F(1e-3)))
TWO_THIRDS = np.array([0x3F2AAAAB], U32).view(F)[0]

_libm = C.CDLL("libm.so.6")
_libm.powf.restype = C.c_float
_libm.powf.argtypes = [C.c_float, C.c_float]


def powf(x, y):
    return np.array([_libm.powf(float(a), float(y)) for a in x], F)


# ---------------------------------------------------------------------------------------------------------------- the restatement
def np_diagonal(dx, dy):
    dx, dy = F(dx), F(dy)
    dx2 = F(dx * dx)
    dy2 = F(dy * dy)
    d2 = F(dx2 + dy2)
    return F(np.sqrt(d2))


def np_flow_channel(dirp, manning, dx, dy, smin, height=None, slope=None):
    """noahmp_hip_flow_channel over a window: (length, conv, s) -- s is the slope before the floor, for the identity test."""
    assert (height is None) != (slope is None)
    d = np.asarray(dirp, np.uint8)
    k = np.where(d > 8, 0, d).astype(np.int64)
    n = np.asarray(manning, F)
    smin = F(smin)
    length = np.where((k == 0) | (k == 1) | (k == 5), F(dx), np.where((k == 3) | (k == 7), F(dy), np_diagonal(dx, dy))).astype(F)
    with np.errstate(all="ignore"):
        if slope is not None:
            s = np.asarray(slope, F)
        else:
            s = np.full(d.shape, smin, F)
            for kk, (sk, inside) in enumerate(np_slopes(height, dx, dy), start=1):
                s = np.where((k == kk) & inside, sk, s).astype(F)
        sf = np.where(s > smin, s, smin).astype(F)
        r = np.sqrt(sf)
        cv = r / n
        conv = np.where(n > 0, cv, F(0.0)).astype(F)
    assert all(t.dtype == F for t in (length, s, sf, r, cv, conv))
    return length, conv, s


def bits_of(cr):
    return np.asarray(cr, F).view(U32)


def np_route_kinematic(x, out_old, out_new, storage, depth=None, diag=None):
    """One call of noahmp_hip_route_kinematic over the window of x (a dict of the block's members): (storage', out_new', depth', diag').
    depth / diag None: not given to the call."""
    m = np.asarray(x["inmask"], np.uint8)
    col = np.asarray(x["col_index"], np.int64)
    ncol = int(x["ncol"])
    owned = (col >= -1) & (col < ncol)
    local = owned & (col >= 0)
    scale, dt = F(x["scale"]), F(x["dt"])
    width, length, conv = (np.asarray(x[k], F) for k in ("width", "length", "conv"))
    with np.errstate(all="ignore"):
        q = np.zeros(m.shape, F)
        for k in range(1, 9):
            on, inside = neighbour(np.asarray(out_old, F), k)
            take = inside & ((m >> (k - 1)) & 1).astype(bool)
            qk = q + on
            q = np.where(take, qk, q).astype(F)
        d = np.where(local, col, 0)
        xa = np.asarray(x["runoff_a"], F).ravel()[d] if ncol else np.zeros(m.shape, F)
        if x.get("runoff_b") is not None and ncol:
            xa = xa + np.asarray(x["runoff_b"], F).ravel()[d]
        xs = xa * scale
        v = np.where(local, xs * np.asarray(x["area"], F), F(0.0)).astype(F)
        sv = np.asarray(storage, F) + v
        s1 = sv + q
        enter = owned & (s1 > 0) & (conv > 0)
        wl = width * length
        h = s1 / wl
        a = width * h
        h2 = h + h
        p = width + h2
        R = a / p
        r23 = np.zeros(m.shape, F)
        r23[enter] = powf(R[enter], TWO_THIRDS)
        vel = conv * r23
        qa = vel * a
        od = qa * dt
        capped = enter & ~(od < s1)
        o = np.where(enter, np.where(capped, s1, od), F(0.0)).astype(F)
        vd = vel * dt
        cr = np.where(enter, vd / length, F(0.0)).astype(F)
        h = np.where(enter, h, F(0.0)).astype(F)
        snew = s1 - o
    assert all(t.dtype == F for t in (q, xs, v, sv, s1, wl, h, a, h2, p, R, vel, qa, od, o, vd, cr, snew))
    if depth is not None:
        depth = np.where(owned, h, depth).astype(F)
    if diag is not None:
        show = owned & ((cr > 0) | np.isnan(cr))
        diag = np.array([max(int(diag[0]), int(bits_of(cr)[show].max()) if show.any() else 0), (int(diag[1]) + int(capped.sum())) & 0xFFFFFFFF], U32)
    return np.where(owned, snew, storage).astype(F), np.where(owned, o, out_new).astype(F), depth, diag


def np_krun(x, storage, out, nstep, depth=None, diag=None):
    """nstep calls, ping-ponging two out planes that both start as `out`: (storage, out, depth, diag)."""
    planes = [np.array(out, F), np.array(out, F)]
    storage = np.array(storage, F)
    cur = 0
    for _ in range(nstep):
        storage, planes[1 - cur], depth, diag = np_route_kinematic(x, planes[cur], planes[1 - cur], storage, depth, diag)
        cur = 1 - cur
    return storage, planes[cur], depth, diag


# ---------------------------------------------------------------------------------------------------------------- the inputs
def manning_plane(ni, nj, seed=0):
    """Manning's n with 0, negative values and NaN among them."""
    r = np.random.default_rng(900 + ni * 17 + nj + seed)
    n = r.uniform(0.02, 0.1, (nj, ni)).astype(F)
    pick = r.random((nj, ni))
    n[pick < 0.08] = 0.0
    n[(pick >= 0.08) & (pick < 0.14)] = -0.05
    n[(pick >= 0.14) & (pick < 0.2)] = np.nan
    n[(pick >= 0.2) & (pick < 0.23)] = -0.0
    return n


def geom_cases(ni, nj):
    """(name, dir, manning, dx, dy, height or None, slope or None) of noahmp_hip_flow_channel: every terrain case with the terrain's own
    directions, random directions with bytes above 8, and slope planes (physical and with NaN / Inf / denormal / negative words)."""
    n = manning_plane(ni, nj)
    out = [(name + ", own dir", np_flow_dir(z, dx, dy), n, dx, dy, z, None) for name, z, dx, dy in trt.terrain_cases(ni, nj)]
    out += [(name + ", random dir", trt.random_dir(ni, nj), n, dx, dy, z, None) for name, z, dx, dy in trt.terrain_cases(ni, nj)[:1] + trt.terrain_cases(ni, nj)[-1:]]
    r = np.random.default_rng(ni + 57 * nj)
    s = r.uniform(-0.01, 0.2, (nj, ni)).astype(F)
    out.append(("slope plane", trt.random_dir(ni, nj, 1), n, DX, DY, None, s))
    out.append(("nasty slope plane", trt.random_dir(ni, nj, 2), nasty(r, ni * nj).reshape(nj, ni), DX, DY, None,
                np.where(r.random((nj, ni)) < 0.4, nasty(r, ni * nj).reshape(nj, ni), s).astype(F)))
    return out


def kin_operands(ni, nj, which, seed=0):
    """The operands of route_operands plus width, length and conv: those of the hills (manning with 0 / negative / NaN: conv 0 and NaN),
    conv negative at some cells; `nasty`: NaN / Inf / denormal / negative words in every plane."""
    ops = trt.route_operands(ni, nj, which, seed)
    ops.pop("release")
    r = np.random.default_rng(5000 + ni * nj + len(which) + seed)
    z = tsh.terrain(ni, nj)
    length, conv, _ = np_flow_channel(np_flow_dir(z, DX, DY), manning_plane(ni, nj), DX, DY, SMIN, height=z)
    conv = np.where(r.random((nj, ni)) < 0.05, F(-1.5), conv).astype(F)
    ops.update(width=r.uniform(1.0, 60.0, (nj, ni)).astype(F), length=length, conv=conv)
    ops["storage"] = np.where(r.random((nj, ni)) < 0.1, -ops["storage"], ops["storage"]).astype(F)      # negative storage
    ops["runoff_a"] = np.where(r.random(ni * nj) < 0.1, -ops["runoff_a"], ops["runoff_a"]).astype(F)      # negative runoff
    if which == "nasty":
        for k in ("width", "length", "conv"):
            ops[k] = np.where(r.random((nj, ni)) < 0.3, nasty(r, ni * nj).reshape(nj, ni), ops[k]).astype(F)
    return ops


def _kblock(mask, col, ncol, ops, rb=True):
    return dict(inmask=mask, col_index=col, ncol=ncol, area=ops["area"], width=ops["width"], length=ops["length"], conv=ops["conv"],
                runoff_a=ops["runoff_a"], runoff_b=ops["runoff_b"] if rb else None, scale=SCALE, dt=DT)


OPTS = ((True, True, True), (False, False, False), (True, True, False), (False, False, True))      # (runoff_b, depth, diag)


@functools.lru_cache(maxsize=None)
def kin_cases(ni, nj):
    """[(what, x, storage, out, depth given, diag given, nstep, (storage, out, depth, diag) of the restatement)] -- made once, shared by
    the host and the device test.  Physical and nasty operands, identity / permuted / mixed col_index, the hills' inmask and random
    bytes, with and without runoff_b, depth and diag, 1, 2 and 25 calls."""
    d, m = trt.hills_network(ni, nj)
    wild = np.random.default_rng(ni * 7 + nj).integers(0, 256, (nj, ni)).astype(np.uint8)
    big = ni * nj > 5000
    out, n = [], 0
    for which in ("physical", "nasty"):
        ops = kin_operands(ni, nj, which)
        for cname, col, ncol in trt.col_indices(ni, nj):
            for mname, mask in (("hills", m), ("random", wild)):
                if big and (mname == "random") != (cname == "mix"):
                    continue                                             # the large window: the two diagonal combinations
                rb, wd, wg = OPTS[n % 4]
                n += 1
                x = _kblock(mask, col, ncol, ops, rb)
                for nstep in ((25,) if big else (1, 2, 25)):
                    what = "%dx%d %s %s mask %s rb %s depth %s diag %s, %d calls" % (ni, nj, which, cname, mname, rb, wd, wg, nstep)
                    want = np_krun(x, ops["storage"], ops["out"], nstep, np.full((nj, ni), POISON, F) if wd else None,
                                   np.array([3, 5], U32) if wg else None)
                    out.append((what, x, ops["storage"], ops["out"], wd, wg, nstep, want))
    return out


# ---------------------------------------------------------------------------------------------------------------- CPU
def build():
    """The host checker: nmp_dev_channel.hpp compiled for the CPU.  Needs nothing of the engine library."""
    deps = [SRC, HEADER] + [os.path.join(CSRC, h) for h in ("nmp_dev_channel.hpp", "nmp_dev_routing.hpp", "nmp_libm.hpp", "nmp_libm_tables.inc")]
    if not os.path.exists(LIB) or any(os.path.getmtime(p) > os.path.getmtime(LIB) for p in deps):
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
    lib.channel_geom_cells.argtypes = [I, I, V, V, V, V, V, V, Fl, Fl, Fl]
    lib.kinematic_cells.argtypes = [I, I] + [V] * 13 + [Fl, Fl, C.c_long]
    lib.channel_geom_cells.restype = lib.kinematic_cells.restype = None
    return lib


_p, _c = trt._p, trt._c


def host_flow_channel(dirp, manning, dx, dy, smin, height=None, slope=None):
    d = _c(dirp, np.uint8)
    nj, ni = d.shape
    n = _c(manning)
    z = _c(height) if height is not None else None
    s = _c(slope) if slope is not None else None
    length, conv = np.full(d.shape, POISON, F), np.full(d.shape, POISON, F)
    _host().channel_geom_cells(ni, nj, _p(z), _p(s), _p(d), _p(n), _p(length), _p(conv), float(dx), float(dy), float(smin))
    return length, conv


def host_krun(x, storage, out, nstep, depth=None, diag=None):
    m = _c(x["inmask"], np.uint8)
    nj, ni = m.shape
    col, area, width, length, conv = _c(x["col_index"], np.int32), _c(x["area"]), _c(x["width"]), _c(x["length"]), _c(x["conv"])
    ra = _c(x["runoff_a"])
    rb = _c(x["runoff_b"]) if x.get("runoff_b") is not None else None
    planes = [_c(out).copy(), _c(out).copy()]
    storage = _c(storage).copy()
    depth = _c(depth).copy() if depth is not None else None
    diag = _c(diag, U32).copy() if diag is not None else None
    cur = 0
    for _ in range(nstep):
        _host().kinematic_cells(ni, nj, _p(m), _p(col), _p(area), _p(width), _p(length), _p(conv), _p(storage), _p(planes[cur]),
                                _p(planes[1 - cur]), _p(ra), _p(rb), _p(depth), _p(diag), float(x["scale"]), float(x["dt"]), int(x["ncol"]))
        cur = 1 - cur
    return storage, planes[cur], depth, diag


def assert_run(got, want, what):
    """(storage, out, depth, diag) of a run against the restatement's: every word; diag[0] as the float it holds."""
    for g, w, nm in zip(got[:3], want[:3], ("storage", "out", "depth")):
        assert (g is None) == (w is None), (what, nm)
        if w is not None:
            assert_same(g, w, "%s: %s" % (what, nm))
    assert (got[3] is None) == (want[3] is None), what
    if want[3] is not None:
        g, w = np.asarray(got[3]).view(U32), np.asarray(want[3]).view(U32)
        assert_same(g[:1].view(F), w[:1].view(F), what + ": diag[0]")
        assert int(g[1]) == int(w[1]), (what, "diag[1]", int(g[1]), int(w[1]))


def test_the_constants():
    """The exponent is the float32 word 0x3F2AAAAB = (float)(2.0/3.0); the diagonal has the roundings of the inverse distances."""
    assert TWO_THIRDS == F(2.0 / 3.0) and float(TWO_THIRDS).hex() == "0x1.5555560000000p-1"
    for dx, dy in ((DX, DY), (3.0, 4.0), (90.0, 30.0)):
        assert F(F(1.0) / np_diagonal(dx, dy)) == np_inverse_distances(dx, dy)[2]
    assert np_diagonal(3.0, 4.0) == 5


@pytest.mark.parametrize("ni, nj", WINDOWS + [CUT])
def test_host_flow_channel_equals_the_restatement(ni, nj):
    """channel_geom_cell compiled for the host against np_flow_channel in every word of length and conv: hills, plains, dx != dy, NaN /
    Inf / denormal / negative terrain, manning 0, negative and NaN, dir bytes above 8, slope given instead of height."""
    for name, d, n, dx, dy, z, s in geom_cases(ni, nj):
        wl, wc, _ = np_flow_channel(d, n, dx, dy, SMIN, height=z, slope=s)
        gl, gc = host_flow_channel(d, n, dx, dy, SMIN, height=z, slope=s)
        assert_same(gl, wl, "%dx%d %s: length" % (ni, nj, name))
        assert_same(gc, wc, "%dx%d %s: conv" % (ni, nj, name))
        with np.errstate(invalid="ignore"):
            assert ((wc == 0) | np.isnan(wc) | (n > 0)).all() and (wc[~(n > 0)].view(U32) == 0).all(), "conv is +0 where manning is not > 0"


@pytest.mark.parametrize("ni, nj", [(67, 35), CUT])
def test_slope_identity(ni, nj):
    """On the terrain's own directions the s plane is, in every bit, the slope that won in noahmp_hip_flow_terrain (np_slopes at the
    chosen k), smin where a cell has no direction; and (conv*manning)^2 recovers max(s, smin): sqrtf, the division and the product are
    one rounding each on r (3 units of 2^-24), the square doubles them and the float64 square adds none: 6 units, asserted as 7."""
    for name, z, dx, dy in trt.terrain_cases(ni, nj)[:2]:
        d = np_flow_dir(z, dx, dy)
        n = np.random.default_rng(3).uniform(0.02, 0.1, (nj, ni)).astype(F)
        length, conv, s = np_flow_channel(d, n, dx, dy, SMIN, height=z)
        slopes = np_slopes(z, dx, dy)
        want = np.full((nj, ni), F(SMIN), F)
        for k in range(1, 9):
            want = np.where(d == k, slopes[k - 1][0], want).astype(F)
        assert_same(s, want, "%s: the s plane" % name)
        assert (s[d != 0] > 0).all() and (d != 0).sum() > ni * nj // 2
        sf = np.maximum(s, F(SMIN)).astype(np.float64)
        back = (conv.astype(F) * n).astype(np.float64) ** 2
        err = np.abs(back / sf - 1).max() / EPS
        print("%s %dx%d: (conv*manning)^2 against max(s, smin): %.2f * 2^-24 (bound 7)" % (name, ni, nj, err))
        assert err <= 7


@pytest.mark.parametrize("ni, nj", WINDOWS + [CUT])
def test_host_route_kinematic_equals_the_restatement(ni, nj):
    """kinematic_cell compiled for the host against np_route_kinematic in every word of storage, out, depth and diag: the cases of
    kin_cases.  Cells that are not owned keep the poison of depth and out_new and their storage, and report nothing."""
    for what, x, storage, out, wd, wg, nstep, want in kin_cases(ni, nj):
        got = host_krun(x, storage, out, nstep, np.full((nj, ni), POISON, F) if wd else None, np.array([3, 5], U32) if wg else None)
        assert_run(got, want, what)
    for cname, col, ncol in trt.col_indices(ni, nj)[2:]:
        c64 = col.astype(np.int64)
        ring = (c64 < -1) | (c64 >= ncol)
        assert ring.any() or ni * nj < 4
        ops = kin_operands(ni, nj, "physical")
        x = _kblock(trt.hills_network(ni, nj)[1], col, ncol, ops)
        poison = np.full((nj, ni), POISON, F)
        s1, o1, h1, g1 = np_route_kinematic(x, ops["out"], poison, ops["storage"], poison, np.zeros(2, U32))
        for plane, keep, nm in ((o1, poison, "out_new"), (h1, poison, "depth"), (s1, ops["storage"], "storage")):
            assert_same(plane[ring], keep[ring], "cells that are not owned keep " + nm)
        x_all_ring = dict(x, col_index=np.full((nj, ni), -2, np.int32))
        assert np_route_kinematic(x_all_ring, ops["out"], poison, ops["storage"], poison, np.zeros(2, U32))[3].tolist() == [0, 0]
        assert host_krun(x_all_ring, ops["storage"], ops["out"], 1, poison, np.zeros(2, U32))[3].tolist() == [0, 0]


def test_the_cases_reach_every_path():
    """The shared cases hold capped and uncapped cells, cells that do not enter (s1 <= 0, NaN s1, conv 0, negative and NaN), NaN cr."""
    ni, nj = 67, 35
    ops = kin_operands(ni, nj, "physical")
    col = np.arange(ni * nj, dtype=np.int32).reshape(nj, ni)
    x = _kblock(trt.hills_network(ni, nj)[1], col, ni * nj, ops)
    s, o, h, g = np_route_kinematic(x, ops["out"], ops["out"], ops["storage"], np.zeros((nj, ni), F), np.zeros(2, U32))
    capped = int(g[1])
    assert 0 < capped < ni * nj and ((o > 0) & (s > 0)).any(), "capped and uncapped cells"
    assert (s.view(U32)[(o > 0) & (s == 0)] == 0).all(), "a capped cell holds +0"
    assert ((o == 0) & (ops["conv"] > 0)).any() and (o[~(ops["conv"] > 0)] == 0).all()
    assert np.isfinite(g[:1].view(F)[0]) and g[:1].view(F)[0] > 0
    opsn = kin_operands(ni, nj, "nasty")
    g = np_route_kinematic(_kblock(x["inmask"], col, ni * nj, opsn), opsn["out"], opsn["out"], opsn["storage"], None, np.zeros(2, U32))[3]
    assert np.isnan(g[:1].view(F)[0]), "a NaN cr shows in diag[0]"


# ---------------------------------------------------------------------------------------------------------------- exact identities
def _straight(n, conv, storage0):
    d = np.full((1, n), 1, np.uint8)                                     # every cell drains east, the last one nowhere
    d[0, -1] = 0
    one = np.ones((1, n), F)
    x = dict(inmask=np_inmask(d), col_index=np.full((1, n), -1, np.int32), ncol=0, area=one, width=one, length=one, conv=np.full((1, n), conv, F),
             runoff_a=np.zeros(1, F), runoff_b=None, scale=1.0, dt=1.0)
    storage = np.zeros((1, n), F)
    storage[0, 0] = storage0
    return x, storage


def test_the_cap_moves_a_pulse_one_cell_per_call():
    """A straight channel of 7 cells, width = length = 1, conv = 1e30, a pulse of 1.0 m3 in the head cell: every cell that holds the pulse
    is capped and releases all of it, so the pulse is in out of cell t-1 after call t, leaves at the cell without a direction in call 7,
    every storage word is exactly +0 and diag[1] counts exactly the capped cells: one per call while the pulse is inside.  With conv = 0
    nothing ever moves.  No tolerance."""
    n = 7
    x, storage = _straight(n, 1e30, 1.0)
    zero = np.zeros((1, n), F)
    for run in (np_krun, host_krun):
        for t in range(1, n + 3):
            s, o, h, g = run(x, storage, zero, t, zero, np.zeros(2, U32))
            want = np.zeros((1, n), F)
            if t <= n:
                want[0, t - 1] = 1.0
            assert_same(o, want, "out after %d calls" % t)
            assert (s.view(U32) == 0).all(), "every storage word is +0"
            assert int(g[1]) == min(t, n), "one capped cell per call while the pulse is inside"
            assert_same(h, want, "depth = s1 / (1*1) of the cell that held the pulse in the last call")
        x0, _ = _straight(n, 0.0, 1.0)
        s, o, h, g = run(x0, storage, zero, 25, zero, np.zeros(2, U32))
        assert_same(s, storage, "conv = 0: the storage stays")
        assert (o.view(U32) == 0).all() and (h.view(U32) == 0).all() and g.tolist() == [0, 0]


# ---------------------------------------------------------------------------------------------------------------- budget
# Where the bounds come from, counted from the rounded operations of the header text in units of 2^-24, as for test_budget_on_the_hills
# of test_routing.  A rounding contributes at most one unit relative to its own result.
#   The input v = ((a + b)*scale)*area: 3 roundings.
#   The water of a cell and call, S' + o against S + v + q: q at most 7 roundings, sv 1, s1 1; o is whatever it is (the SAME o leaves the
#     storage and enters out; a capped cell's S' = s1 - s1 is exact); S' = s1 - o: 1.  10 units of s1 per cell and call, and the s1 of a
#     call add up to at most the input so far: 3 + 5 * (N + 1) units of the total input after N calls with constant input, 258 for N = 50.
#   Against a float64 run of the same scheme the two o differ as well: wl, h, a one each (3 units on a); p = w + (h + h): h + h is exact,
#     1 for the sum and at most h's 2: 3; R = a/p: 3 + 3 + 1 = 7; powf_ is glibc's powf bit for bit (nmp_libm.hpp), a float64 evaluation
#     rounded once: it carries 2/3 of R's error and its own rounding, 4.7 + 1 -> 6 units; vel 7; qa = vel*a: 7 + 3 + 1 = 11; od: 12.
#     12 units of o <= s1 on top of the 10 + 1 of the linear scheme: 23 per cell and call, 3 + 11.5 * (N + 1) = 589.5 -> 590 for N = 50.
#     A perturbation stays a perturbation of at most its own size as long as neither part of (S - o, o) decreases when S grows: o =
#     min(S, Q(S)*dt) has slope dQ/dS*dt = the celerity Courant number where it is not capped, 1 where it is.  The test asserts that
#     courant() stays below 1.
BUDGET_STEPS = 50
BUDGET_BOUND = 3 + 5 * (BUDGET_STEPS + 1)
SPLIT_BOUND = 590


def _krun64(x, storage, nstep, outlets):
    """The scheme of the header text in float64 on the same float32 operands: (storage, what has left at the outlets, total input)."""
    m = x["inmask"]
    col = x["col_index"].astype(np.int64)
    ra, rb = x["runoff_a"].astype(np.float64), x["runoff_b"].astype(np.float64)
    v = (ra[col] + rb[col]) * float(F(x["scale"])) * x["area"].astype(np.float64)
    w, ln, cv = (x[k].astype(np.float64) for k in ("width", "length", "conv"))
    dt, y = float(F(x["dt"])), float(TWO_THIRDS)
    S = storage.astype(np.float64)
    out = np.zeros_like(S)
    left = 0.0
    for _ in range(nstep):
        q = np.zeros_like(S)
        for k in range(1, 9):
            on, inside = neighbour(out, k)
            q = q + np.where(inside & ((m >> (k - 1)) & 1).astype(bool), on, 0.0)
        s1 = (S + v) + q
        h = s1 / (w * ln)
        a = w * h
        od = cv * (a / (w + (h + h))) ** y * a * dt
        out = np.where((s1 > 0) & (cv > 0), np.where(od < s1, od, s1), 0.0)
        S = s1 - out
        left += out[outlets].sum()
    return S, left, v.sum() * nstep


def test_budget_on_the_hills():
    """50 calls with constant input on the 67 x 35 hills: storage + in flight + what has left at the cells without a direction against the
    input, and storage and what has left against a float64 run of the same scheme, under the bounds counted above.  The restatement
    measured 0.13 * 2^-24 of the input for the sum (bound 258) and 0.11 / 0.00 for the storage / what has left against float64 (bound
    590); the celerity Courant number reaches 0.69, no cell is capped and 1 % of the input has left."""
    ni, nj = 67, 35
    z = tsh.terrain(ni, nj)
    d = np_flow_dir(z, DX, DY)
    m = np_inmask(d)
    outlets = d == 0
    ops = trt.route_operands(ni, nj, "physical")
    r = np.random.default_rng(6)
    length, conv, _ = np_flow_channel(d, r.uniform(0.05, 0.2, (nj, ni)).astype(F), DX, DY, SMIN, height=z)
    x = dict(inmask=m, col_index=np.arange(ni * nj, dtype=np.int32).reshape(nj, ni), ncol=ni * nj, area=ops["area"],
             width=r.uniform(50.0, 300.0, (nj, ni)).astype(F), length=length, conv=conv, runoff_a=ops["runoff_a"], runoff_b=ops["runoff_b"],
             scale=float(F(F(300.0) * F(1e-3))), dt=300.0)
    zero = np.zeros((nj, ni), F)
    left = 0.0
    planes, S, cur, diag = [zero.copy(), zero.copy()], zero.copy(), 0, np.zeros(2, U32)
    for _ in range(BUDGET_STEPS):
        S, planes[1 - cur], _, diag = np_route_kinematic(x, planes[cur], planes[1 - cur], S, None, diag)
        cur = 1 - cur
        left += planes[cur][outlets].astype(np.float64).sum()
    gs, go, _, gd = host_krun(x, zero, zero, BUDGET_STEPS, None, np.zeros(2, U32))
    assert_run((gs, go, None, gd), (S, planes[cur], None, diag), "compiled")
    courant = 5.0 / 3.0 * float(diag[:1].view(F)[0])
    S64, left64, total = _krun64(x, zero, BUDGET_STEPS, outlets)
    in_flight = planes[cur][~outlets].astype(np.float64).sum()           # released in the last call and not yet gathered
    have = S.astype(np.float64).sum() + left + in_flight
    r_sum = abs(have - total) / total / EPS
    r_s = abs(S.astype(np.float64).sum() - S64.sum()) / total / EPS
    r_l = abs(left - left64) / total / EPS
    print("%d x %d, %d calls: input %.6g m3, (storage + in flight + left) - input = %.2f * 2^-24 of it (bound %d); against float64: storage %.2f,"
          " left %.2f (bound %d); %.0f %% has left; courant %.3f, %d capped" % (ni, nj, BUDGET_STEPS, total, r_sum, BUDGET_BOUND, r_s, r_l,
                                                                              SPLIT_BOUND, 100 * left / total, courant, int(diag[1])))
    assert courant < 1.0, "the non-expansion argument of the float64 bound"
    assert r_sum <= BUDGET_BOUND
    assert r_s <= SPLIT_BOUND and r_l <= SPLIT_BOUND
    assert 0.005 < left / total < 0.95, "water is both held and released (below a Courant number of 1 most of it is still on its way)"


# ---------------------------------------------------------------------------------------------------------------- the physics
PLANE_L, PLANE_W, PLANE_S, PLANE_N, PLANE_I, PLANE_T = 1000.0, 1000.0, 0.01, 0.05, 1e-5, 6000.0
PLANE_CONV = np.sqrt(PLANE_S) / PLANE_N


def plane_dt(ncell, rain, courant=0.5):
    """dt at which the celerity Courant number 5/3 * vel * dt / dx at equilibrium (depth (rain*L/conv)^(3/5) at the outlet) is `courant`."""
    he = (rain * PLANE_L / PLANE_CONV) ** 0.6
    return courant * (PLANE_L / ncell) / (5.0 / 3.0 * PLANE_CONV * he ** (2.0 / 3.0))


def plane_block(ncell, rain, dt):
    """A row of ncell cells down a plane 1000 m long and wide, uniform input `rain` [m/s] as a runoff plane in mm/s."""
    d = np.full((1, ncell), 1, np.uint8)
    d[0, -1] = 0
    dxc = PLANE_L / ncell
    slope = np.full((1, ncell), PLANE_S, F)
    length, conv, _ = np_flow_channel(d, np.full((1, ncell), PLANE_N, F), dxc, PLANE_W, SMIN, slope=slope)
    assert (length == F(dxc)).all()
    return dict(inmask=np_inmask(d), col_index=np.arange(ncell, dtype=np.int32).reshape(1, ncell), ncol=ncell,
                area=np.full((1, ncell), dxc * PLANE_W, F), width=np.full((1, ncell), PLANE_W, F), length=length, conv=conv,
                runoff_a=np.full(ncell, rain * 1e3, F), runoff_b=None, scale=float(F(F(dt) * F(1e-3))), dt=dt)


def plane_run(ncell, rain, dt, ncall, route=None):
    """The outflow [m3/s] at the foot of the plane after every call, the diag words; route: another per-call function (the reservoirs)."""
    x = plane_block(ncell, rain, dt)
    zero = np.zeros((1, ncell), F)
    S, planes, cur, diag, q = zero.copy(), [zero.copy(), zero.copy()], 0, np.zeros(2, U32), []
    for _ in range(ncall):
        if route is None:
            S, planes[1 - cur], _, diag = np_route_kinematic(x, planes[cur], planes[1 - cur], S, None, diag)
        else:
            S, planes[1 - cur] = route(x, planes[cur], planes[1 - cur], S)
        cur = 1 - cur
        q.append(float(planes[cur][0, -1]) / dt)
    return np.array(q), diag


def analytic_outflow(t, rain):
    """The kinematic wave on a plane under uniform input: w*conv*(i*min(t, te))^(5/3), te = (L / (conv * i^(2/3)))^(3/5)."""
    te = (PLANE_L / (PLANE_CONV * rain ** (2.0 / 3.0))) ** 0.6
    return PLANE_W * PLANE_CONV * (rain * np.minimum(t, te)) ** (5.0 / 3.0)


def test_the_kinematic_wave_on_a_plane_converges():
    """A plane 1000 m long and wide, slope 0.01, n = 0.05, uniform input 1e-5 m/s for 6000 s, N = 16, 32, 64 cells in a row, dt such that
    the celerity Courant number at equilibrium is 0.5: the largest error of the outflow against the analytic solution over the run,
    relative to i*L*w, falls strictly from N = 16 to 32 to 64 (a float64 run of the scheme gives 0.092, 0.071, 0.051; the float32
    restatement, with the outflow of call n taken at t = n*dt, measured 0.0935, 0.0693, 0.0498); courant() at the end is 0.5 within 1 %; no cell is ever capped."""
    errs = []
    for ncell in (16, 32, 64):
        dt = plane_dt(ncell, PLANE_I)
        ncall = int(round(PLANE_T / dt))
        q, diag = plane_run(ncell, PLANE_I, dt, ncall)
        t = dt * np.arange(1, ncall + 1)
        errs.append(float(np.abs(q - analytic_outflow(t, PLANE_I)).max() / (PLANE_I * PLANE_L * PLANE_W)))
        courant = 5.0 / 3.0 * float(diag[:1].view(F)[0])
        print("N = %d: dt %.3f s, %d calls, largest error %.4f of i*L*w, outflow at the end %.6f of it, courant %.4f, capped %d"
              % (ncell, dt, ncall, errs[-1], q[-1] / (PLANE_I * PLANE_L * PLANE_W), courant, int(diag[1])))
        assert abs(courant / 0.5 - 1) <= 0.01
        assert int(diag[1]) == 0
    assert errs[0] > errs[1] > errs[2]


def _time_to(q, dt, level):
    return dt * (1 + int(np.argmax(q >= level)))


def test_a_flood_wave_is_faster_than_a_trickle():
    """The point of the feature.  The same plane, N = 32: with ten times the input the outflow reaches 90 % of its equilibrium i*L*w
    strictly earlier than with the plain input (the kinematic time to equilibrium goes with i^(-2/5)); with the linear reservoirs of
    noahmp_hip_route_runoff and a fixed release the two times are equal."""
    ncell = 32
    dt = plane_dt(ncell, 10 * PLANE_I)                                   # Courant 0.5 for the larger input, 0.2 for the plain one
    ncall = int(round(PLANE_T / dt))
    times = {}
    for name, route in (("kinematic", None), ("reservoirs", lambda x, oo, on, s: trt.np_route(dict(x, release=np.full((1, ncell), 0.2, F)), oo, on, s))):
        for rain in (PLANE_I, 10 * PLANE_I):
            q, diag = plane_run(ncell, rain, dt, ncall, route)
            assert q[-1] >= 0.9 * rain * PLANE_L * PLANE_W, (name, rain)
            times[name, rain] = _time_to(q, dt, 0.9 * rain * PLANE_L * PLANE_W)
    print("time to 90 %% of equilibrium [s]: %r" % times)
    assert times["kinematic", 10 * PLANE_I] < times["kinematic", PLANE_I]
    assert times["reservoirs", 10 * PLANE_I] == times["reservoirs", PLANE_I]


# ---------------------------------------------------------------------------------------------------------------- decomposition, column order
def _kparts(ni, nj, z, ops, x):
    gcol = np.arange(ni * nj, dtype=np.int32).reshape(nj, ni)
    parts = []
    for tile, blk, dblk, owned in trt._parts(ni, nj, z, 2):
        xp = dict(x, inmask=np_inmask(dblk), col_index=np.where(owned, gcol[blk], -2).astype(np.int32),
                  **{k: x[k][blk] for k in ("area", "width", "length", "conv")})
        parts.append(dict(x=xp, tile=tile, blk=blk, owned=owned))
    return parts


def _whole(ni, nj):
    z = tsh.terrain(ni, nj, True)
    ops = kin_operands(ni, nj, "physical")
    d = np_flow_dir(z, DX, DY)
    x = _kblock(np_inmask(d), np.arange(ni * nj, dtype=np.int32).reshape(nj, ni), ni * nj, ops)
    return z, ops, x


def test_decomposition():
    """70 x 130 cut 2 x 2 (directions from margin-2 height windows, the ring of out refreshed from the owners after every call): after
    20 calls no word of storage, out and depth differs from the undecomposed run; the maximum of the four diag[0] and the sum of the
    four diag[1] are the whole's.  Restated and compiled."""
    ni, nj = CUT
    z, ops, x = _whole(ni, nj)
    zero2 = np.zeros(2, U32)
    ws, wo, wh, wg = np_krun(x, ops["storage"], ops["out"], 20, np.zeros((nj, ni), F), zero2)
    for one in (np_route_kinematic, lambda x, oo, on, s, h, g: _host_one(x, oo, on, s, h, g)):
        parts = _kparts(ni, nj, z, ops, x)
        for p in parts:
            p.update(S=ops["storage"][p["blk"]].copy(), out=[ops["out"][p["blk"]].copy(), ops["out"][p["blk"]].copy()],
                     h=np.zeros(ops["out"][p["blk"]].shape, F), g=zero2.copy())
        G, GS, GH, cur = ops["out"].copy(), ops["storage"].copy(), np.zeros((nj, ni), F), 0
        for _ in range(20):
            for p in parts:
                p["S"], p["out"][1 - cur], p["h"], p["g"] = one(p["x"], p["out"][cur], p["out"][1 - cur], p["S"], p["h"], p["g"])
            cur = 1 - cur
            for p in parts:
                for whole, part in ((G, p["out"][cur]), (GS, p["S"]), (GH, p["h"])):
                    whole[p["tile"]] = part[p["owned"]].reshape(whole[p["tile"]].shape)
            for p in parts:
                p["out"][cur] = G[p["blk"]].copy()
        assert trt._differ(GS, ws) + trt._differ(G, wo) + trt._differ(GH, wh) == 0
        assert max(int(p["g"][0]) for p in parts) == int(wg[0]) and sum(int(p["g"][1]) for p in parts) == int(wg[1]) and int(wg[1]) > 0


def _host_one(x, out_old, out_new, storage, depth, diag):
    m = _c(x["inmask"], np.uint8)
    nj, ni = m.shape
    s, o, h, g = _c(storage).copy(), _c(out_new).copy(), _c(depth).copy(), _c(diag, U32).copy()
    keep = [_c(x["col_index"], np.int32)] + [_c(x[k]) for k in ("area", "width", "length", "conv")] + [_c(out_old), _c(x["runoff_a"]), _c(x["runoff_b"])]
    col, area, width, length, conv, old, ra, rb = keep
    _host().kinematic_cells(ni, nj, _p(m), _p(col), _p(area), _p(width), _p(length), _p(conv), _p(s), _p(old), _p(o), _p(ra), _p(rb), _p(h), _p(g),
                            float(x["scale"]), float(x["dt"]), int(x["ncol"]))
    return s, o, h, g


def _permuted(x, ops, ni, nj):
    ncell = ni * nj
    perm = np.random.default_rng(3).permutation(ncell)                   # position p of the store holds tile column perm[p]
    inv = np.empty(ncell, np.int32)
    inv[perm] = np.arange(ncell, dtype=np.int32)
    return dict(x, col_index=inv.reshape(nj, ni), runoff_a=ops["runoff_a"][perm], runoff_b=ops["runoff_b"][perm])


@pytest.mark.parametrize("ni, nj", [(65, 5), (67, 35)])
def test_column_order(ni, nj):
    """The same run with a permuted col_index and the runoff planes permuted with it gives the same window planes and diag words."""
    ops = kin_operands(ni, nj, "physical")
    x = _kblock(trt.hills_network(ni, nj)[1], np.arange(ni * nj, dtype=np.int32).reshape(nj, ni), ni * nj, ops)
    want = np_krun(x, ops["storage"], ops["out"], 10, np.zeros((nj, ni), F), np.zeros(2, U32))
    got = host_krun(_permuted(x, ops, ni, nj), ops["storage"], ops["out"], 10, np.zeros((nj, ni), F), np.zeros(2, U32))
    assert_run(got, want, "permuted")


# ---------------------------------------------------------------------------------------------------------------- refusals and bindings
GEOM_PLANES = ("height", "slope", "dir", "manning", "length", "conv")
KIN_PLANES = ("inmask", "col_index", "area", "width", "length", "conv", "storage", "out_old", "out_new", "runoff_a", "runoff_b", "depth", "diag")
KIN_REQUIRED = KIN_PLANES[:10]
CALLS = ("noahmp_hip_flow_channel", "noahmp_hip_route_kinematic")
NCELL = 15


def _fc_block(ptrs, **kw):
    b = abi.FlowChannel()
    for k in GEOM_PLANES:
        setattr(b, k, ptrs[k])
    b.slope = None
    b.ni, b.nj, b.dx, b.dy, b.smin = 5, 3, DX, DY, SMIN
    for k, v in kw.items():
        setattr(b, k, v)
    return b


def _rk_block(ptrs, **kw):
    b = abi.RouteKinematic()
    for k in KIN_PLANES:
        setattr(b, k, ptrs[k])
    b.scale, b.dt, b.ni, b.nj = 0.6, 600.0, 5, 3
    for k, v in kw.items():
        setattr(b, k, v)
    return b


def refusal_probes(gp, kp):
    """[(site id, call, block or None, ncol)]: one probe per refusal site and per way into it."""
    out = [("channel.null", CALLS[0], None, None)]
    for f in ("dir", "manning", "length", "conv"):
        out.append(("channel.required." + f, CALLS[0], _fc_block(gp, **{f: None}), None))
    out.append(("channel.both", CALLS[0], _fc_block(gp, slope=gp["slope"]), None))
    out.append(("channel.neither", CALLS[0], _fc_block(gp, height=None), None))
    for nm, kw in (("ni", dict(ni=-1)), ("nj", dict(nj=-1)), ("big", dict(ni=65536, nj=32768))):
        out.append(("channel.window." + nm, CALLS[0], _fc_block(gp, **kw), None))
    for nm, kw in (("dx0", dict(dx=0.0)), ("dxnan", dict(dx=float("nan"))), ("dyinf", dict(dy=float("inf"))), ("dyneg", dict(dy=-1.0))):
        out.append(("channel.spacing." + nm, CALLS[0], _fc_block(gp, **kw), None))
    for nm, v in (("zero", 0.0), ("neg", -1e-4), ("nan", float("nan")), ("inf", float("inf"))):
        out.append(("channel.smin." + nm, CALLS[0], _fc_block(gp, smin=v), None))
    out.append(("channel.same.outputs", CALLS[0], _fc_block(gp, conv=gp["length"]), None))
    out.append(("channel.overlap.outputs", CALLS[0], _fc_block(gp, conv=gp["length"] + 4 * (NCELL - 1)), None))
    for f in ("height", "manning", "dir"):
        out.append(("channel.alias.length." + f, CALLS[0], _fc_block(gp, length=gp[f]), None))
        out.append(("channel.alias.conv." + f, CALLS[0], _fc_block(gp, conv=gp[f]), None))
    out.append(("channel.alias.conv.slope", CALLS[0], _fc_block(gp, height=None, slope=gp["slope"], conv=gp["slope"] + 8), None))
    out.append(("kinematic.null", CALLS[1], None, NCELL))
    for f in KIN_REQUIRED:
        out.append(("kinematic.required." + f, CALLS[1], _rk_block(kp, **{f: None}), NCELL))
    out.append(("kinematic.same.out", CALLS[1], _rk_block(kp, out_new=kp["out_old"]), NCELL))
    for nm, kw in (("ni", dict(ni=-1)), ("nj", dict(nj=-1)), ("big", dict(ni=65536, nj=32768))):
        out.append(("kinematic.window." + nm, CALLS[1], _rk_block(kp, **kw), NCELL))
    for nm, ncol in (("neg", -1), ("big", 2 ** 31)):
        out.append(("kinematic.ncol." + nm, CALLS[1], _rk_block(kp), ncol))
    for nm, v in (("zero", 0.0), ("neg", -600.0), ("nan", float("nan")), ("inf", float("inf"))):
        out.append(("kinematic.dt." + nm, CALLS[1], _rk_block(kp, dt=v), NCELL))
    for f in ("storage", "out_old", "out_new"):
        out.append(("kinematic.depth." + f, CALLS[1], _rk_block(kp, depth=kp[f]), NCELL))
    out.append(("kinematic.depth.overlap", CALLS[1], _rk_block(kp, depth=kp["storage"] + 4 * (NCELL - 1)), NCELL))
    for off in (1, 2, 3):
        out.append(("kinematic.diag.misaligned.%d" % off, CALLS[1], _rk_block(kp, diag=kp["diag"] + off), NCELL))
    return out


def _call(lib, fn, block, ncol):
    ref = C.byref(block) if block is not None else None
    return getattr(lib, fn)(ref, None) if ncol is None else getattr(lib, fn)(ref, ncol, None)


def _refusals(lib, gp, kp):
    """Every refusal: -105 and the full text of the fixture."""
    want = json.load(open(REFUSAL_FIXTURE))
    probes = refusal_probes(gp, kp)
    assert sorted(want) == sorted(p[0] for p in probes)
    for site, fn, block, ncol in probes:
        rc = _call(lib, fn, block, ncol)
        assert [rc, lib.noahmp_hip_last_error().decode()] == want[site], site
        assert rc == -105 and want[site][1].startswith(fn + ": "), site


def test_refusals_write_nothing():
    """Every refusal site of the two calls gives -105 and its full text (tests/golden/channel_refusal_text.json) before anything is
    launched or read: the planes here are host memory that the calls must not touch, and they keep their poison."""
    lib = abi.load_library()
    gpl = {k: np.full(32, POISON, F) for k in GEOM_PLANES}
    kpl = {k: np.full(32, POISON, F) for k in KIN_PLANES}
    _refusals(lib, {k: v.ctypes.data for k, v in gpl.items()}, {k: v.ctypes.data for k, v in kpl.items()})
    assert all((p == POISON).all() for p in list(gpl.values()) + list(kpl.values()))
    text = json.load(open(REFUSAL_FIXTURE))
    for site, word in (("channel.both", "exactly one"), ("channel.neither", "exactly one"), ("channel.smin.nan", "smin"), ("channel.spacing.dx0", "dx"),
                       ("channel.window.big", "ni*nj"), ("channel.same.outputs", "different"), ("channel.alias.conv.dir", "share"),
                       ("kinematic.required.width", "required"), ("kinematic.same.out", "different"), ("kinematic.ncol.big", "ncol"),
                       ("kinematic.dt.nan", "dt"), ("kinematic.depth.out_new", "depth"), ("kinematic.diag.misaligned.2", "aligned")):
        assert word in text[site][1], site
    assert len({tuple(v) for v in text.values()}) == 8 + 8


HEADER_LINES = (
    "#define NOAHMP_HIP_HAS_ROUTE_KINEMATIC 1\n", "#define NOAHMP_HIP_ABI_MINOR 3\n", "typedef struct noahmp_flow_channel {", "} noahmp_flow_channel;",
    "typedef struct noahmp_route_kinematic {", "} noahmp_route_kinematic;",
    "int    noahmp_hip_flow_channel(const noahmp_flow_channel* fc, void* stream);",
    "int    noahmp_hip_route_kinematic(const noahmp_route_kinematic* r, int64_t ncol, void* stream);",
    "sf = (s > smin) ? s : smin", "r = sqrtf(sf)", "cv = r / manning[c];  conv[c] = (manning[c] > 0) ? cv : 0",
    "wl = width[c]*length[c];  h = s1/wl;  a = width[c]*h;  h2 = h + h;  p = width[c] + h2;  R = a/p", "r23 = powf(R, 0x1.555556p-1f)",
    "vel = conv[c]*r23;  qa = vel*a;  od = qa*dt", "capped = !(od < s1);  o = capped ? s1 : od", "vd = vel*dt;  cr = vd/length[c]",
    "storage[c] = s1 - o;  out_new[c] = o;  if depth: depth[c] = h", "The call never zeroes them", "a NaN sorts above Inf",
)


def test_bindings_carry_the_channel_calls():
    from tools import gen_abi
    for rel, text in (("include/noahmp_hip.h", gen_abi.c_header()), ("noahmp_amd/fortran/module_sf_noahmpdrv_hip.F90", gen_abi.fortran_shim())):
        assert open(os.path.join(ROOT, rel)).read() == text, rel
    hdr = open(HEADER).read()
    for word in HEADER_LINES:
        assert word in hdr, word
    assert "\n".join(gen_abi.channel_header()) in hdr
    assert "noahmp_route_kinematic" not in gen_abi.ref_harness() and "noahmp_route_kinematic" not in gen_abi.shim_wrap()
    f90 = open(os.path.join(ROOT, "noahmp_amd", "fortran", "module_sf_noahmpdrv_hip.F90")).read()
    for word in tuple("bind(C, name='%s')" % c for c in CALLS) + ("type, bind(C) :: noahmp_flow_channel ", "type, bind(C) :: noahmp_route_kinematic "):
        assert word in f90, word
    for sym in CALLS:
        assert sym in abi.EXPORTED_SYMBOLS
    assert [n for n, _ in abi.FlowChannel._fields_] == list(GEOM_PLANES) + ["ni", "nj", "dx", "dy", "smin"]
    assert [n for n, _ in abi.RouteKinematic._fields_] == list(KIN_PLANES) + ["scale", "dt", "ni", "nj"]
    assert [n for n, _ in abi.RouteKinematic._fields_ if n != "release"] and "release" not in [n for n, _ in abi.RouteKinematic._fields_]
    assert {n for n, _ in abi.Route._fields_} - {"release"} <= {n for n, _ in abi.RouteKinematic._fields_}


def test_ctypes_mirrors_match_the_compiled_header(tmp_path):
    body, want = "", []
    for cname, cls in (("noahmp_flow_channel", abi.FlowChannel), ("noahmp_route_kinematic", abi.RouteKinematic)):
        names = [n for n, _ in cls._fields_]
        body += 'printf(" %%zu", sizeof(%s));' % cname + "".join('printf(" %%zu", offsetof(%s, %s));' % (cname, n) for n in names)
        want += [C.sizeof(cls)] + [getattr(cls, n).offset for n in names]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "noahmp_hip.h"\nint main(){' + body +
                   'printf(" %d %d", NOAHMP_HIP_ABI_MINOR, NOAHMP_HIP_HAS_ROUTE_KINEMATIC); return 0;}')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(v) for v in subprocess.check_output([str(exe)]).split()] == want + [3, 1]


def test_library_exports_the_channel_calls():
    if not os.path.exists(abi.LIB_PATH):
        from noahmp_amd import build as b
        b.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", abi.LIB_PATH]).decode()
    for sym in CALLS:
        assert " T %s\n" % sym in out, sym


@pytest.mark.skipif(tr._flang() is None, reason="no flang")
def test_generated_fortran_types_and_interfaces_compile(tmp_path):
    """The channel part of the generated module compiles, and a caller of the two interfaces type-checks."""
    from tools import gen_abi
    text = "\n".join(["module channel_abi_check", "  use iso_c_binding", "  implicit none"] + gen_abi.channel_f90_types() + ["  interface"] +
                     gen_abi.channel_f90_interfaces() +
                     ["  end interface", "contains", "  function go(planes, ncol) result(rc)", "    type(c_ptr), intent(in) :: planes(13)",
                      "    integer(c_int64_t), value :: ncol", "    type(noahmp_flow_channel) :: fc", "    type(noahmp_route_kinematic) :: r",
                      "    integer(c_int) :: rc",
                      "    fc%height = planes(1); fc%slope = c_null_ptr; fc%dir = planes(2); fc%manning = planes(3); fc%length = planes(4)",
                      "    fc%conv = planes(5); fc%ni = 64; fc%nj = 8; fc%dx = 1000.0; fc%dy = 1000.0; fc%smin = 1.0e-4",
                      "    rc = noahmp_hip_flow_channel(fc, c_null_ptr)",
                      "    r%inmask = planes(6); r%col_index = planes(7); r%area = planes(8); r%width = planes(9); r%length = planes(4)",
                      "    r%conv = planes(5); r%storage = planes(10); r%out_old = planes(11); r%out_new = planes(12); r%runoff_a = planes(13)",
                      "    r%runoff_b = c_null_ptr; r%depth = c_null_ptr; r%diag = c_null_ptr; r%scale = 0.6; r%dt = 600.0; r%ni = 64; r%nj = 8",
                      "    rc = noahmp_hip_route_kinematic(r, ncol, c_null_ptr)",
                      "  end function go", "end module channel_abi_check", ""])
    f = tmp_path / "channel_abi_check.f90"
    f.write_text(text)
    subprocess.check_call([tr._flang(), "-c", str(f), "-o", str(tmp_path / "channel_abi_check.o"), "-J", str(tmp_path)], cwd=str(tmp_path))


def test_width_from_area():
    """a * area^b in float64, rounded once, at and above the threshold; below it the cell's width across its direction."""
    from noahmp_amd.routing import ChannelFlow
    d = np.array([[0, 1, 2, 3, 4], [5, 6, 7, 8, 200]], np.uint8)
    area = np.array([[1e3, 2e3, 3e3, 4e3, 5e3], [6e3, 7e3, 8e3, 9e3, 1e3]])
    dx, dy = 30.0, 40.0
    w = ChannelFlow.width_from_area(area, 2.0, 0.4, 1e9, d, dx, dy)
    assert w.dtype == F and w.tolist() == [[30.0, 40.0, 24.0, 30.0, 24.0], [40.0, 24.0, 30.0, 24.0, 30.0]]
    w = ChannelFlow.width_from_area(area, 2.0, 0.4, 5e3, d, dx, dy)
    assert_same(w[area >= 5e3], (2.0 * area[area >= 5e3] ** 0.4).astype(F), "the hydraulic-geometry width")
    assert w[0, :4].tolist() == [30.0, 40.0, 24.0, 30.0]


# ---------------------------------------------------------------------------------------------------------------- GPU
_dev = tr._dev
_pool, _guards_ok = trt._pool, trt._guards_ok


@pytest.mark.gpu
@pytest.mark.parametrize("ni, nj", WINDOWS + [CUT])
def test_gpu_flow_channel_equals_the_restatement(engine, ni, nj):
    """noahmp_hip_flow_channel against np_flow_channel in every word of length and conv, the cases of the host test; the destinations sit
    at an odd offset inside a poisoned pool whose guard words keep the poison.  An empty window writes nothing."""
    import torch
    ncell = ni * nj
    pool, (ld, cd) = _pool(ncell, 2, torch.float32, POISON)
    ld, cd = ld.view(nj, ni), cd.view(nj, ni)
    for name, d, n, dx, dy, z, s in geom_cases(ni, nj):
        pool.fill_(POISON)
        torch.cuda.synchronize()
        engine.flow_channel(engine.flow_channel_block(_dev(d), _dev(n), ld, cd, dx, dy, SMIN, height=_dev(z) if z is not None else None,
                                                      slope=_dev(s) if s is not None else None))
        engine.stream_sync()
        wl, wc, _ = np_flow_channel(d, n, dx, dy, SMIN, height=z, slope=s)
        assert_same(ld.cpu().numpy(), wl, "%dx%d %s: length" % (ni, nj, name))
        assert_same(cd.cpu().numpy(), wc, "%dx%d %s: conv" % (ni, nj, name))
        assert _guards_ok(pool, ncell, POISON), name
    pool.fill_(POISON)
    torch.cuda.synchronize()
    name, d, n, dx, dy, z, s = geom_cases(ni, nj)[0]
    b = engine.flow_channel_block(_dev(d), _dev(n), ld, cd, dx, dy, SMIN, height=_dev(z))
    b.nj = 0
    engine.flow_channel(b)
    engine.stream_sync()
    assert (pool.cpu().numpy() == POISON).all()


def _gpu_krun(eng, x, storage, out, nstep, with_depth, diag0):
    """nstep calls of noahmp_hip_route_kinematic on planes at odd offsets inside poisoned pools: ((storage, out, depth, diag), guards)."""
    import torch
    nj, ni = x["inmask"].shape
    ncell = ni * nj
    pool, (sd, o0, o1, hd) = _pool(ncell, 4, torch.float32, POISON)
    sd, o0, o1, hd = (t.view(nj, ni) for t in (sd, o0, o1, hd))
    sd.copy_(_dev(storage))
    o0.copy_(_dev(out))
    o1.copy_(_dev(out))
    gpool = torch.full((8,), 77, dtype=torch.int32, device="cuda")
    diag = None
    if diag0 is not None:
        diag = gpool[3:5]
        diag.copy_(_dev(np.asarray(diag0, U32).view(np.int32)))
    ra = _dev(x["runoff_a"])
    rb = _dev(x["runoff_b"]) if x.get("runoff_b") is not None else None
    m, col, area, width, length, conv = (_dev(x[k]) for k in ("inmask", "col_index", "area", "width", "length", "conv"))
    torch.cuda.synchronize()
    planes, cur = [o0, o1], 0
    for _ in range(nstep):
        eng.route_kinematic(eng.route_kinematic_block(m, col, area, width, length, conv, sd, planes[cur], planes[1 - cur], ra, rb, x["scale"], x["dt"],
                                                      depth=hd if with_depth else None, diag=diag), x["ncol"])
        cur = 1 - cur
    eng.stream_sync()
    g = gpool.cpu().numpy()
    ok = _guards_ok(pool, ncell, POISON) and (g[:3] == 77).all() and (g[5:] == 77).all() and (diag is not None or (g == 77).all())
    ok = ok and (with_depth or (hd.cpu().numpy() == POISON).all())
    return (sd.cpu().numpy(), planes[cur].cpu().numpy(), hd.cpu().numpy() if with_depth else None,
            g[3:5].view(U32).copy() if diag is not None else None), ok


@pytest.mark.gpu
@pytest.mark.parametrize("ni, nj", WINDOWS + [CUT])
def test_gpu_route_kinematic_equals_the_restatement(engine, ni, nj):
    """noahmp_hip_route_kinematic against np_route_kinematic in every word of storage, out, depth and both diag words after 1, 2 and 25
    calls: the cases of the host test (diag starts at [3, 5]: the call accumulates and never zeroes; without diag and depth the other
    planes keep their bits and nothing else is written); guard words keep the poison.  (65, 5) and (67, 35): the last workgroup is partly
    past ncell; (1, 1): one live lane.  An empty window writes nothing."""
    import torch
    for what, x, storage, out, wd, wg, nstep, want in kin_cases(ni, nj):
        got, ok = _gpu_krun(engine, x, storage, out, nstep, wd, np.array([3, 5], U32) if wg else None)
        assert_run(got, want, what)
        assert ok, what + ": guard words"
    what, x, storage, out, wd, wg, nstep, want = kin_cases(ni, nj)[0]
    pool, (sd, o0, o1, hd) = _pool(ni * nj, 4, torch.float32, POISON)
    diag = torch.full((2,), 77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    b = engine.route_kinematic_block(*(_dev(x[k]) for k in ("inmask", "col_index", "area", "width", "length", "conv")), sd.view(nj, ni),
                                     o0.view(nj, ni), o1.view(nj, ni), _dev(x["runoff_a"]), None, SCALE, DT, depth=hd.view(nj, ni), diag=diag)
    b.nj = 0
    engine.route_kinematic(b, ni * nj)
    engine.stream_sync()
    assert (pool.cpu().numpy() == POISON).all() and (diag.cpu().numpy() == 77).all()


@pytest.mark.gpu
def test_gpu_diag_accumulates_and_null_diag_changes_nothing(engine):
    """Two runs of 5 calls on the 67 x 35 hills: with diag the words after 5 calls are the maximum and the sum over all five (never
    zeroed in between); a second batch on top of them only grows them; without diag and depth storage and out have the same bits."""
    ni, nj = 67, 35
    ops = kin_operands(ni, nj, "physical")
    x = _kblock(trt.hills_network(ni, nj)[1], np.arange(ni * nj, dtype=np.int32).reshape(nj, ni), ni * nj, ops)
    want = np_krun(x, ops["storage"], ops["out"], 5, np.zeros((nj, ni), F), np.zeros(2, U32))
    got, ok = _gpu_krun(engine, x, ops["storage"], ops["out"], 5, True, np.zeros(2, U32))
    assert_run(got, want, "with diag")
    assert ok
    per_call = [np_krun(x, ops["storage"], ops["out"], n, None, np.zeros(2, U32))[3] for n in range(1, 6)]
    assert int(want[3][1]) == int(per_call[-1][1]) > int(per_call[0][1]) > 0, "the count is the sum over the calls"
    bare, ok = _gpu_krun(engine, x, ops["storage"], ops["out"], 5, False, None)
    assert ok and bare[2] is None and bare[3] is None
    assert_same(bare[0], want[0], "storage without diag and depth")
    assert_same(bare[1], want[1], "out without diag and depth")
    again, ok = _gpu_krun(engine, x, ops["storage"], ops["out"], 5, False, want[3])
    assert int(again[3][1]) == 2 * int(want[3][1]) and int(again[3][0]) == int(want[3][0])


@pytest.mark.gpu
@pytest.mark.parametrize("ni, nj", [(65, 5), (67, 35)])
def test_gpu_column_order(engine, ni, nj):
    """A sorted store followed through col_index: the planes and the diag words are those of the unsorted run."""
    ops = kin_operands(ni, nj, "physical")
    x = _kblock(trt.hills_network(ni, nj)[1], np.arange(ni * nj, dtype=np.int32).reshape(nj, ni), ni * nj, ops)
    want = np_krun(x, ops["storage"], ops["out"], 10, np.zeros((nj, ni), F), np.zeros(2, U32))
    for xx, nm in ((x, "identity"), (_permuted(x, ops, ni, nj), "permuted")):
        got, ok = _gpu_krun(engine, xx, ops["storage"], ops["out"], 10, True, np.zeros(2, U32))
        assert_run(got, want, nm)
        assert ok


class _RingFromOwners:
    """A stand-in for Comm in one process: exchange_halo copies the ring of the plane from the whole-domain out plane of the same call
    (the restatement's), enqueued only on torch's current stream."""

    def __init__(self, whole_planes, blk, ring):
        self.whole, self.blk, self.ring, self.calls = whole_planes, blk, ring, 0

    def exchange_halo(self, planes, geom):
        import torch
        assert len(planes) == 1 and geom == "geom"
        planes[0].copy_(torch.where(self.ring, self.whole[self.calls][self.blk], planes[0]))
        self.calls += 1


@pytest.mark.gpu
def test_gpu_decomposition(engine):
    """ChannelFlow.step(comm=..., nsub=2) on the four parts of 70 x 130 (set_terrain on margin-2 windows, set_geometry with the height
    window cut to the block), ten steps = 20 calls, the ring of out refreshed after every call: storage, out and depth have 0 differing
    words against the whole-domain restatement; the maximum of the four diag[0] and the sum of the four diag[1] are the whole's."""
    import types
    import torch
    from noahmp_amd.routing import ChannelFlow, FlowNetwork
    ni, nj = CUT
    nstep, nsub, dt = 10, 2, 2 * DT
    z = tsh.terrain(ni, nj, True)
    ops = kin_operands(ni, nj, "physical")
    d = np_flow_dir(z, DX, DY)
    n = np.random.default_rng(8).uniform(0.03, 0.08, (nj, ni)).astype(F)
    length, conv, _ = np_flow_channel(d, n, DX, DY, SMIN, height=z)
    ncell = ni * nj
    x = dict(_kblock(np_inmask(d), np.arange(ncell, dtype=np.int32).reshape(nj, ni), ncell, ops), length=length, conv=conv,
             scale=float(F(dt) * F(1e-3)) / nsub, dt=dt / nsub)
    S, planes, cur, whole, H, G = ops["storage"].copy(), [ops["out"].copy(), ops["out"].copy()], 0, [], np.zeros((nj, ni), F), np.zeros(2, U32)
    for _ in range(nstep * nsub):
        S, planes[1 - cur], H, G = np_route_kinematic(x, planes[cur], planes[1 - cur], S, H, G)
        cur = 1 - cur
        whole.append(_dev(planes[cur]))
    torch.cuda.synchronize()
    bits, capped, differ = [], 0, 0
    for (tile, win, idx), (_, blk, bidx) in zip(tsh._cuts(ni, nj, 2), tsh._cuts(ni, nj, 1)):
        tj, ti = tile
        net = FlowNetwork(engine, ti.stop - ti.start, tj.stop - tj.start)
        net.set_terrain(_dev(z[win]), DX, DY, origin=(ti.start - win[1].start, tj.start - win[0].start))
        net.set_area(_dev(ops["area"][blk]))
        net.set_input_columns(None)
        net.storage.copy_(_dev(ops["storage"][blk]))
        for o in net.out:
            o.copy_(_dev(ops["out"][blk]))
        ch = ChannelFlow(net)
        ch.set_geometry(_dev(ops["width"][blk]), _dev(n[blk]), smin=SMIN, height=_dev(z[win]))
        own = bidx >= 0
        assert_same(ch.length.cpu().numpy()[own], length[blk][own], "part %s: length on the tile" % (tile,))
        assert_same(ch.conv.cpu().numpy()[own], conv[blk][own], "part %s: conv on the tile" % (tile,))
        store = types.SimpleNamespace(ni=net.ni, nj=net.nj, a=dict(runsfxy=_dev(ops["runoff_a"].reshape(nj, ni)[tile]),
                                                                   runsbxy=_dev(ops["runoff_b"].reshape(nj, ni)[tile])))
        comm = _RingFromOwners(whole, blk, _dev(~own))
        torch.cuda.synchronize()
        for _ in range(nstep):
            ch.step(store, dt, nsub=nsub, comm=comm, geom="geom")
        engine.stream_sync()
        torch.cuda.synchronize()
        assert comm.calls == nstep * nsub and net.last_dt == dt / nsub
        differ += trt._differ(net.tile_view(net.storage).cpu().numpy(), S[tile]) + trt._differ(net.out[net.cur].cpu().numpy(), planes[cur][blk])
        differ += trt._differ(net.tile_view(ch.depth()).cpu().numpy(), H[tile])
        w = ch.diag.cpu().numpy().view(U32)
        bits.append(int(w[0]))
        capped += ch.capped()
        assert ch.courant() == 5.0 / 3.0 * float(w[:1].view(F)[0])
    assert differ == 0
    assert max(bits) == int(G[0]) and capped == int(G[1]) and capped > 0


@pytest.mark.gpu
def test_gpu_refusals_launch_nothing(engine):
    """The refusals with device planes: -105, the full texts of the fixture, and every plane keeps its poison."""
    import torch
    fl = torch.full((len(GEOM_PLANES) + len(KIN_PLANES), 32), POISON, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    gp = {k: fl[n].data_ptr() for n, k in enumerate(GEOM_PLANES)}
    kp = {k: fl[len(GEOM_PLANES) + n].data_ptr() for n, k in enumerate(KIN_PLANES)}
    _refusals(engine.lib, gp, kp)
    engine.stream_sync()
    torch.cuda.synchronize()
    assert (fl.cpu().numpy() == POISON).all()


@pytest.mark.gpu
def test_gpu_set_geometry_and_width(engine):
    """set_geometry takes net.filled by default, raises without a surface, asserts width > 0; reset_diag zeroes the words."""
    from noahmp_amd.routing import ChannelFlow, FlowNetwork
    ni, nj = 67, 35
    z = tsh.terrain(ni, nj)
    net = FlowNetwork(engine, ni, nj)
    net.set_terrain(_dev(z), DX, DY)
    ch = ChannelFlow(net)
    with pytest.raises(ValueError, match="slope"):
        ch.set_geometry(10.0, 0.05)
    with pytest.raises(AssertionError):
        ch.set_geometry(0.0, 0.05, height=_dev(z))
    net.set_terrain(_dev(z), DX, DY, fill=1e-3)
    ch = ChannelFlow(net)
    ch.set_geometry(10.0, 0.05)
    filled = net.filled.cpu().numpy()
    wl, wc, _ = np_flow_channel(net.dir.cpu().numpy(), np.full((nj, ni), 0.05, F), DX, DY, 1e-4, height=filled)
    assert_same(ch.length.cpu().numpy(), wl, "length from the filled surface")
    assert_same(ch.conv.cpu().numpy(), wc, "conv from the filled surface")
    ch.diag.fill_(9)
    ch.reset_diag()
    assert ch.capped() == 0 and ch.courant() == 0.0


def _channel_engine_run(engine, tables, height, sort, route):
    """Three engine steps of the 35 x 67 mixed tile at a rainy hour, each followed by ChannelFlow.step(nsub=2)."""
    import torch
    from noahmp_amd import synth
    from noahmp_amd.routing import ChannelFlow, FlowNetwork
    T, tb = tables
    s = synth.mixed_small(tb, ni=trt.ENG_NI, nj=trt.ENG_NJ)
    lake = np.random.default_rng(11).random((trt.ENG_NJ, trt.ENG_NI)) < 0.06
    s.a["ivgtyp"][lake] = s.cfg.iswater
    s.a["xland"][lake] = 2.0
    synth.first_step_fixups(s)
    synth.diurnal_forcing(s, 11, t_offset=s.t_offset)
    d = s.to_device("cuda:0")
    torch.cuda.synchronize()
    net = ch = None
    if route:
        net = FlowNetwork(engine, trt.ENG_NI, trt.ENG_NJ)
        net.set_terrain(_dev(height), DX, DX, origin=(trt.ENG_MARGIN, 0))
        ch = ChannelFlow(net)
        ch.set_geometry(20.0, 0.05, height=_dev(height))
    perm = None
    if sort:
        engine.sort_store(d)
        perm = d.sort_perm.cpu().numpy()
        if route:
            ch.follow(d)
    seen = []
    for it in range(1, trt.ENG_STEPS + 1):
        st = engine.noahmplsm(d, it, 2000, 180.0)
        assert st.code == 0
        if route:
            ch.step(d, d.cfg.dt, nsub=2)
            engine.stream_sync()
        planes = []
        for k in ("runsfxy", "runsbxy"):
            p = d.a[k].cpu().numpy().ravel().copy()
            if perm is not None:
                t = np.empty_like(p)
                t[perm] = p
                p = t
            planes.append(p)
        seen.append(planes)
    return d, net, ch, seen


@pytest.mark.gpu
def test_gpu_engine_run_in_a_valley(engine, tables):
    """Three noahmplsm steps of a 35 x 67 mixed tile in the valley terrain, each followed by ChannelFlow.step(nsub=2): storage, out, depth
    and diag equal the restatement driven by the store's own runoff planes; the sorted store gives identical planes; every array of the
    store is bit-identical to the run without routing; discharge() and state_dict() work as with FlowNetwork.step; courant() is finite."""
    from tools.compare import exact_check
    height = tsv._valley()
    d, net, ch, seen = _channel_engine_run(engine, tables, height, False, True)
    dt = d.cfg.dt
    x = dict(inmask=net.inmask.cpu().numpy(), col_index=net.col_index.cpu().numpy(), ncol=trt.ENG_NI * trt.ENG_NJ, area=net.area.cpu().numpy(),
             width=ch.width.cpu().numpy(), length=ch.length.cpu().numpy(), conv=ch.conv.cpu().numpy(), scale=float(F(dt) * F(1e-3)) / 2, dt=dt / 2)
    blk = (slice(None), slice(trt.ENG_MARGIN - 1, trt.ENG_MARGIN + trt.ENG_NI + 1))
    wl, wc, _ = np_flow_channel(net.dir.cpu().numpy(), np.full(net.block_shape, 0.05, F), DX, DX, 1e-4, height=height[blk])
    own = x["col_index"] >= -1
    assert_same(x["length"][own], wl[own], "length")
    assert_same(x["conv"][own], wc[own], "conv")
    S = np.zeros(net.block_shape, F)
    planes, cur, H, G = [S.copy(), S.copy()], 0, S.copy(), np.zeros(2, U32)
    for ra, rb in seen:
        x["runoff_a"], x["runoff_b"] = ra, rb
        for _ in range(2):
            S, planes[1 - cur], H, G = np_route_kinematic(x, planes[cur], planes[1 - cur], S, H, G)
            cur = 1 - cur
    got = (net.storage.cpu().numpy(), net.out[net.cur].cpu().numpy(), ch.depth().cpu().numpy(), ch.diag.cpu().numpy().view(U32))
    assert_run(got, (S, planes[cur], H, G), "valley run")
    assert (planes[cur] > 0).any() and net.last_dt == dt / 2
    courant = ch.courant()
    assert np.isfinite(courant) and courant == 5.0 / 3.0 * float(G[:1].view(F)[0]) and courant > 0 and ch.capped() == int(G[1])
    q, q64 = net.discharge().cpu().numpy().astype(np.float64), planes[cur].astype(np.float64) / (dt / 2)
    assert (np.abs(q - q64) <= 3 * EPS * np.abs(q64)).all() and (q64 > 0).any()
    ds, nets, chs, seen_s = _channel_engine_run(engine, tables, height, True, True)
    assert (ds.sort_perm.cpu().numpy() != np.arange(trt.ENG_NI * trt.ENG_NJ)).any()
    got_s = (nets.storage.cpu().numpy(), nets.out[nets.cur].cpu().numpy(), chs.depth().cpu().numpy(), chs.diag.cpu().numpy().view(U32))
    assert_run(got_s, (S, planes[cur], H, G), "sorted valley run")
    without, _, _, _ = _channel_engine_run(engine, tables, height, False, False)
    ok, lines = exact_check(without.to_host(), d.to_host())
    assert ok, "\n".join(lines)
    state = net.state_dict()
    net.storage.zero_()
    net.out[net.cur].zero_()
    net.load_state_dict(state)
    assert_same(net.storage.cpu().numpy(), S, "the restart state: storage")
    assert_same(net.out[net.cur].cpu().numpy(), planes[cur], "the restart state: out")
