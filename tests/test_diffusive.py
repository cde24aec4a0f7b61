"""Diffusive-wave routing on the D8 network: backwater, also from lakes (noahmp_hip_flow_drop, noahmp_hip_route_diffusive,
noahmp_hip_lake_depth; nmp_dev_diffusive.hpp, nmp_dev_lakes.hpp; routing.DiffusiveFlow, routing.Lakes.set_datum).

No reference routine stands behind the calls; the contract is the text in include/noahmp_hip.h.  np_flow_drop, np_route_diffusive and
np_lake_depth restate it in numpy, one rounded operation per line (float32; float64 for the lake's stage), with glibc's own powf called
per element through ctypes (test_channel.powf).  Everything is compared with the restatement bit for bit (test_regrid.assert_same: equal
bits, or both NaN): the per-cell functions compiled for the host in both forms of the downstream-depth access, the three kernels, the
variant library with the other form, and engine runs through DiffusiveFlow and Lakes.  diag[0] holds float32 bits and is compared as a
float; diag[1..3] are compared as words.  A tolerance appears only in the budget check; where it comes from is counted there."""
import ctypes as C
import functools
import json
import os
import subprocess

import numpy as np
import pytest

from noahmp_amd import abi
import test_channel as tc
import test_lakes as tl
import test_regrid as tr
import test_routing as trt
import test_shadow as tsh
import test_skyview as tsv
from test_channel import DT, SCALE, SMIN, TWO_THIRDS, np_flow_channel, np_route_kinematic, powf
from test_regrid import F, assert_same, nasty
from test_routing import CUT, DX, DY, EPS, POISON, U32, WINDOWS, neighbour, np_flow_dir, np_inmask, np_inverse_distances

ROOT = tr.ROOT
CSRC = tr.CSRC
SRC = os.path.join(ROOT, "tests", "host_emul", "diffusive_check.hip")
LIB = os.path.join(ROOT, "tests", "host_emul", "libdiffusive_check.so")
DEFAULT_LOAD_ALL = 0                                                     # NMP_DIFFUSIVE_LOAD_ALL of noahmp_diffusive.hip as the library is built
LIB_OTHER = os.path.join(CSRC, "variants", "lib_diffusive_hd_other.so")  # the library with the other form of the downstream-depth access
HEADER = os.path.join(ROOT, "include", "noahmp_hip.h")
REFUSAL_FIXTURE = os.path.join(ROOT, "tests", "golden", "diffusive_refusal_text.json")
LIMIT = 0.5
F8 = np.float64
I64 = np.int64
Q = tl.Q


# ---------------------------------------------------------------------------------------------------------------- the restatement
def _k_of(dirp):
    d = np.asarray(dirp, np.uint8)
    return np.where(d > 8, 0, d).astype(np.int64)


def np_flow_drop(dirp, dx, dy, height=None, slope=None):
    """noahmp_hip_flow_drop over a window: the drop plane."""
    assert (height is None) != (slope is None)
    k = _k_of(dirp)
    with np.errstate(all="ignore"):
        if slope is not None:
            length = np.where((k == 0) | (k == 1) | (k == 5), F(dx), np.where((k == 3) | (k == 7), F(dy), tc.np_diagonal(dx, dy))).astype(F)
            drop = np.asarray(slope, F) * length
        else:
            z = np.asarray(height, F)
            drop = np.zeros(z.shape, F)
            for kk in range(1, 9):
                zn, inside = neighbour(z, kk)
                dz = z - zn
                drop = np.where((k == kk) & inside, dz, drop).astype(F)
    assert drop.dtype == F
    return drop


def np_downstream(dirp, plane):
    """(the plane's value at every cell's downstream cell, has = the cell has a downstream cell inside the window)."""
    k = _k_of(dirp)
    p = np.asarray(plane, F)
    hd, has = p.copy(), np.zeros(k.shape, bool)
    for kk in range(1, 9):
        dn, inside = neighbour(p, kk)
        pick = (k == kk) & inside
        hd = np.where(pick, dn, hd).astype(F)
        has |= pick
    return hd, has


def np_route_diffusive(x, out_old, out_new, storage, depth_old, depth_new, diag=None, detail=None):
    """One call of noahmp_hip_route_diffusive over the window of x (a dict of the block's members): (storage', out_new', depth_new',
    diag').  diag None: not given to the call.  detail: a dict that receives the masks of the paths and the dh plane."""
    m = np.asarray(x["inmask"], np.uint8)
    col = np.asarray(x["col_index"], np.int64)
    ncol = int(x["ncol"])
    owned = (col >= -1) & (col < ncol)
    local = owned & (col >= 0)
    scale, dt, limit = F(x["scale"]), F(x["dt"]), F(x["limit"])
    width, length, conv, manning, drop = (np.asarray(x[k], F) for k in ("width", "length", "conv", "manning", "drop"))
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
        hd, has = np_downstream(x["dir"], depth_old)
        wl = width * length
        enter = owned & (s1 > 0) & (conv > 0)
        h = s1 / wl
        dd = h - hd
        dh = drop + dd
        open_ = np.where(has, dh > 0, True)
        sf = dh / length
        r = np.sqrt(sf)
        cvd_d = r / manning
        cvd = np.where(has, cvd_d, conv).astype(F)
        half = limit * dh
        lim = half * wl
        go = enter & open_
        a = width * h
        h2 = h + h
        p = width + h2
        R = a / p
        r23 = np.zeros(m.shape, F)
        r23[go] = powf(R[go], TWO_THIRDS)
        vel = cvd * r23
        qa = vel * a
        od = qa * dt
        capped0 = go & ~(od < s1)
        o = np.where(capped0, s1, od).astype(F)
        limited = go & has & (lim < o)
        o = np.where(limited, lim, o).astype(F)
        o = np.where(go, o, F(0.0)).astype(F)
        vd = vel * dt
        cr = np.where(go, vd / length, F(0.0)).astype(F)
        blocked = enter & ~open_
        s2 = s1 - o
        h1 = s2 / wl
        dnew = np.where(s2 > 0, h1, F(0.0)).astype(F)
    assert all(t.dtype == F for t in (q, xs, v, sv, s1, hd, wl, h, dd, dh, sf, r, cvd, half, lim, a, h2, p, R, vel, qa, od, o, vd, cr, s2, h1, dnew))
    capped = capped0 & ~limited
    if diag is not None:
        show = owned & ((cr > 0) | np.isnan(cr))
        diag = np.array([max(int(diag[0]), int(tc.bits_of(cr)[show].max()) if show.any() else 0), (int(diag[1]) + int(capped.sum())) & 0xFFFFFFFF,
                         (int(diag[2]) + int(limited.sum())) & 0xFFFFFFFF, (int(diag[3]) + int(blocked.sum())) & 0xFFFFFFFF], U32)
    if detail is not None:
        detail.update(open=go & has, blocked=blocked, limited=limited, capped=capped, outlet=enter & ~has, held=owned & (s1 > 0) & ~(conv > 0),
                      ring=~owned, nan_dh=enter & has & np.isnan(dh), dh=dh, s1=s1, enter=enter, has=has)
    return (np.where(owned, s2, storage).astype(F), np.where(owned, o, out_new).astype(F), np.where(owned, dnew, depth_new).astype(F), diag)


def np_drun(x, storage, out, depth, nstep, diag=None):
    """nstep calls, ping-ponging two out planes that both start as `out` and two depth planes that both start as `depth`:
    (storage, out, depth, diag)."""
    planes = [np.array(out, F), np.array(out, F)]
    deps = [np.array(depth, F), np.array(depth, F)]
    storage = np.array(storage, F)
    cur = 0
    for _ in range(nstep):
        storage, planes[1 - cur], deps[1 - cur], diag = np_route_diffusive(x, planes[cur], planes[1 - cur], storage, deps[cur], deps[1 - cur], diag)
        cur = 1 - cur
    return storage, planes[cur], deps[cur], diag


def np_lake_depth(member_cell, member_lake, nmember, volume, area, datum, bed, depth, q):
    """One call of noahmp_hip_lake_depth in float64: the depth plane."""
    out = np.array(depth, F)
    flat, b = out.reshape(-1), np.asarray(bed, F).reshape(-1)
    vol, area, datum = np.asarray(volume, I64), np.asarray(area, F8), np.asarray(datum, F8)
    q = F8(q)
    with np.errstate(all="ignore"):
        for e in range(int(nmember)):
            c, l = int(member_cell[e]), int(member_lake[e])
            if not (0 <= c < flat.size and 0 <= l < vol.size):
                continue
            volm = F8(float(vol[l])) * q
            h = volm / area[l] if area[l] > 0 else F8(0.0)
            el = datum[l] + h
            d = el - F8(b[c])
            flat[c] = F(d) if d > 0 else F(0.0)
    return out


# ---------------------------------------------------------------------------------------------------------------- the inputs
def diff_operands(ni, nj, which, seed=0):
    """The operands of test_channel.kin_operands plus dir, manning, drop and depth: half of the drops are the hills' own (steep: open,
    capped), half gentle or adverse (blocked, limited); `nasty`: NaN / Inf / denormal / negative words in every plane."""
    ops = tc.kin_operands(ni, nj, which, seed)
    r = np.random.default_rng(7000 + ni * nj + len(which) + seed)
    z = tsh.terrain(ni, nj)
    d = np_flow_dir(z, DX, DY)
    steep = np_flow_drop(d, DX, DY, height=z)
    gentle = r.uniform(-0.05, 0.1, (nj, ni)).astype(F)
    ops["drop"] = np.where(r.random((nj, ni)) < 0.5, gentle, steep).astype(F)
    ops["manning"] = tc.manning_plane(ni, nj)                            # the plane conv was made from: 0, negative and NaN among them
    ops["depth"] = r.uniform(0.0, 0.12, (nj, ni)).astype(F)
    ops["dir_hills"] = d
    if which == "nasty":
        for k in ("drop", "manning", "depth"):
            ops[k] = np.where(r.random((nj, ni)) < 0.25, nasty(r, ni * nj).reshape(nj, ni), ops[k]).astype(F)
    return ops


def _dblock(dirp, mask, col, ncol, ops, rb=True, limit=LIMIT):
    return dict(inmask=mask, col_index=col, ncol=ncol, dir=dirp, area=ops["area"], width=ops["width"], length=ops["length"], conv=ops["conv"],
                manning=ops["manning"], drop=ops["drop"], runoff_a=ops["runoff_a"], runoff_b=ops["runoff_b"] if rb else None, scale=SCALE,
                dt=DT, limit=limit)


OPTS = ((True, True), (False, False), (True, False), (False, True))      # (runoff_b, diag)
DIAG0 = (3, 5, 7, 11)                                                    # the call accumulates and never zeroes


@functools.lru_cache(maxsize=None)
def diff_cases(ni, nj):
    """[(what, x, storage, out, depth, diag given, nstep, (storage, out, depth, diag) of the restatement)] -- made once, shared by the
    host and the device tests.  Physical and nasty operands, identity / permuted / mixed col_index (ring cells and cells without local
    input), the hills' directions with their inmask and random directions (bytes above 8, directions out of the window) with random
    inmask bytes, with and without runoff_b and diag, two limits, 1, 2 and 25 calls."""
    wild = np.random.default_rng(ni * 7 + nj).integers(0, 256, (nj, ni)).astype(np.uint8)
    big = ni * nj > 5000
    out, n = [], 0
    for which in ("physical", "nasty"):
        ops = diff_operands(ni, nj, which)
        for cname, col, ncol in trt.col_indices(ni, nj):
            for dname, dirp, mask in (("hills", ops["dir_hills"], np_inmask(ops["dir_hills"])), ("random", trt.random_dir(ni, nj), wild)):
                if big and (dname == "random") != (cname == "mix"):
                    continue                                             # the large window: the two diagonal combinations
                rb, wg = OPTS[n % 4]
                limit = (LIMIT, 0.2)[(n // 4) % 2]
                n += 1
                x = _dblock(dirp, mask, col, ncol, ops, rb, limit)
                for nstep in ((25,) if big else (1, 2, 25)):
                    what = "%dx%d %s %s dir %s rb %s diag %s limit %g, %d calls" % (ni, nj, which, cname, dname, rb, wg, limit, nstep)
                    want = np_drun(x, ops["storage"], ops["out"], ops["depth"], nstep, np.array(DIAG0, U32) if wg else None)
                    out.append((what, x, ops["storage"], ops["out"], ops["depth"], wg, nstep, want))
    return out


# ---------------------------------------------------------------------------------------------------------------- CPU
def build():
    """The host checker: nmp_dev_diffusive.hpp and nmp_dev_lakes.hpp compiled for the CPU.  Needs nothing of the engine library."""
    deps = [SRC, HEADER] + [os.path.join(CSRC, h) for h in ("nmp_dev_diffusive.hpp", "nmp_dev_channel.hpp", "nmp_dev_routing.hpp",
                                                            "nmp_dev_lakes.hpp", "nmp_libm.hpp", "nmp_libm_tables.inc")]
    if not os.path.exists(LIB) or any(os.path.getmtime(p) > os.path.getmtime(LIB) for p in deps):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off",
                               "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), SRC, "-o", LIB])


def build_variant():
    """The variant library with the other form of the downstream-depth access: one translation unit compiled again."""
    from noahmp_amd import build as b
    b.build_unit_variant("noahmp_diffusive.hip", ["-DNMP_DIFFUSIVE_LOAD_ALL=%d" % (1 - DEFAULT_LOAD_ALL)], LIB_OTHER)


@functools.lru_cache(maxsize=None)
def _host():
    build()
    try:
        import torch  # noqa: F401  (map torch's HIP runtime first, noahmp_amd/abi.py::load_library)
    except ImportError:
        pass
    lib = C.CDLL(LIB)
    V, Fl, I, L, D = C.c_void_p, C.c_float, C.c_int, C.c_longlong, C.c_double
    lib.flow_drop_cells.argtypes = [I, I, V, V, V, V, Fl, Fl]
    lib.diffusive_cells.argtypes = [I, I] + [V] * 17 + [Fl, Fl, Fl, C.c_long, I]
    lib.lake_depth_entries.argtypes = [V, V, L, V, V, V, V, V, I, L, D]
    lib.flow_drop_cells.restype = lib.diffusive_cells.restype = lib.lake_depth_entries.restype = None
    return lib


_p, _c = trt._p, trt._c


def host_flow_drop(dirp, dx, dy, height=None, slope=None):
    d = _c(dirp, np.uint8)
    nj, ni = d.shape
    z = _c(height) if height is not None else None
    s = _c(slope) if slope is not None else None
    drop = np.full(d.shape, POISON, F)
    _host().flow_drop_cells(ni, nj, _p(z), _p(s), _p(d), _p(drop), float(dx), float(dy))
    return drop


def host_one(x, out_old, out_new, storage, depth_old, depth_new, diag=None, load_all=0):
    """One call of the compiled per-cell function over the window: (storage', out_new', depth_new', diag')."""
    m = _c(x["inmask"], np.uint8)
    nj, ni = m.shape
    s, o, dn = _c(storage).copy(), _c(out_new).copy(), _c(depth_new).copy()
    g = _c(diag, U32).copy() if diag is not None else None
    keep = [_c(x["col_index"], np.int32), _c(x["dir"], np.uint8)] + [_c(x[k]) for k in ("area", "width", "length", "conv", "manning", "drop")] + \
           [_c(out_old), _c(x["runoff_a"]), _c(x["runoff_b"]) if x.get("runoff_b") is not None else None, _c(depth_old)]
    col, dirp, area, width, length, conv, manning, drop, old, ra, rb, dold = keep
    _host().diffusive_cells(ni, nj, _p(m), _p(col), _p(dirp), _p(area), _p(width), _p(length), _p(conv), _p(manning), _p(drop), _p(s), _p(old),
                            _p(o), _p(ra), _p(rb), _p(dold), _p(dn), _p(g), float(x["scale"]), float(x["dt"]), float(x["limit"]), int(x["ncol"]),
                            int(load_all))
    return s, o, dn, g


def host_drun(x, storage, out, depth, nstep, diag=None, load_all=0):
    planes = [_c(out).copy(), _c(out).copy()]
    deps = [_c(depth).copy(), _c(depth).copy()]
    storage = _c(storage).copy()
    cur = 0
    for _ in range(nstep):
        storage, planes[1 - cur], deps[1 - cur], diag = host_one(x, planes[cur], planes[1 - cur], storage, deps[cur], deps[1 - cur], diag, load_all)
        cur = 1 - cur
    return storage, planes[cur], deps[cur], diag


def host_lake_depth(member_cell, member_lake, nmember, volume, area, datum, bed, depth, q):
    mc, ml = _c(member_cell, np.int32), _c(member_lake, np.int32)
    vol, ar, da, b, out = _c(volume, I64), _c(area, F8), _c(datum, F8), _c(bed), _c(depth).copy()
    _host().lake_depth_entries(_p(mc), _p(ml), int(nmember), _p(vol), _p(ar), _p(da), _p(b), _p(out), vol.size, out.size, float(q))
    return out


def assert_run(got, want, what):
    """(storage, out, depth, diag) of a run against the restatement's: every word; diag[0] as the float it holds."""
    for g, w, nm in zip(got[:3], want[:3], ("storage", "out", "depth")):
        assert_same(g, w, "%s: %s" % (what, nm))
    assert (got[3] is None) == (want[3] is None), what
    if want[3] is not None:
        g, w = np.asarray(got[3]).view(U32), np.asarray(want[3]).view(U32)
        assert_same(g[:1].view(F), w[:1].view(F), what + ": diag[0]")
        assert g[1:].tolist() == w[1:].tolist(), (what, "diag[1..3]", g[1:].tolist(), w[1:].tolist())


def _inv_plane(dirp, dx, dy):
    inv_x, inv_y, inv_d = np_inverse_distances(dx, dy)
    k = _k_of(dirp)
    return np.where(k % 2 == 0, inv_d, np.where((k == 3) | (k == 7), inv_y, inv_x)).astype(F)


@pytest.mark.parametrize("ni, nj", WINDOWS + [CUT])
def test_host_flow_drop_equals_the_restatement(ni, nj):
    """flow_drop_cell compiled for the host against np_flow_drop in every word: the cases of test_channel.geom_cases.  With heights
    drop * inv[k] is, in every bit, the slope before the floor of np_flow_channel at the cells with a downstream cell, and the drop is +0
    at the others; with slopes it is slope * len."""
    for name, d, n, dx, dy, z, s in tc.geom_cases(ni, nj):
        want = np_flow_drop(d, dx, dy, height=z, slope=s)
        assert_same(host_flow_drop(d, dx, dy, height=z, slope=s), want, "%dx%d %s: drop" % (ni, nj, name))
        length, _, sl = np_flow_channel(d, n, dx, dy, SMIN, height=z, slope=s)
        with np.errstate(all="ignore"):
            if z is not None:
                _, has = np_downstream(d, np.zeros((nj, ni), F))
                assert_same((want * _inv_plane(d, dx, dy)).astype(F)[has], sl[has], "%s: drop * inv is the slope that won" % name)
                assert (want[~has].view(U32) == 0).all(), "+0 where there is no downstream cell"
            else:
                assert_same(want, (np.asarray(s, F) * length).astype(F), "%s: slope * len" % name)


@pytest.mark.parametrize("ni, nj", WINDOWS + [CUT])
def test_host_route_diffusive_equals_the_restatement(ni, nj):
    """diffusive_cell compiled for the host, in both forms of the downstream-depth access, against np_route_diffusive in every word of
    storage, out, depth and diag: the cases of diff_cases.  Cells that are not owned keep their storage and the poison of out_new and
    depth_new, and report nothing."""
    for what, x, storage, out, depth, wg, nstep, want in diff_cases(ni, nj):
        for load_all in (0, 1):
            got = host_drun(x, storage, out, depth, nstep, np.array(DIAG0, U32) if wg else None, load_all)
            assert_run(got, want, "%s, load_all %d" % (what, load_all))
    ops = diff_operands(ni, nj, "physical")
    poison = np.full((nj, ni), POISON, F)
    for cname, col, ncol in trt.col_indices(ni, nj)[2:]:
        c64 = col.astype(np.int64)
        ring = (c64 < -1) | (c64 >= ncol)
        assert ring.any() or ni * nj < 4
        x = _dblock(ops["dir_hills"], np_inmask(ops["dir_hills"]), col, ncol, ops)
        s1, o1, h1, g1 = np_route_diffusive(x, ops["out"], poison, ops["storage"], ops["depth"], poison, np.zeros(4, U32))
        for plane, keep, nm in ((o1, poison, "out_new"), (h1, poison, "depth_new"), (s1, ops["storage"], "storage")):
            assert_same(plane[ring], keep[ring], "cells that are not owned keep " + nm)
        x_all_ring = dict(x, col_index=np.full((nj, ni), -2, np.int32))
        assert np_route_diffusive(x_all_ring, ops["out"], poison, ops["storage"], ops["depth"], poison, np.zeros(4, U32))[3].tolist() == [0] * 4
        assert host_one(x_all_ring, ops["out"], poison, ops["storage"], ops["depth"], poison, np.zeros(4, U32))[3].tolist() == [0] * 4


def test_the_cases_reach_every_path():
    """The restatement's own counts over the shared cases of 67 x 35: open, blocked, limited, capped, no downstream cell, held, ring and
    a NaN dh each occur at least once; a NaN cr shows in diag[0] of a nasty case and a physical case has a finite one."""
    ni, nj = 67, 35
    counts = dict(open=0, blocked=0, limited=0, capped=0, outlet=0, held=0, ring=0, nan_dh=0)
    nan_cr = finite_cr = False
    for what, x, storage, out, depth, wg, nstep, want in diff_cases(ni, nj):
        if nstep != 1:
            continue
        detail = {}
        g = np_route_diffusive(x, out, out, storage, depth, depth, np.zeros(4, U32), detail)[3]
        for k in counts:
            counts[k] += int(detail[k].sum())
        cr = g[:1].view(F)[0]
        nan_cr |= bool(np.isnan(cr))
        finite_cr |= bool(np.isfinite(cr) and cr > 0)
        assert int(g[1]) == int(detail["capped"].sum()) and int(g[2]) == int(detail["limited"].sum()) and int(g[3]) == int(detail["blocked"].sum())
        assert not (detail["capped"] & detail["limited"]).any() and not (detail["blocked"] & detail["open"]).any()
    print("paths reached over the one-call cases of %d x %d: %r" % (ni, nj, counts))
    assert all(v >= 1 for v in counts.values()), counts
    assert nan_cr and finite_cr


def test_outlet_identity():
    """With dir zero everywhere every cell is an outlet: storage and out_new have the bits of np_route_kinematic on the same operands,
    after 1 and 10 calls, restated and compiled; nothing is limited or blocked and depth is storage / (width*length) where storage > 0."""
    ni, nj = 67, 35
    for which in ("physical", "nasty"):
        ops = diff_operands(ni, nj, which)
        col = np.arange(ni * nj, dtype=np.int32).reshape(nj, ni)
        zero_dir = np.zeros((nj, ni), np.uint8)
        x = _dblock(zero_dir, np_inmask(ops["dir_hills"]), col, ni * nj, ops)
        for nstep in (1, 10):
            ks, ko, _, kg = tc.np_krun(x, ops["storage"], ops["out"], nstep, None, np.zeros(2, U32))
            for run in (np_drun, host_drun):
                s, o, h, g = run(x, ops["storage"], ops["out"], ops["depth"], nstep, np.zeros(4, U32))
                assert_same(s, ks, "%s %d calls: storage" % (which, nstep))
                assert_same(o, ko, "%s %d calls: out" % (which, nstep))
                assert_same(g[:1].view(F), kg[:1].view(F), "diag[0]")
                assert g[1:].tolist() == [int(kg[1]), 0, 0]
                with np.errstate(all="ignore"):
                    assert_same(h, np.where(s > 0, s / (x["width"] * x["length"]), F(0.0)).astype(F), "depth at the end of the call")


# ---------------------------------------------------------------------------------------------------------------- the physics
ROW_W, ROW_L, ROW_N = 10.0, 1000.0, 0.05                                 # 10 m x 1 km cells, n = 0.05


def row_block(bed, dt, runoff=None, limit=LIMIT):
    """A row of cells draining east over the bed heights `bed` [m], the last one nowhere; runoff [mm/s] per cell or None."""
    n = len(bed)
    d = np.full((1, n), 1, np.uint8)
    d[0, -1] = 0
    z = np.asarray(bed, F).reshape(1, n)
    manning = np.full((1, n), ROW_N, F)
    length, conv, _ = np_flow_channel(d, manning, ROW_L, ROW_L, SMIN, height=z)
    assert (length == F(ROW_L)).all()
    return dict(inmask=np_inmask(d), col_index=np.arange(n, dtype=np.int32).reshape(1, n) if runoff is not None else np.full((1, n), -1, np.int32),
                ncol=n if runoff is not None else 0, dir=d, area=np.full((1, n), ROW_W * ROW_L, F), width=np.full((1, n), ROW_W, F), length=length,
                conv=conv, manning=manning, drop=np_flow_drop(d, ROW_L, ROW_L, height=z),
                runoff_a=np.asarray(runoff, F) if runoff is not None else np.zeros(1, F), runoff_b=None, scale=float(F(F(dt) * F(1e-3))), dt=dt,
                limit=limit)


def test_water_at_rest_stays_at_rest():
    """A row with bed steps that are multiples of 0.5 m and a level surface at 2 m: the depths are multiples of 0.5 m, storage = depth *
    1e4 m3 is exact, and drop + (h - hd) is exactly 0 at every cell that holds water (the last wet cell drains into a dry cell whose bed
    is at the surface).  No input.  Every out_new is +0, every storage word is unchanged after 10 calls, and diag[3] is 10 times the
    five cells that hold water and have a downstream cell; restated and compiled.  np_route_kinematic on the same row releases from the
    first call."""
    bed = [1.0, 0.5, 0.0, 0.5, 1.5, 2.0, 1.0]
    level = 2.0
    x = row_block(bed, 60.0)
    depth0 = np.maximum(F(level) - np.asarray(bed, F), F(0.0)).reshape(1, -1).astype(F)
    depth0[0, 5:] = 0.0                                                  # the rim at the surface and the dry cell below it
    storage0 = (depth0 * F(ROW_W * ROW_L)).astype(F)
    wet = int((depth0 > 0).sum())
    assert wet == 5 and (storage0[0, 5:] == 0).all()
    detail = {}
    np_route_diffusive(x, np.zeros_like(depth0), np.zeros_like(depth0), storage0, depth0, depth0, None, detail)
    assert (detail["dh"][0, :wet].view(U32) << 1 == 0).all(), "drop + (h - hd) is exactly 0 at every cell that holds water"
    zero = np.zeros_like(depth0)
    for run in (np_drun, host_drun):
        planes, deps, S, cur, g = [zero.copy(), zero.copy()], [depth0.copy(), depth0.copy()], storage0.copy(), 0, np.zeros(4, U32)
        one = np_route_diffusive if run is np_drun else host_one
        for _ in range(10):
            S, planes[1 - cur], deps[1 - cur], g = one(x, planes[cur], planes[1 - cur], S, deps[cur], deps[1 - cur], g)
            cur = 1 - cur
            assert (planes[cur].view(U32) == 0).all(), "every out_new is +0"
        assert (S.view(U32) == storage0.view(U32)).all() and (deps[cur].view(U32) == depth0.view(U32)).all()
        assert g.tolist() == [0, 0, 0, 10 * wet]
    ks, ko, _, _ = np_route_kinematic(x, zero, zero, storage0)
    assert (ko[0, :wet] > 0).all(), "the kinematic wave releases at the bed slope (at least smin) from the first call"


STEP_N, STEP_AT, STEP_CALLS = 32, 15, 1500


def _step_row(dt=60.0):
    """1 x 32, 0.5 m drop per cell, except a step of -1 m at cell 15 (its downstream cell's bed is 1 m higher); steady input of 2 m3/s
    into each of the cells 10 .. 13."""
    bed = np.zeros(STEP_N)
    for c in range(1, STEP_N):
        bed[c] = bed[c - 1] - 0.5
    bed[STEP_AT + 1:] += 1.5                                             # drop[15] = -1, the others 0.5
    runoff = np.zeros(STEP_N, F)
    runoff[10:14] = 2.0 / (ROW_W * ROW_L) * 1e3                          # mm/s over the cell's area: 2 m3/s
    x = row_block(bed, dt, runoff)
    assert x["drop"][0, STEP_AT] == -1 and (np.delete(x["drop"][0, :-1], STEP_AT) == 0.5).all()
    return x


def test_adverse_step():
    """Cell 15 releases +0 in every call in which drop + (h - hd) is not > 0, although it holds water; no cell below it holds water
    before the first releasing call; releasing begins within the run, after which the pool stands above the step.  The kinematic
    restatement passes water over the step in the very call in which it arrives."""
    x = _step_row()
    zero = np.zeros((1, STEP_N), F)
    planes, deps, S, cur, g = [zero.copy(), zero.copy()], [zero.copy(), zero.copy()], zero.copy(), 0, np.zeros(4, U32)
    first, blocked_calls = None, 0
    for t in range(STEP_CALLS):
        detail = {}
        S, planes[1 - cur], deps[1 - cur], g = np_route_diffusive(x, planes[cur], planes[1 - cur], S, deps[cur], deps[1 - cur], g, detail)
        cur = 1 - cur
        o15 = planes[cur][0, STEP_AT]
        if not detail["dh"][0, STEP_AT] > 0:
            assert o15.view(U32) == 0, "call %d: no release while the surface is not above the downstream cell's" % t
            blocked_calls += bool(detail["blocked"][0, STEP_AT])
        if o15 > 0 and first is None:
            first = t
            assert detail["s1"][0, STEP_AT] / F(ROW_W * ROW_L) > 1.0, "the pool stands above the step when it first spills"
        if first is None:
            assert (S[0, STEP_AT + 1:] == 0).all() and (planes[cur][0, STEP_AT:] == 0).all(), "call %d: nothing has passed the step" % t
    print("adverse step: cell %d held water and was blocked in %d calls, first release in call %s of %d; diag %r"
          % (STEP_AT, blocked_calls, first, STEP_CALLS, g.tolist()))
    assert first is not None and blocked_calls >= 10 and int(g[3]) >= blocked_calls
    assert (S[0, STEP_AT + 1:] > 0).any(), "after the pool spills water is on its way below the step"
    got = host_drun(x, zero, zero, zero, 200, np.zeros(4, U32))
    assert_run(got, np_drun(x, zero, zero, zero, 200, np.zeros(4, U32)), "the step, compiled")
    planes, S, cur, arrived = [zero.copy(), zero.copy()], zero.copy(), 0, None
    for t in range(STEP_CALLS):
        before = S[0, STEP_AT] + planes[cur][0, STEP_AT - 1]
        S, planes[1 - cur], _, _ = np_route_kinematic(x, planes[cur], planes[1 - cur], S)
        cur = 1 - cur
        if before > 0:
            arrived = t
            assert planes[cur][0, STEP_AT] > 0, "the kinematic wave has no backwater: it passes water uphill from the call in which it arrives"
            break
    assert arrived is not None


# ---------------------------------------------------------------------------------------------------------------- budget
# The bound is the one counted for test_channel.test_budget_on_the_hills, from the rounded operations of the header text in units of
# 2^-24: the input v = ((a + b)*scale)*area, 3 roundings; per cell and call q at most 7, sv 1, s1 1 and s2 = s1 - o 1 (o, whatever it is
# -- Manning's, capped or limited -- is the SAME float32 number that leaves the storage and enters out, and a capped cell's s1 - s1 is
# exact): 10 units of s1, and the s1 of a call add up to at most the input so far: 3 + 5 * (N + 1) units of the total input after N calls
# with constant input.  depth_new is a diagnostic of s2 and enters no budget.  (The split against a float64 run of test_channel is not
# taken over: `open` is a discontinuity, so a perturbation does not stay a perturbation.)
BUDGET_STEPS = tc.BUDGET_STEPS
BUDGET_BOUND = 3 + 5 * (BUDGET_STEPS + 1)


def test_budget_on_the_hills():
    """50 calls with constant input on the 67 x 35 hills, half of the drops gentle or adverse: storage + in flight + what has left at
    the cells without a direction against the input, under the bound counted above; water is held back (blocked and limited cells
    occur) and released.  The restatement measured 0.22 * 2^-24 of the input (bound 258)."""
    ni, nj = 67, 35
    z = tsh.terrain(ni, nj)
    d = np_flow_dir(z, DX, DY)
    outlets = d == 0
    ops = trt.route_operands(ni, nj, "physical")
    r = np.random.default_rng(6)
    manning = r.uniform(0.05, 0.2, (nj, ni)).astype(F)
    length, conv, _ = np_flow_channel(d, manning, DX, DY, SMIN, height=z)
    drop = np.where(r.random((nj, ni)) < 0.5, r.uniform(-0.05, 0.1, (nj, ni)), np_flow_drop(d, DX, DY, height=z)).astype(F)
    x = dict(inmask=np_inmask(d), col_index=np.arange(ni * nj, dtype=np.int32).reshape(nj, ni), ncol=ni * nj, dir=d, area=ops["area"],
             width=r.uniform(50.0, 300.0, (nj, ni)).astype(F), length=length, conv=conv, manning=manning, drop=drop, runoff_a=ops["runoff_a"],
             runoff_b=ops["runoff_b"], scale=float(F(F(300.0) * F(1e-3))), dt=300.0, limit=LIMIT)
    zero = np.zeros((nj, ni), F)
    left = 0.0
    planes, deps, S, cur, diag = [zero.copy(), zero.copy()], [zero.copy(), zero.copy()], zero.copy(), 0, np.zeros(4, U32)
    for _ in range(BUDGET_STEPS):
        S, planes[1 - cur], deps[1 - cur], diag = np_route_diffusive(x, planes[cur], planes[1 - cur], S, deps[cur], deps[1 - cur], diag)
        cur = 1 - cur
        left += planes[cur][outlets].astype(F8).sum()
    got = host_drun(x, zero, zero, zero, BUDGET_STEPS, np.zeros(4, U32))
    assert_run(got, (S, planes[cur], deps[cur], diag), "compiled")
    v = (x["runoff_a"].astype(F8) + x["runoff_b"].astype(F8)) * float(F(x["scale"])) * x["area"].astype(F8).ravel()
    total = v.sum() * BUDGET_STEPS
    in_flight = planes[cur][~outlets].astype(F8).sum()                   # released in the last call and not yet gathered
    have = S.astype(F8).sum() + left + in_flight
    r_sum = abs(have - total) / total / EPS
    print("%d x %d, %d calls: input %.6g m3, (storage + in flight + left) - input = %.2f * 2^-24 of it (bound %d); %.1f %% has left; capped %d,"
          " limited %d, blocked %d" % (ni, nj, BUDGET_STEPS, total, r_sum, BUDGET_BOUND, 100 * left / total, int(diag[1]), int(diag[2]), int(diag[3])))
    assert (S >= 0).all() and (planes[cur] >= 0).all(), "the s1 of a call add up to at most the input so far"
    assert r_sum <= BUDGET_BOUND
    assert int(diag[2]) > 0 and int(diag[3]) > 0 and left > 0


# ---------------------------------------------------------------------------------------------------------------- decomposition, column order
def _whole(ni, nj):
    z = tsh.terrain(ni, nj, True)
    ops = diff_operands(ni, nj, "physical")
    d = np_flow_dir(z, DX, DY)
    r = np.random.default_rng(12)
    ops["drop"] = np.where(r.random((nj, ni)) < 0.5, r.uniform(-0.05, 0.1, (nj, ni)), np_flow_drop(d, DX, DY, height=z)).astype(F)
    x = _dblock(d, np_inmask(d), np.arange(ni * nj, dtype=np.int32).reshape(nj, ni), ni * nj, ops)
    return z, ops, x


def _dparts(ni, nj, z, x):
    gcol = np.arange(ni * nj, dtype=np.int32).reshape(nj, ni)
    parts = []
    for tile, blk, dblk, owned in trt._parts(ni, nj, z, 2):
        xp = dict(x, inmask=np_inmask(dblk), dir=dblk, col_index=np.where(owned, gcol[blk], -2).astype(np.int32),
                  **{k: x[k][blk] for k in ("area", "width", "length", "conv", "manning", "drop")})
        parts.append(dict(x=xp, tile=tile, blk=blk, owned=owned))
    return parts


def _cut_run(one, ni, nj, z, ops, x, ncall, refresh_depth):
    """ncall calls on the four parts of the 2 x 2 cut; after every call the ring of out (and of depth) is refreshed from the owners.
    Returns the global storage, out and depth planes and the parts' diag words."""
    parts = _dparts(ni, nj, z, x)
    for p in parts:
        b = p["blk"]
        p.update(S=ops["storage"][b].copy(), out=[ops["out"][b].copy(), ops["out"][b].copy()], h=[ops["depth"][b].copy(), ops["depth"][b].copy()],
                 g=np.zeros(4, U32))
    G, GS, GH, cur = ops["out"].copy(), ops["storage"].copy(), ops["depth"].copy(), 0
    for _ in range(ncall):
        for p in parts:
            p["S"], p["out"][1 - cur], p["h"][1 - cur], p["g"] = one(p["x"], p["out"][cur], p["out"][1 - cur], p["S"], p["h"][cur], p["h"][1 - cur], p["g"])
        cur = 1 - cur
        for p in parts:
            for whole, part in ((G, p["out"][cur]), (GS, p["S"]), (GH, p["h"][cur])):
                whole[p["tile"]] = part[p["owned"]].reshape(whole[p["tile"]].shape)
        for p in parts:
            p["out"][cur] = G[p["blk"]].copy()
            if refresh_depth:
                p["h"][cur] = GH[p["blk"]].copy()
    return GS, G, GH, [p["g"] for p in parts]


def test_decomposition():
    """70 x 130 cut 2 x 2 (directions from margin-2 height windows, the rings of out AND depth refreshed from the owners after every
    call): after 20 calls no word of storage, out and depth differs from the undecomposed run; the maximum of the four diag[0] and the
    sums of the four diag[1..3] are the whole's.  Restated and compiled.  Without the refresh of depth words differ: the ring matters."""
    ni, nj = CUT
    z, ops, x = _whole(ni, nj)
    ws, wo, wh, wg = np_drun(x, ops["storage"], ops["out"], ops["depth"], 20, np.zeros(4, U32))
    for one in (np_route_diffusive, host_one):
        GS, G, GH, gs = _cut_run(one, ni, nj, z, ops, x, 20, True)
        assert trt._differ(GS, ws) + trt._differ(G, wo) + trt._differ(GH, wh) == 0
        assert max(int(g[0]) for g in gs) == int(wg[0])
        assert [sum(int(g[n]) for g in gs) for n in (1, 2, 3)] == [int(wg[n]) for n in (1, 2, 3)] and min(int(v) for v in wg[1:]) > 0
    GS, G, GH, gs = _cut_run(host_one, ni, nj, z, ops, x, 20, False)
    stale = trt._differ(GS, ws) + trt._differ(G, wo)
    print("without the refresh of the ring of depth %d words of storage and out differ" % stale)
    assert stale > 0


def _permuted(x, ops, ni, nj):
    return tc._permuted(x, ops, ni, nj)


@pytest.mark.parametrize("ni, nj", [(65, 5), (67, 35)])
def test_column_order(ni, nj):
    """The same run with a permuted col_index and the runoff planes permuted with it gives the same window planes and diag words."""
    ops = diff_operands(ni, nj, "physical")
    x = _dblock(ops["dir_hills"], np_inmask(ops["dir_hills"]), np.arange(ni * nj, dtype=np.int32).reshape(nj, ni), ni * nj, ops)
    want = np_drun(x, ops["storage"], ops["out"], ops["depth"], 10, np.zeros(4, U32))
    got = host_drun(_permuted(x, ops, ni, nj), ops["storage"], ops["out"], ops["depth"], 10, np.zeros(4, U32))
    assert_run(got, want, "permuted")


def test_diag_accumulates_and_null_diag_changes_nothing():
    """The compiled cell function on the 67 x 35 hills: the words after 5 calls are the maximum and the sums over all five, a second
    batch on top of them only grows them, and without diag storage, out and depth have the same bits."""
    ni, nj = 67, 35
    ops = diff_operands(ni, nj, "physical")
    x = _dblock(ops["dir_hills"], np_inmask(ops["dir_hills"]), np.arange(ni * nj, dtype=np.int32).reshape(nj, ni), ni * nj, ops)
    want = np_drun(x, ops["storage"], ops["out"], ops["depth"], 5, np.zeros(4, U32))
    got = host_drun(x, ops["storage"], ops["out"], ops["depth"], 5, np.zeros(4, U32))
    assert_run(got, want, "with diag")
    first = np_drun(x, ops["storage"], ops["out"], ops["depth"], 1, np.zeros(4, U32))[3]
    assert all(int(want[3][n]) > int(first[n]) > 0 for n in (1, 2, 3)), "the counts are the sums over the calls"
    bare = host_drun(x, ops["storage"], ops["out"], ops["depth"], 5, None)
    assert bare[3] is None
    assert_run(bare[:3] + (want[3],), want, "without diag")
    again = host_drun(x, ops["storage"], ops["out"], ops["depth"], 5, want[3])[3]
    assert again[1:].tolist() == [2 * int(v) for v in want[3][1:]] and int(again[0]) == int(want[3][0])


# ---------------------------------------------------------------------------------------------------------------- the lake's stage
def lake_depth_case(ni, nj):
    """Five lakes on a window: one with area 0, one whose members lie above its surface; the list holds pads (-1, out of range cells
    and lakes) and entries past nmember that name real cells."""
    ncell = ni * nj
    r = np.random.default_rng(40 + ncell)
    nlake = 5
    nlist = min(ncell, 40) + 8
    cells = r.permutation(ncell)[:nlist - 8].astype(np.int32)
    mc = np.concatenate([cells, np.array([-1, ncell, ncell + 7, -2 ** 31, 2 ** 31 - 1, -1, -1, -1], np.int64).astype(np.int32)])
    ml = r.integers(0, nlake, nlist).astype(np.int32)
    ml[nlist - 3:] = (-1, nlake, 2 ** 31 - 1)
    mc[nlist - 3:] = cells[:3] if cells.size >= 3 else 0                  # a real cell with a pad lake
    order = r.permutation(nlist)
    mc, ml = mc[order], ml[order]
    nmember = nlist - 4                                                  # the last four entries lie past the list
    bed = r.uniform(100.0, 104.0, (nj, ni)).astype(F)
    area = np.array([2.5e5, 0.0, 1.0e4, 7.0e5, 3.0e4], F8)
    datum = np.array([100.5, 103.0, 90.0, 101.0, 99.75], F8)
    volume = np.array([int(3.0e5 / Q), int(5.0e5 / Q), int(1.0e4 / Q), 12345678901, 0], I64)      # lake 2: surface at 91 m, below every bed
    depth = r.uniform(0.0, 2.0, (nj, ni)).astype(F)
    return mc, ml, nmember, volume, area, datum, bed, depth


@pytest.mark.parametrize("ni, nj", WINDOWS + [CUT])
def test_host_lake_depth_equals_the_restatement(ni, nj):
    """lake_depth_entry compiled for the host against the float64 restatement in every word of the depth plane; pads and the entries
    past nmember leave their cells alone, a lake with area 0 stands at its datum, a member above the surface gets 0."""
    mc, ml, nmember, volume, area, datum, bed, depth = lake_depth_case(ni, nj)
    want = np_lake_depth(mc, ml, nmember, volume, area, datum, bed, depth, Q)
    assert_same(host_lake_depth(mc, ml, nmember, volume, area, datum, bed, depth, Q), want, "depth")
    valid = (mc[:nmember] >= 0) & (mc[:nmember] < ni * nj) & (ml[:nmember] >= 0) & (ml[:nmember] < 5)
    touched = np.zeros(ni * nj, bool)
    touched[mc[:nmember][valid]] = True
    assert_same(want.reshape(-1)[~touched], depth.reshape(-1)[~touched], "cells that are not listed keep their depth")
    for c, l in zip(mc[:nmember][valid], ml[:nmember][valid]):
        got = want.reshape(-1)[c]
        if l == 1:
            assert got == F(max(103.0 - float(bed.reshape(-1)[c]), 0.0)), "area 0: level 0, the surface is the datum"
        if l == 2:
            assert got.view(U32) == 0, "a member above the surface"


def test_datum_from_fill():
    """datum = min(filled over the members) - mean(filled - raw over the members), float64: a lake that holds area * its mean depth has
    its surface at the spill level."""
    from noahmp_amd.routing import Lakes
    raw = np.array([[5.0, 5.0, 5.0, 5.0, 5.0], [5.0, 2.0, 1.0, 3.5, 5.0], [5.0, 5.0, 5.0, 4.0, 9.0], [9.0, 9.0, 7.0, 9.0, 9.0]])
    filled = np.maximum(raw, 4.0)
    filled[3, 2] = 8.0
    lake_id = np.where(filled - raw >= 0.5, 1, 0).astype(np.int32)
    lake_id[3, 2] = 2
    datum = Lakes.datum_from_fill(raw, filled, lake_id)
    assert datum.dtype == F8 and datum.tolist() == [4.0 - (2.0 + 3.0 + 0.5) / 3.0, 8.0 - 1.0]
    mean_depth = (filled - raw)[lake_id == 1].mean()
    assert datum[0] + mean_depth == 4.0


# ---------------------------------------------------------------------------------------------------------------- refusals and bindings
DROP_PLANES = ("height", "slope", "dir", "drop")
DIF_PLANES = ("inmask", "col_index", "dir", "area", "width", "length", "conv", "manning", "drop", "storage", "out_old", "out_new", "runoff_a",
              "runoff_b", "depth_old", "depth_new", "diag")
DIF_REQUIRED = tuple(k for k in DIF_PLANES if k not in ("runoff_b", "diag"))
LD_PLANES = ("member_cell", "member_lake", "volume", "area", "datum", "bed", "depth")
CALLS = ("noahmp_hip_flow_drop", "noahmp_hip_route_diffusive", "noahmp_hip_lake_depth")
NCELL = 15
DISTINCT_TEXTS = 6 + 10 + 11


def _fd_block(ptrs, **kw):
    b = abi.FlowDrop()
    for k in DROP_PLANES:
        setattr(b, k, ptrs[k])
    b.slope = None
    b.ni, b.nj, b.dx, b.dy = 5, 3, DX, DY
    for k, v in kw.items():
        setattr(b, k, v)
    return b


def _rd_block(ptrs, **kw):
    b = abi.RouteDiffusive()
    for k in DIF_PLANES:
        setattr(b, k, ptrs[k])
    b.scale, b.dt, b.limit, b.ni, b.nj = 0.6, 600.0, LIMIT, 5, 3
    for k, v in kw.items():
        setattr(b, k, v)
    return b


def _ld_block(ptrs, **kw):
    b = abi.LakeDepth()
    for k in LD_PLANES:
        setattr(b, k, ptrs[k])
    b.nmember, b.nlake, b.ncell, b.quantum = 4, 2, NCELL, Q
    for k, v in kw.items():
        setattr(b, k, v)
    return b


def refusal_probes(fp, dp, lp):
    """[(site id, call, block or None, ncol)]: one probe per refusal site and per way into it."""
    out = [("drop.null", CALLS[0], None, None)]
    for f in ("dir", "drop"):
        out.append(("drop.required." + f, CALLS[0], _fd_block(fp, **{f: None}), None))
    out.append(("drop.both", CALLS[0], _fd_block(fp, slope=fp["slope"]), None))
    out.append(("drop.neither", CALLS[0], _fd_block(fp, height=None), None))
    for nm, kw in (("ni", dict(ni=-1)), ("nj", dict(nj=-1)), ("big", dict(ni=65536, nj=32768))):
        out.append(("drop.window." + nm, CALLS[0], _fd_block(fp, **kw), None))
    for nm, kw in (("dx0", dict(dx=0.0)), ("dxnan", dict(dx=float("nan"))), ("dyinf", dict(dy=float("inf"))), ("dyneg", dict(dy=-1.0))):
        out.append(("drop.spacing." + nm, CALLS[0], _fd_block(fp, **kw), None))
    for f in ("height", "dir"):
        out.append(("drop.alias." + f, CALLS[0], _fd_block(fp, drop=fp[f]), None))
    out.append(("drop.alias.slope", CALLS[0], _fd_block(fp, height=None, slope=fp["slope"], drop=fp["slope"] + 8), None))
    out.append(("drop.overlap.height", CALLS[0], _fd_block(fp, drop=fp["height"] + 4 * (NCELL - 1)), None))
    out.append(("diffusive.null", CALLS[1], None, NCELL))
    for f in DIF_REQUIRED:
        out.append(("diffusive.required." + f, CALLS[1], _rd_block(dp, **{f: None}), NCELL))
    out.append(("diffusive.same.out", CALLS[1], _rd_block(dp, out_new=dp["out_old"]), NCELL))
    out.append(("diffusive.same.depth", CALLS[1], _rd_block(dp, depth_new=dp["depth_old"]), NCELL))
    for nm, kw in (("ni", dict(ni=-1)), ("nj", dict(nj=-1)), ("big", dict(ni=65536, nj=32768))):
        out.append(("diffusive.window." + nm, CALLS[1], _rd_block(dp, **kw), NCELL))
    for nm, ncol in (("neg", -1), ("big", 2 ** 31)):
        out.append(("diffusive.ncol." + nm, CALLS[1], _rd_block(dp), ncol))
    for nm, v in (("zero", 0.0), ("neg", -600.0), ("nan", float("nan")), ("inf", float("inf"))):
        out.append(("diffusive.dt." + nm, CALLS[1], _rd_block(dp, dt=v), NCELL))
        out.append(("diffusive.limit." + nm, CALLS[1], _rd_block(dp, limit=v if nm != "neg" else -0.5), NCELL))
    for f in ("storage", "out_old", "out_new"):
        out.append(("diffusive.depth_new." + f, CALLS[1], _rd_block(dp, depth_new=dp[f]), NCELL))
    out.append(("diffusive.depth_new.overlap.depth_old", CALLS[1], _rd_block(dp, depth_new=dp["depth_old"] + 4 * (NCELL - 1)), NCELL))
    out.append(("diffusive.depth_new.overlap.storage", CALLS[1], _rd_block(dp, depth_new=dp["storage"] - 4 * (NCELL - 1)), NCELL))
    for off in (1, 2, 3):
        out.append(("diffusive.diag.misaligned.%d" % off, CALLS[1], _rd_block(dp, diag=dp["diag"] + off), NCELL))
    out.append(("lake_depth.null", CALLS[2], None, None))
    for nm, v in (("neg", -1), ("big", 2 ** 31)):
        out.append(("lake_depth.nmember." + nm, CALLS[2], _ld_block(lp, nmember=v), None))
        out.append(("lake_depth.ncell." + nm, CALLS[2], _ld_block(lp, ncell=v), None))
    out.append(("lake_depth.nlake.neg", CALLS[2], _ld_block(lp, nlake=-1), None))
    for f in LD_PLANES:
        out.append(("lake_depth.required." + f, CALLS[2], _ld_block(lp, **{f: None}), None))
    for nm, v in tl.BAD_QUANTA:
        out.append(("lake_depth.quantum." + nm, CALLS[2], _ld_block(lp, quantum=v), None))
    for f in ("volume", "area", "datum"):
        out.append(("lake_depth.misaligned." + f, CALLS[2], _ld_block(lp, **{f: lp[f] + 4}), None))
    for f in ("bed", "depth"):
        out.append(("lake_depth.misaligned." + f, CALLS[2], _ld_block(lp, **{f: lp[f] + 2}), None))
    for f in ("member_cell", "member_lake", "bed", "volume", "area", "datum"):
        out.append(("lake_depth.alias." + f, CALLS[2], _ld_block(lp, depth=lp[f]), None))
    out.append(("lake_depth.overlap.bed", CALLS[2], _ld_block(lp, depth=lp["bed"] + 4 * (NCELL - 1)), None))
    return out


def _call(lib, fn, block, ncol):
    ref = C.byref(block) if block is not None else None
    return getattr(lib, fn)(ref, None) if ncol is None else getattr(lib, fn)(ref, ncol, None)


def _refusals(lib, fp, dp, lp):
    """Every refusal: -105 and the full text of the fixture."""
    want = json.load(open(REFUSAL_FIXTURE))
    probes = refusal_probes(fp, dp, lp)
    assert sorted(want) == sorted(p[0] for p in probes)
    for site, fn, block, ncol in probes:
        rc = _call(lib, fn, block, ncol)
        assert [rc, lib.noahmp_hip_last_error().decode()] == want[site], site
        assert rc == -105 and want[site][1].startswith(fn + ": "), site


def test_refusals_write_nothing():
    """Every refusal site of the three calls gives -105 and its full text (tests/golden/diffusive_refusal_text.json) before anything
    is launched or read: the planes here are host memory that the calls must not touch, and they keep their poison."""
    lib = abi.load_library()
    pools = [{k: np.full(32, POISON, F) for k in names} for names in (DROP_PLANES, DIF_PLANES, LD_PLANES)]
    _refusals(lib, *({k: v.ctypes.data for k, v in pl.items()} for pl in pools))
    assert all((p == POISON).all() for pl in pools for p in pl.values())
    text = json.load(open(REFUSAL_FIXTURE))
    for site, word in (("drop.both", "exactly one"), ("drop.neither", "exactly one"), ("drop.spacing.dx0", "dx"), ("drop.window.big", "ni*nj"),
                       ("drop.alias.dir", "share"), ("drop.required.drop", "required"), ("diffusive.required.manning", "required"),
                       ("diffusive.required.depth_new", "required"), ("diffusive.same.out", "different"), ("diffusive.same.depth", "depth_old and depth_new"),
                       ("diffusive.ncol.big", "ncol"), ("diffusive.dt.nan", "dt"), ("diffusive.limit.nan", "limit"), ("diffusive.limit.zero", "limit"),
                       ("diffusive.depth_new.out_new", "depth_new"), ("diffusive.depth_new.overlap.depth_old", "share"),
                       ("diffusive.diag.misaligned.2", "aligned"), ("lake_depth.quantum.three", "power of two"), ("lake_depth.required.datum", "datum"),
                       ("lake_depth.required.bed", "bed"), ("lake_depth.misaligned.area", "8 bytes"), ("lake_depth.misaligned.depth", "4 bytes"),
                       ("lake_depth.alias.bed", "share"), ("lake_depth.nmember.big", "nmember"), ("lake_depth.ncell.neg", "ncell")):
        assert word in text[site][1], site
    assert len({tuple(v) for v in text.values()}) == DISTINCT_TEXTS


HEADER_LINES = (
    "#define NOAHMP_HIP_HAS_ROUTE_DIFFUSIVE 1\n", "#define NOAHMP_HIP_ABI_MINOR 3\n", "typedef struct noahmp_flow_drop {", "} noahmp_flow_drop;",
    "typedef struct noahmp_route_diffusive {", "} noahmp_route_diffusive;", "typedef struct noahmp_lake_depth {", "} noahmp_lake_depth;",
    "int    noahmp_hip_flow_drop(const noahmp_flow_drop* fd, void* stream);",
    "int    noahmp_hip_route_diffusive(const noahmp_route_diffusive* r, int64_t ncol, void* stream);",
    "int    noahmp_hip_lake_depth(const noahmp_lake_depth* t, void* stream);",
    "hd = depth_old[dn];  dd = h - hd;  dh = drop[c] + dd", "open = dh > 0", "sf = dh/length[c];  r = sqrtf(sf);  cvd = r/manning[c]",
    "half = limit*dh;  lim = half*wl", "else { open = true;  cvd = conv[c] }",
    "a = width[c]*h;  h2 = h + h;  p = width[c] + h2;  R = a/p;  r23 = powf(R, 0x1.555556p-1f)", "vel = cvd*r23;  qa = vel*a;  od = qa*dt",
    "capped = !(od < s1);  o = capped ? s1 : od", "limited = has && lim < o;  o = limited ? lim : o", "vd = vel*dt;  cr = vd/length[c]",
    "s2 = s1 - o;  storage[c] = s2;  out_new[c] = o", "h1 = s2/wl;  depth_new[c] = (s2 > 0) ? h1 : 0",
    "NOT a difference of two stage planes", "NOW REPRESENTED", "THE RING-1 RULE", "Hunter et al. 2005", "The call never zeroes them",
    "vol = (double)volume[l]*q;  h = (area[l] > 0) ? vol/area[l] : 0", "e = datum[l] + h", "d = e - (double)bed[c]", "depth[c] = (d > 0) ? (float)d : 0",
    # the three lines of the earlier blocks that name this as missing stay as they are
    "NOT represented: kinematic or diffusive wave, channel geometry, backwater, losses and lakes",
    "NOT represented: diffusive wave and backwater, trapezoidal sections, losses, an implicit solve.", "backwater into inflowing channels.",
)


def test_bindings_carry_the_diffusive_calls():
    from tools import gen_abi
    for rel, text in (("include/noahmp_hip.h", gen_abi.c_header()), ("noahmp_amd/fortran/module_sf_noahmpdrv_hip.F90", gen_abi.fortran_shim())):
        assert open(os.path.join(ROOT, rel)).read() == text, rel
    hdr = open(HEADER).read()
    for word in HEADER_LINES:
        assert word in hdr, word
    assert "\n".join(gen_abi.diffusive_header()) in hdr
    assert "noahmp_route_diffusive" not in gen_abi.ref_harness() and "noahmp_route_diffusive" not in gen_abi.shim_wrap()
    f90 = open(os.path.join(ROOT, "noahmp_amd", "fortran", "module_sf_noahmpdrv_hip.F90")).read()
    for word in tuple("bind(C, name='%s')" % c for c in CALLS) + ("type, bind(C) :: noahmp_flow_drop ", "type, bind(C) :: noahmp_route_diffusive ",
                                                                  "type, bind(C) :: noahmp_lake_depth "):
        assert word in f90, word
    for sym in CALLS:
        assert sym in abi.EXPORTED_SYMBOLS
    assert [n for n, _ in abi.FlowDrop._fields_] == list(DROP_PLANES) + ["ni", "nj", "dx", "dy"]
    assert [n for n, _ in abi.RouteDiffusive._fields_] == list(DIF_PLANES) + ["scale", "dt", "limit", "ni", "nj"]
    assert [n for n, _ in abi.LakeDepth._fields_] == ["member_cell", "member_lake", "nmember", "volume", "area", "datum", "bed", "depth", "nlake",
                                                     "ncell", "quantum"]
    kin = {n for n, _ in abi.RouteKinematic._fields_}
    assert kin - {"depth"} <= {n for n, _ in abi.RouteDiffusive._fields_} and "depth" not in {n for n, _ in abi.RouteDiffusive._fields_}


def test_ctypes_mirrors_match_the_compiled_header(tmp_path):
    body, want = "", []
    for cname, cls in (("noahmp_flow_drop", abi.FlowDrop), ("noahmp_route_diffusive", abi.RouteDiffusive), ("noahmp_lake_depth", abi.LakeDepth)):
        names = [n for n, _ in cls._fields_]
        body += 'printf(" %%zu", sizeof(%s));' % cname + "".join('printf(" %%zu", offsetof(%s, %s));' % (cname, n) for n in names)
        want += [C.sizeof(cls)] + [getattr(cls, n).offset for n in names]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "noahmp_hip.h"\nint main(){' + body +
                   'printf(" %d %d", NOAHMP_HIP_ABI_MINOR, NOAHMP_HIP_HAS_ROUTE_DIFFUSIVE); return 0;}')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(v) for v in subprocess.check_output([str(exe)]).split()] == want + [3, 1]


def test_library_exports_the_diffusive_calls():
    if not os.path.exists(abi.LIB_PATH):
        from noahmp_amd import build as b
        b.build()
    build_variant()
    for path in (abi.LIB_PATH, LIB_OTHER):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        for sym in CALLS:
            assert " T %s\n" % sym in out, (path, sym)


@pytest.mark.skipif(tr._flang() is None, reason="no flang")
def test_generated_fortran_types_and_interfaces_compile(tmp_path):
    """The diffusive part of the generated module compiles, and a caller of the three interfaces type-checks."""
    from tools import gen_abi
    text = "\n".join(["module diffusive_abi_check", "  use iso_c_binding", "  implicit none"] + gen_abi.diffusive_f90_types() + ["  interface"] +
                     gen_abi.diffusive_f90_interfaces() +
                     ["  end interface", "contains", "  function go(planes, ncol) result(rc)", "    type(c_ptr), intent(in) :: planes(20)",
                      "    integer(c_int64_t), value :: ncol", "    type(noahmp_flow_drop) :: fd", "    type(noahmp_route_diffusive) :: r",
                      "    type(noahmp_lake_depth) :: t", "    integer(c_int) :: rc",
                      "    fd%height = planes(1); fd%slope = c_null_ptr; fd%dir = planes(2); fd%drop = planes(3)",
                      "    fd%ni = 64; fd%nj = 8; fd%dx = 1000.0; fd%dy = 1000.0",
                      "    rc = noahmp_hip_flow_drop(fd, c_null_ptr)",
                      "    r%inmask = planes(4); r%col_index = planes(5); r%dir = planes(2); r%area = planes(6); r%width = planes(7)",
                      "    r%length = planes(8); r%conv = planes(9); r%manning = planes(10); r%drop = planes(3); r%storage = planes(11)",
                      "    r%out_old = planes(12); r%out_new = planes(13); r%runoff_a = planes(14); r%runoff_b = c_null_ptr",
                      "    r%depth_old = planes(15); r%depth_new = planes(16); r%diag = c_null_ptr",
                      "    r%scale = 0.6; r%dt = 600.0; r%limit = 0.5; r%ni = 64; r%nj = 8",
                      "    rc = noahmp_hip_route_diffusive(r, ncol, c_null_ptr)",
                      "    t%member_cell = planes(17); t%member_lake = planes(18); t%nmember = 128_c_int64_t; t%volume = planes(19)",
                      "    t%area = planes(20); t%datum = planes(20); t%bed = planes(1); t%depth = planes(16)",
                      "    t%nlake = 2; t%ncell = 512_c_int64_t; t%quantum = 2.0d0**(-10)",
                      "    rc = noahmp_hip_lake_depth(t, c_null_ptr)",
                      "  end function go", "end module diffusive_abi_check", ""])
    f = tmp_path / "diffusive_abi_check.f90"
    f.write_text(text)
    subprocess.check_call([tr._flang(), "-c", str(f), "-o", str(tmp_path / "diffusive_abi_check.o"), "-J", str(tmp_path)], cwd=str(tmp_path))


def test_sub_steps_default_is_unchanged():
    """FlowNetwork._sub_steps without `also` hands exchange_halo the one out plane, as before; with it the named planes travel in the
    same call, after out."""
    import types
    from noahmp_amd.routing import FlowNetwork
    seen = []
    comm = types.SimpleNamespace(exchange_halo=lambda planes, geom: seen.append(list(planes)))
    sync = types.SimpleNamespace(synchronize=lambda: None)
    fake = types.SimpleNamespace(out=["out0", "out1"], cur=0, after_launch=[], engine=types.SimpleNamespace(stream_sync=lambda s: None),
                                 torch=types.SimpleNamespace(cuda=types.SimpleNamespace(current_stream=lambda: sync)), last_dt=None)
    FlowNetwork._sub_steps(fake, lambda a, b: None, 600.0, 2, comm, "geom", None)
    assert seen == [["out1"], ["out0"]] and fake.last_dt == 300.0
    seen.clear()
    FlowNetwork._sub_steps(fake, lambda a, b: None, 600.0, 2, comm, "geom", None, also=lambda new: ["depth%d" % new])
    assert seen == [["out1", "depth1"], ["out0", "depth0"]]


# ---------------------------------------------------------------------------------------------------------------- GPU
_dev = tr._dev
_pool, _guards_ok = trt._pool, trt._guards_ok


@pytest.fixture(scope="module")
def engine_other(tables):
    """The variant library: noahmp_hip_route_diffusive with the other form of the downstream-depth access."""
    from noahmp_amd.driver import Engine
    build_variant()                                                      # nothing to do where __graft_entry__.build() has run
    if not os.path.exists(LIB_OTHER):
        pytest.fail("%s missing: __graft_entry__.build() compiles it" % LIB_OTHER)
    return Engine(tables[0], lib_path=LIB_OTHER)


@pytest.mark.gpu
@pytest.mark.parametrize("ni, nj", WINDOWS + [CUT])
def test_gpu_flow_drop_equals_the_restatement(engine, ni, nj):
    """noahmp_hip_flow_drop against np_flow_drop in every word, the cases of the host test; the destination sits at an odd offset
    inside a poisoned pool whose guard words keep the poison.  An empty window writes nothing."""
    import torch
    ncell = ni * nj
    pool, (dd,) = _pool(ncell, 1, torch.float32, POISON)
    dd = dd.view(nj, ni)
    for name, d, n, dx, dy, z, s in tc.geom_cases(ni, nj):
        pool.fill_(POISON)
        torch.cuda.synchronize()
        engine.flow_drop(engine.flow_drop_block(_dev(d), dd, dx, dy, height=_dev(z) if z is not None else None,
                                                slope=_dev(s) if s is not None else None))
        engine.stream_sync()
        assert_same(dd.cpu().numpy(), np_flow_drop(d, dx, dy, height=z, slope=s), "%dx%d %s: drop" % (ni, nj, name))
        assert _guards_ok(pool, ncell, POISON), name
    pool.fill_(POISON)
    torch.cuda.synchronize()
    name, d, n, dx, dy, z, s = tc.geom_cases(ni, nj)[0]
    b = engine.flow_drop_block(_dev(d), dd, dx, dy, height=_dev(z))
    b.nj = 0
    engine.flow_drop(b)
    engine.stream_sync()
    assert (pool.cpu().numpy() == POISON).all()


def _gpu_drun(eng, x, storage, out, depth, nstep, diag0):
    """nstep calls of noahmp_hip_route_diffusive on planes at odd offsets inside poisoned pools: ((storage, out, depth, diag), guards)."""
    import torch
    nj, ni = x["inmask"].shape
    ncell = ni * nj
    pool, (sd, o0, o1, h0, h1) = _pool(ncell, 5, torch.float32, POISON)
    sd, o0, o1, h0, h1 = (t.view(nj, ni) for t in (sd, o0, o1, h0, h1))
    sd.copy_(_dev(storage))
    for t in (o0, o1):
        t.copy_(_dev(out))
    for t in (h0, h1):
        t.copy_(_dev(depth))
    gpool = torch.full((10,), 77, dtype=torch.int32, device="cuda")
    diag = None
    if diag0 is not None:
        diag = gpool[3:7]
        diag.copy_(_dev(np.asarray(diag0, U32).view(np.int32)))
    ra = _dev(x["runoff_a"])
    rb = _dev(x["runoff_b"]) if x.get("runoff_b") is not None else None
    m, col, dirp, area, width, length, conv, manning, drop = (_dev(x[k]) for k in ("inmask", "col_index", "dir", "area", "width", "length", "conv",
                                                                                   "manning", "drop"))
    torch.cuda.synchronize()
    planes, deps, cur = [o0, o1], [h0, h1], 0
    for _ in range(nstep):
        eng.route_diffusive(eng.route_diffusive_block(m, col, dirp, area, width, length, conv, manning, drop, sd, planes[cur], planes[1 - cur], ra, rb,
                                                      deps[cur], deps[1 - cur], x["scale"], x["dt"], limit=x["limit"], diag=diag), x["ncol"])
        cur = 1 - cur
    eng.stream_sync()
    g = gpool.cpu().numpy()
    ok = _guards_ok(pool, ncell, POISON) and (g[:3] == 77).all() and (g[7:] == 77).all() and (diag is not None or (g == 77).all())
    return (sd.cpu().numpy(), planes[cur].cpu().numpy(), deps[cur].cpu().numpy(), g[3:7].view(U32).copy() if diag is not None else None), ok


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["default", "other"])
@pytest.mark.parametrize("ni, nj", WINDOWS + [CUT])
def test_gpu_route_diffusive_equals_the_restatement(engine, engine_other, form, ni, nj):
    """noahmp_hip_route_diffusive, in the library's form of the downstream-depth access and in the variant library's, against
    np_route_diffusive in every word of storage, out, depth and the four diag words after 1, 2 and 25 calls: the cases of the host test
    (diag starts at [3, 5, 7, 11]: the call accumulates and never zeroes; without diag nothing else is written); guard words keep the
    poison.  (65, 5) and (67, 35): the last workgroup is partly past ncell; (1, 1): one live lane.  An empty window writes nothing."""
    import torch
    eng = engine if form == "default" else engine_other
    for what, x, storage, out, depth, wg, nstep, want in diff_cases(ni, nj):
        got, ok = _gpu_drun(eng, x, storage, out, depth, nstep, np.array(DIAG0, U32) if wg else None)
        assert_run(got, want, what)
        assert ok, what + ": guard words"
    what, x, storage, out, depth, wg, nstep, want = diff_cases(ni, nj)[0]
    pool, (sd, o0, o1, h0, h1) = _pool(ni * nj, 5, torch.float32, POISON)
    diag = torch.full((4,), 77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    b = eng.route_diffusive_block(*(_dev(x[k]) for k in ("inmask", "col_index", "dir", "area", "width", "length", "conv", "manning", "drop")),
                                  sd.view(nj, ni), o0.view(nj, ni), o1.view(nj, ni), _dev(x["runoff_a"]), None, h0.view(nj, ni), h1.view(nj, ni), SCALE,
                                  DT, diag=diag)
    b.nj = 0
    eng.route_diffusive(b, ni * nj)
    eng.stream_sync()
    assert (pool.cpu().numpy() == POISON).all() and (diag.cpu().numpy() == 77).all()


@pytest.mark.gpu
def test_gpu_diag_accumulates_and_null_diag_changes_nothing(engine):
    """Two runs of 5 calls on the 67 x 35 hills: with diag the words after 5 calls are the maximum and the sums over all five; a second
    batch on top of them only grows them; without diag storage, out and depth have the same bits."""
    ni, nj = 67, 35
    ops = diff_operands(ni, nj, "physical")
    x = _dblock(ops["dir_hills"], np_inmask(ops["dir_hills"]), np.arange(ni * nj, dtype=np.int32).reshape(nj, ni), ni * nj, ops)
    want = np_drun(x, ops["storage"], ops["out"], ops["depth"], 5, np.zeros(4, U32))
    got, ok = _gpu_drun(engine, x, ops["storage"], ops["out"], ops["depth"], 5, np.zeros(4, U32))
    assert_run(got, want, "with diag")
    assert ok
    bare, ok = _gpu_drun(engine, x, ops["storage"], ops["out"], ops["depth"], 5, None)
    assert ok and bare[3] is None
    assert_run(bare[:3] + (want[3],), want, "without diag")
    again, ok = _gpu_drun(engine, x, ops["storage"], ops["out"], ops["depth"], 5, want[3])
    assert again[3][1:].tolist() == [2 * int(v) for v in want[3][1:]] and int(again[3][0]) == int(want[3][0])


@pytest.mark.gpu
@pytest.mark.parametrize("ni, nj", [(65, 5), (67, 35)])
def test_gpu_column_order(engine, ni, nj):
    """A sorted store followed through col_index: the planes and the diag words are those of the unsorted run."""
    ops = diff_operands(ni, nj, "physical")
    x = _dblock(ops["dir_hills"], np_inmask(ops["dir_hills"]), np.arange(ni * nj, dtype=np.int32).reshape(nj, ni), ni * nj, ops)
    want = np_drun(x, ops["storage"], ops["out"], ops["depth"], 10, np.zeros(4, U32))
    for xx, nm in ((x, "identity"), (_permuted(x, ops, ni, nj), "permuted")):
        got, ok = _gpu_drun(engine, xx, ops["storage"], ops["out"], ops["depth"], 10, np.zeros(4, U32))
        assert_run(got, want, nm)
        assert ok


@pytest.mark.gpu
@pytest.mark.parametrize("ni, nj", WINDOWS + [CUT])
def test_gpu_lake_depth_equals_the_restatement(engine, ni, nj):
    """noahmp_hip_lake_depth against the float64 restatement in every word of the depth plane, which sits inside a poisoned pool whose
    guard words keep the poison; the list is longer than nmember.  nmember = 0 writes nothing."""
    import torch
    mc, ml, nmember, volume, area, datum, bed, depth = lake_depth_case(ni, nj)
    pool, (dd,) = _pool(ni * nj, 1, torch.float32, POISON)
    dd = dd.view(nj, ni)
    dd.copy_(_dev(depth))
    torch.cuda.synchronize()
    keep = (_dev(mc), _dev(ml), _dev(volume), _dev(area), _dev(datum), _dev(bed))
    b = engine.lake_depth_block(*keep, dd, Q)
    b.nmember = nmember
    engine.lake_depth(b)
    engine.stream_sync()
    assert_same(dd.cpu().numpy(), np_lake_depth(mc, ml, nmember, volume, area, datum, bed, depth, Q), "depth")
    assert _guards_ok(pool, ni * nj, POISON)
    dd.copy_(_dev(depth))
    torch.cuda.synchronize()
    b.nmember = 0
    engine.lake_depth(b)
    engine.stream_sync()
    assert_same(dd.cpu().numpy(), depth, "nmember = 0")


class _RingsFromOwners:
    """A stand-in for Comm in one process: exchange_halo copies the rings of out and depth from the whole-domain planes of the same call
    (the restatement's), enqueued only on torch's current stream."""

    def __init__(self, whole, blk, ring):
        self.whole, self.blk, self.ring, self.calls = whole, blk, ring, 0

    def exchange_halo(self, planes, geom):
        import torch
        assert len(planes) == 2 and geom == "geom", "out and the new depth plane travel in one call"
        for plane, w in zip(planes, self.whole[self.calls]):
            plane.copy_(torch.where(self.ring, w[self.blk], plane))
        self.calls += 1


@pytest.mark.gpu
def test_gpu_decomposition(engine):
    """DiffusiveFlow.step(comm=..., nsub=2) on the four parts of 70 x 130 (set_terrain on margin-2 windows, set_geometry with the
    height window cut to the block), ten steps = 20 calls, the rings of out and depth refreshed after every call in ONE exchange:
    storage, out and depth have 0 differing words against the whole-domain restatement; the maximum of the four diag[0] and the sums
    of the four diag[1..3] are the whole's."""
    import types
    import torch
    from noahmp_amd.routing import DiffusiveFlow, FlowNetwork
    ni, nj = CUT
    nstep, nsub, dt = 10, 2, 2 * DT
    z = tsh.terrain(ni, nj, True)
    ops = diff_operands(ni, nj, "physical")
    d = np_flow_dir(z, DX, DY)
    n = np.random.default_rng(8).uniform(0.03, 0.08, (nj, ni)).astype(F)
    length, conv, _ = np_flow_channel(d, n, DX, DY, SMIN, height=z)
    ncell = ni * nj
    ops = dict(ops, manning=n, drop=np_flow_drop(d, DX, DY, height=z), length=length, conv=conv)
    x = dict(_dblock(d, np_inmask(d), np.arange(ncell, dtype=np.int32).reshape(nj, ni), ncell, ops), scale=float(F(dt) * F(1e-3)) / nsub, dt=dt / nsub)
    S, planes, deps, cur, whole, G = ops["storage"].copy(), [ops["out"].copy(), ops["out"].copy()], [ops["depth"].copy(), ops["depth"].copy()], 0, [], np.zeros(4, U32)
    for _ in range(nstep * nsub):
        S, planes[1 - cur], deps[1 - cur], G = np_route_diffusive(x, planes[cur], planes[1 - cur], S, deps[cur], deps[1 - cur], G)
        cur = 1 - cur
        whole.append((_dev(planes[cur]), _dev(deps[cur])))
    torch.cuda.synchronize()
    words, differ = [], 0
    for (tile, win, idx), (_, blk, bidx) in zip(tsh._cuts(ni, nj, 2), tsh._cuts(ni, nj, 1)):
        tj, ti = tile
        net = FlowNetwork(engine, ti.stop - ti.start, tj.stop - tj.start)
        net.set_terrain(_dev(z[win]), DX, DY, origin=(ti.start - win[1].start, tj.start - win[0].start))
        net.set_area(_dev(ops["area"][blk]))
        net.set_input_columns(None)
        net.storage.copy_(_dev(ops["storage"][blk]))
        for o in net.out:
            o.copy_(_dev(ops["out"][blk]))
        df = DiffusiveFlow(net)
        df.set_geometry(_dev(ops["width"][blk]), _dev(n[blk]), smin=SMIN, height=_dev(z[win]))
        for h in df._d:
            h.copy_(_dev(ops["depth"][blk]))
        own = bidx >= 0
        assert_same(df.drop.cpu().numpy()[own], ops["drop"][blk][own], "part %s: drop on the tile" % (tile,))
        store = types.SimpleNamespace(ni=net.ni, nj=net.nj, a=dict(runsfxy=_dev(ops["runoff_a"].reshape(nj, ni)[tile]),
                                                                   runsbxy=_dev(ops["runoff_b"].reshape(nj, ni)[tile])))
        comm = _RingsFromOwners(whole, blk, _dev(~own))
        torch.cuda.synchronize()
        for _ in range(nstep):
            df.step(store, dt, nsub=nsub, comm=comm, geom="geom")
        engine.stream_sync()
        torch.cuda.synchronize()
        assert comm.calls == nstep * nsub and net.last_dt == dt / nsub
        differ += trt._differ(net.tile_view(net.storage).cpu().numpy(), S[tile]) + trt._differ(net.out[net.cur].cpu().numpy(), planes[cur][blk])
        differ += trt._differ(df.depth().cpu().numpy(), deps[cur][blk])
        w = df.diag.cpu().numpy().view(U32)
        words.append(w.copy())
        assert (df.capped(), df.limited(), df.blocked()) == tuple(int(v) for v in w[1:])
        assert df.courant() == 5.0 / 3.0 * float(w[:1].view(F)[0])
    assert differ == 0
    assert max(int(w[0]) for w in words) == int(G[0]) and [sum(int(w[k]) for w in words) for k in (1, 2, 3)] == [int(v) for v in G[1:]]


@pytest.mark.gpu
def test_gpu_refusals_launch_nothing(engine):
    """The refusals with device planes: -105, the full texts of the fixture, and every plane keeps its poison."""
    import torch
    names = (DROP_PLANES, DIF_PLANES, LD_PLANES)
    fl = torch.full((sum(len(n) for n in names), 32), POISON, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ptrs, row = [], 0
    for group in names:
        ptrs.append({k: fl[row + n].data_ptr() for n, k in enumerate(group)})
        row += len(group)
    _refusals(engine.lib, *ptrs)
    engine.stream_sync()
    torch.cuda.synchronize()
    assert (fl.cpu().numpy() == POISON).all()


def _diffusive_engine_run(engine, tables, height, sort, restart_after=None):
    """Three engine steps of the 35 x 67 mixed tile at a rainy hour, each followed by DiffusiveFlow.step(nsub=2).  restart_after = n:
    after n steps the state_dict goes into a NEW network and flow, which make the remaining steps."""
    import torch
    from noahmp_amd import synth
    from noahmp_amd.routing import DiffusiveFlow, FlowNetwork
    T, tb = tables
    s = synth.mixed_small(tb, ni=trt.ENG_NI, nj=trt.ENG_NJ)
    lake = np.random.default_rng(11).random((trt.ENG_NJ, trt.ENG_NI)) < 0.06
    s.a["ivgtyp"][lake] = s.cfg.iswater
    s.a["xland"][lake] = 2.0
    synth.first_step_fixups(s)
    synth.diurnal_forcing(s, 11, t_offset=s.t_offset)
    d = s.to_device("cuda:0")
    torch.cuda.synchronize()

    def make():
        net = FlowNetwork(engine, trt.ENG_NI, trt.ENG_NJ)
        net.set_terrain(_dev(height), DX, DX, origin=(trt.ENG_MARGIN, 0))
        df = DiffusiveFlow(net)
        df.set_geometry(20.0, 0.05, height=_dev(height))
        return net, df

    net, df = make()
    perm = None
    if sort:
        engine.sort_store(d)
        perm = d.sort_perm.cpu().numpy()
        df.follow(d)
    seen = []
    for it in range(1, trt.ENG_STEPS + 1):
        st = engine.noahmplsm(d, it, 2000, 180.0)
        assert st.code == 0
        df.step(d, d.cfg.dt, nsub=2)
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
        if restart_after == it:
            state = df.state_dict()
            assert sorted(state) == ["depth", "out", "storage"]
            has_input = net.has_input
            net, df = make()
            net.set_input_columns(has_input)
            if sort:
                df.follow(d)
            df.load_state_dict(state)
    return d, net, df, seen


@pytest.mark.gpu
def test_gpu_engine_run_in_a_valley(engine, tables):
    """Three noahmplsm steps of a 35 x 67 mixed tile in the valley terrain, each followed by DiffusiveFlow.step(nsub=2): storage, out,
    depth and diag equal the restatement driven by the store's own runoff planes; the sorted store gives identical planes; a run whose
    state_dict is loaded into a new network and flow after the second step ends with the bits of the uninterrupted run; discharge()
    works as with FlowNetwork.step; courant() is finite."""
    height = tsv._valley()
    d, net, df, seen = _diffusive_engine_run(engine, tables, height, False)
    dt = d.cfg.dt
    blk = (slice(None), slice(trt.ENG_MARGIN - 1, trt.ENG_MARGIN + trt.ENG_NI + 1))
    dirp = net.dir.cpu().numpy()
    manning = np.full(net.block_shape, 0.05, F)
    x = dict(inmask=net.inmask.cpu().numpy(), col_index=net.col_index.cpu().numpy(), ncol=trt.ENG_NI * trt.ENG_NJ, dir=dirp, area=net.area.cpu().numpy(),
             width=df.width.cpu().numpy(), length=df.length.cpu().numpy(), conv=df.conv.cpu().numpy(), manning=manning,
             drop=np_flow_drop(dirp, DX, DX, height=height[blk]), scale=float(F(dt) * F(1e-3)) / 2, dt=dt / 2, limit=LIMIT)
    assert_same(df.drop.cpu().numpy(), x["drop"], "drop")
    assert_same(df.manning.cpu().numpy(), manning, "manning")
    S = np.zeros(net.block_shape, F)
    planes, deps, cur, G = [S.copy(), S.copy()], [S.copy(), S.copy()], 0, np.zeros(4, U32)
    for ra, rb in seen:
        x["runoff_a"], x["runoff_b"] = ra, rb
        for _ in range(2):
            S, planes[1 - cur], deps[1 - cur], G = np_route_diffusive(x, planes[cur], planes[1 - cur], S, deps[cur], deps[1 - cur], G)
            cur = 1 - cur
    want = (S, planes[cur], deps[cur], G)
    got = (net.storage.cpu().numpy(), net.out[net.cur].cpu().numpy(), df.depth().cpu().numpy(), df.diag.cpu().numpy().view(U32))
    assert_run(got, want, "valley run")
    assert (planes[cur] > 0).any() and (deps[cur] > 0).any() and net.last_dt == dt / 2
    courant = df.courant()
    assert np.isfinite(courant) and courant == 5.0 / 3.0 * float(G[:1].view(F)[0]) and courant > 0
    assert (df.capped(), df.limited(), df.blocked()) == tuple(int(v) for v in G[1:])
    q, q64 = net.discharge().cpu().numpy().astype(F8), planes[cur].astype(F8) / (dt / 2)
    assert (np.abs(q - q64) <= 3 * EPS * np.abs(q64)).all() and (q64 > 0).any()
    ds, nets, dfs, _ = _diffusive_engine_run(engine, tables, height, True)
    assert (ds.sort_perm.cpu().numpy() != np.arange(trt.ENG_NI * trt.ENG_NJ)).any()
    got_s = (nets.storage.cpu().numpy(), nets.out[nets.cur].cpu().numpy(), dfs.depth().cpu().numpy(), dfs.diag.cpu().numpy().view(U32))
    assert_run(got_s, want, "sorted valley run")
    dr, netr, dfr, _ = _diffusive_engine_run(engine, tables, height, False, restart_after=2)
    assert netr is not net
    got_r = (netr.storage.cpu().numpy(), netr.out[netr.cur].cpu().numpy(), dfr.depth().cpu().numpy(), None)
    assert_run(got_r, want[:3] + (None,), "the restart round trip")


BW_N, BW_LAKE, BW_DT, BW_CALLS = 8, 5, 60.0, 400


def _backwater_row():
    """1 x 8, 0.5 m drop per cell, 10 m x 1 km sections; cell 5 is a one-cell lake of 1e4 m2 that never releases (its crest is out of
    reach); steady input of 1 m3/s into cell 3."""
    bed = 0.5 * (BW_N - 1 - np.arange(BW_N))
    runoff = np.zeros(BW_N, F)
    runoff[3] = 1.0 / (ROW_W * ROW_L) * 1e3
    x = row_block(bed, BW_DT, runoff)
    par = tl.lake_params(1, area=ROW_W * ROW_L, weir_h=tl.NEVER, weir_l=1.0)
    par = {k: np.asarray(par[k], F8) for k in tl.PARAMS}
    par["orifice_h"][:] = tl.NEVER
    return np.asarray(bed, F).reshape(1, BW_N), x, par


@functools.lru_cache(maxsize=None)
def _backwater_restated():
    """The run of test_gpu_lake_backwater_through_lakes restated: np_route_diffusive, then test_lakes' take and release, then
    np_lake_depth, per call; asserts what the issue asks of the cell upstream of the lake."""
    bed, x, par = _backwater_row()
    up = BW_LAKE - 1
    datum = float(bed[0, BW_LAKE])
    vol0 = 1.75 * ROW_W * ROW_L
    lake_id = np.zeros((1, BW_N), np.int32)
    lake_id[0, BW_LAKE] = 1
    mc, ml = np.array([BW_LAKE], np.int32), np.array([0], np.int32)
    xr = dict(x, conv=np.where(lake_id > 0, F(0.0), x["conv"]).astype(F), runoff_b=np.zeros(BW_N, F))
    zero = np.zeros((1, BW_N), F)
    S, planes, deps, cur = zero.copy(), [zero.copy(), zero.copy()], [zero.copy(), zero.copy()], 0
    vol, inf = np.array([int(np.floor(vol0 / Q))], I64), np.zeros(1, I64)
    G, left, record = np.zeros(4, U32), [], []
    for _ in range(BW_CALLS):
        S, planes[1 - cur], deps[1 - cur], G = np_route_diffusive(xr, planes[cur], planes[1 - cur], S, deps[cur], deps[1 - cur], G)
        cur = 1 - cur
        left.append(float(planes[cur][0, -1]))
        a = tl._exact_sum(S, list(vol) + list(inf), Q, left)
        S, inf = tl.np_lake_take(mc, ml, S, inf, Q)
        vol, inf, planes[cur], _, _, _ = tl.np_lake_release(vol, inf, par, np.array([BW_LAKE], np.int32), planes[cur], Q, BW_DT)
        deps[cur] = np_lake_depth(mc, ml, 1, vol, par["area"], np.array([datum], F8), bed, deps[cur], Q)
        assert tl._exact_sum(S, list(vol) + list(inf), Q, left) == a, "the lake calls move the exact sum by 0"
        stage = F(datum + float(vol[0]) * Q / par["area"][0] - float(bed[0, BW_LAKE]))
        assert deps[cur][0, BW_LAKE] == stage
        record.append((planes[cur][0, up], deps[cur][0, up], deps[cur][0, BW_LAKE]))
    outs, hs = np.array([r[0] for r in record]), np.array([r[1] for r in record])
    first = int(np.argmax(outs > 0))
    print("lake backwater: the cell upstream releases first in call %d of %d at depth %.3f m under a lake stage of %.3f m; diag %r"
          % (first, BW_CALLS, hs[first - 1], record[first - 1][2], G.tolist()))
    assert 20 < first < BW_CALLS and (outs[:first].view(U32) == 0).all() and (np.diff(hs[:first]) > 0).all(), "blocked, and the depth grows"
    assert (outs[first:] > 0).all(), "it releases from then on"
    assert hs[first - 1] + F(0.5) > record[first - 1][2] - F(0.02), "it spills when its surface reaches the lake's"
    return S, planes, deps, cur, vol, G, outs, hs, record, first


def test_lake_backwater_restated():
    """The restated backwater run on its own (no GPU): the assertions are inside _backwater_restated."""
    S, planes, deps, cur, vol, G, outs, hs, record, first = _backwater_restated()
    assert int(G[3]) >= first - 1 and int(vol[0]) > int(np.floor(1.75 * ROW_W * ROW_L / Q)), "the lake has taken what reached it"


@pytest.mark.gpu
def test_gpu_lake_backwater_through_lakes(engine):
    """A one-cell lake whose surface (set_volume_m3, set_datum) stands 1.25 m above the bed of the channel cell that drains into it:
    under DiffusiveFlow that cell's out is +0 and its depth grows in every call until drop + (h - hd) > 0, and it releases from then on;
    every word of storage, out, depth and the lake's volume equals a restated run (np_route_diffusive, test_lakes' take and release,
    np_lake_depth), in which the take, the release and the depth call move the exact sum of lake volume and network water by 0; the
    depth plane at the member is the float64 stage.  The same setup under ChannelFlow releases from the first call."""
    import types
    import torch
    from noahmp_amd.routing import ChannelFlow, DiffusiveFlow, FlowNetwork, Lakes
    bed, x, par = _backwater_row()
    up = BW_LAKE - 1                                                     # the channel cell that drains into the lake
    datum = float(bed[0, BW_LAKE])                                       # level 0 at the member's bed
    vol0 = 1.75 * ROW_W * ROW_L                                          # the surface 1.75 m above the member's bed: 1.25 m above the cell upstream
    lake_id = np.zeros((1, BW_N), np.int32)
    lake_id[0, BW_LAKE] = 1
    store = types.SimpleNamespace(ni=BW_N, nj=1, a=dict(runsfxy=_dev(x["runoff_a"]), runsbxy=_dev(np.zeros(BW_N, F))))

    def make(cls):
        net = FlowNetwork(engine, BW_N, 1)
        net.set_directions(_dev(x["dir"]), dx=ROW_L, dy=ROW_L)
        net.set_area(_dev(x["area"]))
        net.set_input_columns(None)
        flow = cls(net)
        flow.set_geometry(ROW_W, ROW_N, smin=SMIN, height=_dev(bed))
        lakes = Lakes(flow)
        lakes.set_lakes(lake_id, par, [(BW_LAKE, 0)])
        lakes.set_volume_m3(vol0)
        lakes.set_datum(datum)
        lakes.attach()
        return net, flow, lakes

    S, planes, deps, cur, vol, G, outs, hs, record, first = _backwater_restated()
    # the device run
    net, df, lakes = make(DiffusiveFlow)
    torch.cuda.synchronize()
    seen = []
    for _ in range(BW_CALLS):
        df.step(store, BW_DT)
        seen.append(net.out[net.cur][0, up].clone())
    engine.stream_sync()
    torch.cuda.synchronize()
    assert_run((net.storage.cpu().numpy(), net.out[net.cur].cpu().numpy(), df.depth().cpu().numpy(), df.diag.cpu().numpy().view(U32)),
               (S, planes[cur], deps[cur], G), "backwater run")
    assert lakes.volume.cpu().numpy().tolist() == vol.tolist() and df.blocked() == int(G[3]) >= first - 1
    assert_same(torch.stack(seen).cpu().numpy(), outs, "out of the cell upstream of the lake, every call")
    assert df.depth().cpu().numpy()[0, BW_LAKE] == record[-1][2], "the depth plane at the member is the lake's stage"
    # the kinematic wave has no backwater
    netk, ch, lakesk = make(ChannelFlow)
    torch.cuda.synchronize()
    for _ in range(2):                                                   # water reaches the cell in the second call
        ch.step(store, BW_DT)
    engine.stream_sync()
    assert float(netk.out[netk.cur][0, up].item()) > 0, "under ChannelFlow the cell releases in the first call in which it holds water"
    assert hs[1] > 0 and outs[1].view(U32) == 0, "under DiffusiveFlow it holds water in that call and releases +0"
