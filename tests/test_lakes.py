"""Lakes on the D8 network: level-pool storage and outflow (noahmp_hip_lake_take, noahmp_hip_lake_release; nmp_dev_lakes.hpp;
routing.Lakes).

No reference routine stands behind the calls; the contract is the text in include/noahmp_hip.h.  np_lake_take and np_lake_release restate
it: the take in numpy, the release per lake with numpy's float64 scalars and Python integers, one rounded operation per line.  Everything
is compared with the restatement word for word: the per-item functions compiled for the host, both kernels (and the per-lane-atomic
variant of the take), and runs through routing.Lakes.  A tolerance appears only in the steady-state check; it is derived there."""
import ctypes as C
import functools
import json
import math
import os
import subprocess

import numpy as np
import pytest

from noahmp_amd import abi
import test_channel as tc
import test_regrid as tr
import test_routing as trt
import test_shadow as tsh
import test_skyview as tsv
from test_regrid import F, assert_same
from test_routing import CUT, DX, DY, POISON, U32, np_flow_dir, np_inmask

ROOT = tr.ROOT
CSRC = tr.CSRC
SRC = os.path.join(ROOT, "tests", "host_emul", "lakes_check.hip")
LIB = os.path.join(ROOT, "tests", "host_emul", "liblakes_check.so")
LIB_PER_LANE = os.path.join(CSRC, "variants", "lib_lakes_per_lane.so")     # the library with -DNMP_LAKES_PER_LANE=1
HEADER = os.path.join(ROOT, "include", "noahmp_hip.h")
REFUSAL_FIXTURE = os.path.join(ROOT, "tests", "golden", "lakes_refusal_text.json")
WINDOWS = [(65, 5), (67, 35), CUT]
Q = 2.0 ** -10
I64 = np.int64
F8 = np.float64
PARAMS = ("area", "weir_h", "weir_c", "weir_l", "orifice_h", "orifice_c", "orifice_a")
CAP = 2 ** 62
TWO_G = F8(19.6133)
DT = 300.0
NEVER = 1e30                                                             # a crest no level reaches


# ---------------------------------------------------------------------------------------------------------------- the restatement
def np_lake_take(member_cell, member_lake, storage, inflow, q, detail=None):
    """One call of noahmp_hip_lake_take: (storage', inflow').  detail: a list that receives (s, n, rem) of the taken cells."""
    st = np.array(storage, F)
    flat = st.reshape(-1)
    inf = np.array(inflow, I64)
    ncell, nlake = flat.size, inf.size
    mc, ml = np.asarray(member_cell, I64), np.asarray(member_lake, I64)
    valid = (mc >= 0) & (mc < ncell) & (ml >= 0) & (ml < nlake)
    c, l = mc[valid], ml[valid]
    assert np.unique(c).size == c.size, "a cell is listed at most once"
    q = F8(q)
    invq = F8(1.0) / q
    with np.errstate(all="ignore"):
        s = flat[c]
        ok = s >= F(q)
        t = s.astype(F8) * invq
        ok &= t < F8(CAP)
        n = np.floor(np.where(ok, t, 0.0)).astype(I64)
        nq = n.astype(F8) * q
        rem = (s.astype(F8) - nq).astype(F)
    flat[c[ok]] = rem[ok]
    np.add.at(inf, l[ok], n[ok])
    if detail is not None:
        detail.append((s[ok], n[ok], rem[ok], s[~ok]))
    return st, inf


def np_lake_release(volume, inflow, par, outlet_cell, out_new, q, dt, level=None, outflow=None, diag=None, trace=None):
    """One call of noahmp_hip_lake_release: (volume', inflow', out_new', level', outflow', diag').  level / outflow / diag None: not given
    to the call.  trace: a list that receives the set of paths every lake took."""
    vol, inf = np.array(volume, I64), np.array(inflow, I64)
    out = np.array(out_new, F)
    oflat = out.reshape(-1)
    ncell = oflat.size
    level = None if level is None else np.array(level, F8)
    outflow = None if outflow is None else np.array(outflow, F)
    diag = None if diag is None else np.array(diag, U32)
    q, dt = F8(q), F8(dt)
    invq = F8(1.0) / q
    p = {k: np.asarray(par[k], F8) for k in PARAMS}
    with np.errstate(all="ignore"):
        for l in range(vol.size):
            tags = set()
            v0 = int(vol[l]) + int(inf[l])
            inf[l] = 0
            area = p["area"][l]
            volm = F8(float(v0)) * q
            h = volm / area if area > 0 else F8(0.0)
            tags.add("area" if area > 0 else "no area")
            hw = h - p["weir_h"][l]
            qw = F8(0.0)
            if hw > 0:
                r = np.sqrt(hw)
                a = p["weir_c"][l] * p["weir_l"][l]
                b = a * hw
                qw = b * r
                tags.add("weir")
            ho = h - p["orifice_h"][l]
            qo = F8(0.0)
            if ho > 0:
                g = TWO_G * ho
                r = np.sqrt(g)
                a = p["orifice_c"][l] * p["orifice_a"][l]
                qo = a * r
                tags.add("orifice")
            qt = qw + qo
            od = qt * dt
            t = od * invq
            n = 0
            if t >= 1:
                n = int(math.floor(t)) if t < F8(CAP) else CAP
                tags.add("t below 2^62" if t < F8(CAP) else "t at or above 2^62")
            elif t != t:
                tags.add("od nan")
            elif t > 0:
                tags.add("t below 1")
            if v0 <= 0:
                n = 0
                tags.add("nothing held")
            elif n > v0:
                n = v0
                tags.add("capped")
            emptied = n > 0 and n == v0
            if emptied:
                tags.add("emptied")
            if n >= 2 ** 24:
                sh = n.bit_length() - 24
                if (n >> sh) << sh != n:
                    tags.add("bits cut")
                n = (n >> sh) << sh
                tags.add("truncated")
            vol[l] = v0 - n
            o = F(F8(float(n)) * q)
            assert float(o) == n * float(q), "n*q is a float32 value"
            oc = int(outlet_cell[l])
            if 0 <= oc < ncell:
                oflat[oc] = o
                tags.add("outlet owned")
            else:
                tags.add("outlet not owned")
            if n > 0:
                tags.add("released")
            if level is not None:
                level[l] = h
            if outflow is not None:
                outflow[l] = o
            if diag is not None:
                diag[0] = (int(diag[0]) + int(emptied)) & 0xFFFFFFFF
            if trace is not None:
                trace.append(tags)
    return vol, inf, out, level, outflow, diag


# ---------------------------------------------------------------------------------------------------------------- the inputs
@functools.lru_cache(maxsize=None)
def layout(ni, nj):
    """The lakes of a window as lists of cells: 1, 63, 64, 65 and 257 members (100 where 257 do not fit: the 65 x 5 window has 325
    cells), a lake with no member, and one of 3 behind it.  The cells are scattered: the calls do not look at where a cell lies."""
    ncell = ni * nj
    sizes = [1, 63, 64, 65, 257 if ncell >= 193 + 257 + 3 + 16 else 100, 0, 3]
    r = np.random.default_rng(300 + ncell)
    perm = r.permutation(ncell)
    cells, at = [], 0
    for n in sizes:
        cells.append(np.sort(perm[at:at + n]).astype(I64))
        at += n
    return dict(ncell=ncell, nlake=len(sizes), cells=cells, unused=perm[at:].astype(I64))


def list_forms(ni, nj):
    """[(name, member_cell, member_lake)]: sorted by lake and padded to whole waves with -1; shuffled without pads; shuffled with -1 and
    out-of-range entries; the empty list."""
    lay = layout(ni, nj)
    ncell, nlake = lay["ncell"], lay["nlake"]
    r = np.random.default_rng(17 + ncell)
    mc, ml = [], []
    for l, c in enumerate(lay["cells"]):
        pad = (-c.size) % 64
        mc += [c, np.full(pad, -1, I64)]
        ml += [np.full(c.size, l, I64), np.full(pad, -1, I64)]
    sorted_c, sorted_l = np.concatenate(mc), np.concatenate(ml)
    plain_c = np.concatenate(lay["cells"])
    plain_l = np.concatenate([np.full(c.size, l, I64) for l, c in enumerate(lay["cells"])])
    order = r.permutation(plain_c.size)
    shuf_c, shuf_l = plain_c[order], plain_l[order]
    u = lay["unused"]
    bad_c = np.array([-1, ncell, ncell + 5, 2 ** 31 - 1, -2 ** 31, u[0], u[1], u[2], -7, u[3]], I64)
    bad_l = np.array([-1, 0, 1, 2, 0, nlake, -3, 2 ** 31 - 1, 4, -2 ** 31], I64)
    wild_c, wild_l = np.concatenate([shuf_c, bad_c]), np.concatenate([shuf_l, bad_l])
    order = r.permutation(wild_c.size)
    i32 = lambda a: a.astype(np.int32)      # noqa: E731
    return [("sorted and padded", i32(sorted_c), i32(sorted_l)), ("shuffled", i32(shuf_c), i32(shuf_l)),
            ("with pads and out-of-range entries", i32(wild_c[order]), i32(wild_l[order])), ("empty", np.zeros(0, np.int32), np.zeros(0, np.int32))]


def lake_storage(ni, nj, q=Q, seed=0):
    """A storage plane: water everywhere, and on the members of the largest lake the special words of the text."""
    lay = layout(ni, nj)
    r = np.random.default_rng(23 + lay["ncell"] + seed)
    s = r.uniform(0.0, 3.0e3, (nj, ni)).astype(F)
    flat = s.reshape(-1)
    small = r.random(lay["ncell"]) < 0.1
    flat[small] = r.choice(np.array([q / 2, 0.0, 1e-30, -0.0, q * (1 - 2.0 ** -24)], F), int(small.sum()))
    c = lay["cells"][4]
    flat[c[:9]] = np.array([np.nan, -1.0, np.inf, CAP * q, CAP * q / 2, q / 2, q, 0.0, 3 * q], F)
    return s


INFLOW0 = np.array([5, 0, -3, 1 << 40, 7, 11, 0], I64)                   # the call accumulates and never zeroes


RELEASE_NAMES = ("weir only", "orifice only", "both", "neither", "area 0", "area negative", "capped", "truncated", "od nan", "nothing held",
                 "t infinite", "negative volume", "inflow only", "t below 1", "exactly 2^24")


def release_case(ncell, q=Q):
    """The lakes of RELEASE_NAMES: (par, volume, inflow, outlet_cell)."""
    n = len(RELEASE_NAMES)
    par = dict(area=np.full(n, 1.0e4), weir_h=np.full(n, 2.0), weir_c=np.full(n, 1.7), weir_l=np.full(n, 5.0), orifice_h=np.full(n, 0.5),
               orifice_c=np.full(n, 0.6), orifice_a=np.full(n, 0.3))
    words = lambda m3: int(m3 / q)      # noqa: E731
    vol = np.full(n, words(2.5e4), I64)                                  # h = 2.5 m
    inf = np.arange(n, dtype=I64) * 3
    k = RELEASE_NAMES.index
    par["orifice_h"][k("weir only")] = NEVER
    par["weir_h"][k("orifice only")] = NEVER
    par["weir_h"][k("neither")], par["orifice_h"][k("neither")] = 3.0, 2.75
    par["area"][k("area 0")], par["weir_h"][k("area 0")] = 0.0, -1.0
    par["area"][k("area negative")], par["orifice_h"][k("area negative")] = -5.0, -0.25
    vol[k("capped")], par["area"][k("capped")], par["weir_h"][k("capped")], par["weir_l"][k("capped")] = words(10.0), 100.0, 0.0, 1.0e6
    vol[k("truncated")], par["area"][k("truncated")], par["weir_h"][k("truncated")], par["weir_l"][k("truncated")] = words(1.0e9), 1.0e6, 0.0, 1.0
    par["weir_c"][k("od nan")] = np.nan
    vol[k("nothing held")], inf[k("nothing held")], par["weir_h"][k("nothing held")] = 0, 0, -1.0
    par["weir_c"][k("t infinite")], par["weir_l"][k("t infinite")] = 1.0e300, 1.0e300
    vol[k("negative volume")], inf[k("negative volume")] = -5, 2
    vol[k("inflow only")], inf[k("inflow only")] = 0, words(3.0e4)
    par["weir_l"][k("t below 1")], par["weir_c"][k("t below 1")], par["orifice_h"][k("t below 1")] = 1.0e-12, 1.0, NEVER
    # hw = 2.5 - 1.5 = 1 exactly (no inflow: 2.5e4 m3 is a whole number of quanta), so od = l*dt lies at (2^24 + 0.5) q and floor()
    # gives 2^24, the smallest truncated count: nothing is cut from it
    par["weir_h"][k("exactly 2^24")], par["weir_c"][k("exactly 2^24")], par["orifice_h"][k("exactly 2^24")] = 1.5, 1.0, NEVER
    par["weir_l"][k("exactly 2^24")], inf[k("exactly 2^24")] = (2 ** 24 + 0.5) * q / DT, 0
    r = np.random.default_rng(ncell)
    oc = r.permutation(ncell)[:n].astype(np.int32)
    oc[k("neither")], oc[k("area negative")], oc[k("od nan")], oc[k("t below 1")] = -1, ncell, min(ncell + 3, 2 ** 31 - 1), -2 ** 31
    return par, vol, inf, oc


OPTS = ((True, True, True), (False, False, False), (True, False, True), (False, True, False))      # (level, outflow, diag)


# ---------------------------------------------------------------------------------------------------------------- CPU
def build():
    """The host checker: nmp_dev_lakes.hpp compiled for the CPU.  Needs nothing of the engine library."""
    deps = [SRC, HEADER, os.path.join(CSRC, "nmp_dev_lakes.hpp")]
    if not os.path.exists(LIB) or any(os.path.getmtime(p) > os.path.getmtime(LIB) for p in deps):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off",
                               "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), SRC, "-o", LIB])


def build_variant():
    """The variant library in which every lane of the take sends its own atomic: one translation unit compiled again."""
    from noahmp_amd import build as b
    b.build_unit_variant("noahmp_lakes.hip", ["-DNMP_LAKES_PER_LANE=1"], LIB_PER_LANE)


@functools.lru_cache(maxsize=None)
def _host():
    build()
    try:
        import torch  # noqa: F401  (map torch's HIP runtime first, noahmp_amd/abi.py::load_library)
    except ImportError:
        pass
    lib = C.CDLL(LIB)
    V, L, I, D = C.c_void_p, C.c_longlong, C.c_int, C.c_double
    lib.lake_take_entries.argtypes = [V, V, L, V, V, I, L, D]
    lib.lake_release_lakes.argtypes = [V] * 11 + [L, V, V, V, I, D, D]
    lib.lake_take_entries.restype = lib.lake_release_lakes.restype = None
    return lib


_p, _c = trt._p, trt._c


def host_lake_take(member_cell, member_lake, storage, inflow, q, detail=None):
    mc, ml = _c(member_cell, np.int32), _c(member_lake, np.int32)
    st, inf = _c(storage).copy(), _c(inflow, I64).copy()
    _host().lake_take_entries(_p(mc), _p(ml), mc.size, _p(st), _p(inf), inf.size, st.size, float(q))
    return st, inf


def host_lake_release(volume, inflow, par, outlet_cell, out_new, q, dt, level=None, outflow=None, diag=None, trace=None):
    vol, inf, out = _c(volume, I64).copy(), _c(inflow, I64).copy(), _c(out_new).copy()
    pl = [_c(par[k], F8) for k in PARAMS]
    oc = _c(outlet_cell, np.int32)
    level = None if level is None else _c(level, F8).copy()
    outflow = None if outflow is None else _c(outflow).copy()
    diag = None if diag is None else _c(diag, U32).copy()
    _host().lake_release_lakes(_p(vol), _p(inf), *[_p(a) for a in pl], _p(oc), _p(out), out.size, _p(level), _p(outflow), _p(diag), vol.size,
                               float(q), float(dt))
    return vol, inf, out, level, outflow, diag


def same_words(a, b, what):
    """0 differing words: integer words as they are, floats bit for bit (or both NaN)."""
    assert (a is None) == (b is None), what
    if a is None:
        return
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype.kind == "f":
        u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
        bad = ~((a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b)))
    else:
        bad = a != b
    assert not bad.any(), "%s: %d of %d words differ, first at %s: %r vs %r" % (what, bad.sum(), bad.size, np.argwhere(bad)[0], a[bad][0], b[bad][0])


def assert_release(got, want, what):
    for g, w, nm in zip(got, want, ("volume", "inflow", "out_new", "level", "outflow", "diag")):
        same_words(g, w, "%s: %s" % (what, nm))


@functools.lru_cache(maxsize=None)
def take_cases(ni, nj):
    """[(what, member_cell, member_lake, storage, inflow, q, (storage', inflow') of the restatement)] -- made once, shared by the host
    and the device tests."""
    out = []
    for q in (Q, 8.0):
        s = lake_storage(ni, nj, q)
        for name, mc, ml in list_forms(ni, nj):
            out.append(("%dx%d %s q %g" % (ni, nj, name, q), mc, ml, s, INFLOW0, q, np_lake_take(mc, ml, s, INFLOW0, q)))
    name, mc, ml = list_forms(ni, nj)[2]
    out.append(("%dx%d no lakes" % (ni, nj), mc, ml, s, np.zeros(0, I64), Q, np_lake_take(mc, ml, s, np.zeros(0, I64), Q)))
    return out


@functools.lru_cache(maxsize=None)
def release_cases(ni, nj):
    """[(what, par, volume, inflow, outlet_cell, out_new, level, outflow, diag, q, dt, want)]."""
    ncell = ni * nj
    out = []
    r = np.random.default_rng(ncell + 1)
    plane = r.uniform(0.0, 10.0, (nj, ni)).astype(F)
    for n, q in enumerate((Q, Q, 8.0, 2.0 ** -20)):
        par, vol, inf, oc = release_case(ncell, q)
        wl, wo, wd = OPTS[n]
        nl = vol.size
        lev = np.full(nl, 7.0, F8) if wl else None
        ofl = np.full(nl, POISON, F) if wo else None
        dg = np.array([3], U32) if wd else None
        want = np_lake_release(vol, inf, par, oc, plane, q, DT, lev, ofl, dg)
        out.append(("%dx%d q %g level %s outflow %s diag %s" % (ni, nj, q, wl, wo, wd), par, vol, inf, oc, plane, lev, ofl, dg, q, DT, want))
    empty = {k: np.zeros(0, F8) for k in PARAMS}
    z64 = np.zeros(0, I64)
    out.append(("%dx%d no lakes" % (ni, nj), empty, z64, z64, np.zeros(0, np.int32), plane, None, None, np.array([3], U32), Q, DT,
                np_lake_release(z64, z64, empty, np.zeros(0, np.int32), plane, Q, DT, None, None, np.array([3], U32))))
    return out


@pytest.mark.parametrize("ni, nj", WINDOWS)
def test_host_take_equals_the_restatement(ni, nj):
    """The compiled lake_take_entry over every list form (sorted and padded, shuffled, with -1 and out-of-range entries, empty, no lakes)
    against np_lake_take: 0 differing words of storage and inflow."""
    for what, mc, ml, s, inf, q, want in take_cases(ni, nj):
        got = host_lake_take(mc, ml, s, inf, q)
        same_words(got[0], want[0], what + ": storage")
        same_words(got[1], want[1], what + ": inflow")


@pytest.mark.parametrize("ni, nj", WINDOWS)
def test_host_release_equals_the_restatement(ni, nj):
    """The compiled lake_release_one over the lakes of RELEASE_NAMES, with and without level, outflow and diag, three quanta: 0
    differing words of volume, inflow, out_new, level, outflow and diag."""
    for what, par, vol, inf, oc, plane, lev, ofl, dg, q, dt, want in release_cases(ni, nj):
        assert_release(host_lake_release(vol, inf, par, oc, plane, q, dt, lev, ofl, dg), want, what)


def test_the_cases_reach_every_path():
    """The inputs above reach: a storage taken, one below a quantum, NaN, -1 and +Inf storages, one >= 2^62 q; weir only, orifice only,
    both, neither; area <= 0; a release capped by the volume (emptied); a truncated release (n >= 2^24) that loses bits; od NaN; an
    outlet that is not owned; and the lake sizes 1, 63, 64, 65 and 257."""
    ni, nj = 67, 35
    lay = layout(ni, nj)
    assert [c.size for c in lay["cells"]] == [1, 63, 64, 65, 257, 0, 3]
    assert [c.size for c in layout(*CUT)["cells"]] == [1, 63, 64, 65, 257, 0, 3] and [c.size for c in layout(65, 5)["cells"]][4] == 100
    detail = []
    name, mc, ml = list_forms(ni, nj)[2]
    s = lake_storage(ni, nj)
    np_lake_take(mc, ml, s, INFLOW0, Q, detail)
    taken, n, rem, left = detail[0]
    assert taken.size > 300 and (n >= 1).all() and (n == 1).any() and (n == CAP // 2).any()
    with np.errstate(invalid="ignore"):
        assert np.isnan(left).any() and (left == -1).any() and (left == np.inf).any() and (left == F(CAP * Q)).any()
        assert ((left >= 0) & (left < F(Q))).any() and (left == F(Q * (1 - 2.0 ** -24))).any()
    assert (mc == -1).any() and (mc >= ni * nj).any() and (ml >= lay["nlake"]).any() and (ml < -1).any()
    trace = []
    par, vol, inf, oc = release_case(ni * nj)
    np_lake_release(vol, inf, par, oc, np.zeros((nj, ni), F), Q, DT, trace=trace)
    t = dict(zip(RELEASE_NAMES, trace))
    assert {"weir", "orifice"} & t["weir only"] == {"weir"} and {"weir", "orifice"} & t["orifice only"] == {"orifice"}
    assert {"weir", "orifice"} <= t["both"] and not {"weir", "orifice"} & t["neither"] and "released" not in t["neither"]
    assert "no area" in t["area 0"] and "weir" in t["area 0"] and "no area" in t["area negative"] and "orifice" in t["area negative"]
    assert {"capped", "emptied"} <= t["capped"] and "truncated" not in t["capped"]
    assert {"truncated", "bits cut", "released"} <= t["truncated"] and "capped" not in t["truncated"]
    assert "od nan" in t["od nan"] and "released" not in t["od nan"]
    assert "nothing held" in t["nothing held"] and "t below 2^62" in t["nothing held"]
    assert {"t at or above 2^62", "capped", "emptied", "truncated"} <= t["t infinite"]
    assert "nothing held" in t["negative volume"] and "released" in t["inflow only"]
    assert "t below 1" in t["t below 1"] and "released" not in t["t below 1"]
    assert "truncated" in t["exactly 2^24"] and "bits cut" not in t["exactly 2^24"]
    assert sum("outlet not owned" in x for x in trace) == 4 and "outlet owned" in t["both"]


@pytest.mark.parametrize("ni, nj", WINDOWS)
def test_exactness(ni, nj):
    """Per taken cell rem + n*q == s in float64 and rem < q; a shuffled list, a padded list and a list split into four sub-lists taken
    in any order give the same inflow words (and storage); after a release (double)out_new[outlet] == n*q."""
    for q in (Q, 8.0, 2.0 ** -20):
        s = lake_storage(ni, nj, q)
        forms = list_forms(ni, nj)
        detail = []
        want = np_lake_take(forms[0][1], forms[0][2], s, INFLOW0, q, detail)
        taken, n, rem, _ = detail[0]
        assert taken.size and (rem.astype(F8) + n.astype(F8) * q == taken.astype(F8)).all() and (rem < F(q)).all() and (rem >= 0).all()
        for take in (np_lake_take, host_lake_take):
            for name, mc, ml in forms[1:3]:
                got = take(mc, ml, s, INFLOW0, q)
                same_words(got[0], want[0], name + ": storage")
                same_words(got[1], want[1], name + ": inflow")
            name, mc, ml = forms[1]
            for order in ((0, 1, 2, 3), (3, 1, 0, 2), (2, 3, 1, 0)):
                st, inf = s, INFLOW0
                for k in order:
                    st, inf = take(mc[k::4], ml[k::4], st, inf, q)
                same_words(st, want[0], "four sub-lists %r: storage" % (order,))
                same_words(inf, want[1], "four sub-lists %r: inflow" % (order,))
        par, vol, inf, oc = release_case(ni * nj, q)
        before = vol + inf
        v2, i2, out, _, ofl, _ = np_lake_release(vol, inf, par, oc, np.full((nj, ni), POISON, F), q, DT, outflow=np.zeros(vol.size, F))
        nrel = before - v2
        assert (i2 == 0).all() and (nrel >= 0).all() and (nrel > 0).sum() >= 8
        assert (ofl.astype(F8) == nrel.astype(F8) * q).all() and all(int(a) * q == float(b) for a, b in zip(nrel, ofl))
        owned = (oc >= 0) & (oc < ni * nj)
        assert (out.reshape(-1)[oc[owned]].astype(F8) == nrel[owned].astype(F8) * q).all()
        untouched = np.ones(ni * nj, bool)
        untouched[oc[owned]] = False
        assert (out.reshape(-1)[untouched] == POISON).all()


# ---------------------------------------------------------------------------------------------------------------- runs with the routing restatements
def _hold(plane, members):
    return np.where(members, F(0.0), plane).astype(F)


class LakeRun:
    """The restated chain routing call -> take -> release on one window.  route: np_route or np_route_kinematic (or compiled ones)."""

    def __init__(self, x, kinematic, members_of, par, outlet_cell, storage, out, q=Q, take=np_lake_take, release=np_lake_release, route=None):
        nj, ni = x["inmask"].shape
        self.members = np.zeros((nj, ni), bool)
        mc, ml = [], []
        for l, cells in enumerate(members_of):
            cells = np.sort(np.asarray(cells, I64))
            self.members.reshape(-1)[cells] = True
            mc.append(cells)
            ml.append(np.full(cells.size, l, I64))
        self.mc = np.concatenate(mc).astype(np.int32) if mc else np.zeros(0, np.int32)
        self.ml = np.concatenate(ml).astype(np.int32) if ml else np.zeros(0, np.int32)
        key = "conv" if kinematic else "release"
        self.x = dict(x, **{key: _hold(x[key], self.members)})
        self.kinematic, self.par, self.oc, self.q = kinematic, par, np.asarray(outlet_cell, np.int32), q
        self.take, self.release = take, release
        self.route = route or (tc.np_route_kinematic if kinematic else trt.np_route)
        nl = len(members_of)
        self.S, self.out, self.cur = np.array(storage, F), [np.array(out, F), np.array(out, F)], 0
        self.vol, self.inf = np.zeros(nl, I64), np.zeros(nl, I64)
        self.level, self.outflow, self.diag = np.zeros(nl, F8), np.zeros(nl, F), np.zeros(1, U32)

    def route_call(self):
        new = 1 - self.cur
        if self.kinematic:
            self.S, self.out[new], _, _ = self.route(self.x, self.out[self.cur], self.out[new], self.S, None, None)
        else:
            self.S, self.out[new] = self.route(self.x, self.out[self.cur], self.out[new], self.S)
        self.cur = new

    def take_call(self):
        self.S, self.inf = self.take(self.mc, self.ml, self.S, self.inf, self.q)

    def release_call(self, dt):
        self.vol, self.inf, self.out[self.cur], self.level, self.outflow, self.diag = self.release(
            self.vol, self.inf, self.par, self.oc, self.out[self.cur], self.q, dt, self.level, self.outflow, self.diag)

    def call(self, dt):
        self.route_call()
        self.take_call()
        self.release_call(dt)


def lake_params(nlake, **kw):
    par = dict(area=np.full(nlake, 1.0e4), weir_h=np.full(nlake, 1.0), weir_c=np.full(nlake, 1.7), weir_l=np.full(nlake, 10.0),
               orifice_h=np.full(nlake, NEVER), orifice_c=np.full(nlake, 0.6), orifice_a=np.full(nlake, 0.0))
    for k, v in kw.items():
        par[k] = np.broadcast_to(np.asarray(v, F8), (nlake,)).copy()
    return par


def hills_lake(ni, nj, z):
    """A lake on the hills that drains OUT of the network: the pit (a cell without a direction, away from the edge) with the most
    neighbours draining into it, and those neighbours.  Returns (dir, member cells, outlet cell)."""
    d = np_flow_dir(z, DX, DY)
    m = np_inmask(d)
    inner = np.zeros(d.shape, bool)
    inner[2:-2, 2:-2] = True
    pits = np.argwhere((d == 0) & inner & (m != 0))
    assert len(pits), "the hills have pits"
    count = [bin(int(m[j, i])).count("1") for j, i in pits]
    j, i = pits[int(np.argmax(count))]
    cells = [j * ni + i]
    for k in range(1, 9):
        if (int(m[j, i]) >> (k - 1)) & 1:
            cells.append((j + trt.DJ[k - 1]) * ni + i + trt.DI[k - 1])
    return d, np.array(cells, I64), int(j * ni + i)


def _exact_sum(storage, words, q, left):
    """storage + words*q + left as the correctly rounded float64 of the EXACT sum (math.fsum): equal exact sums give equal values."""
    return math.fsum([float(v) for v in storage.reshape(-1)] + [int(w) * float(q) for w in words] + list(left))


@pytest.mark.parametrize("kinematic", [False, True])
def test_budget_on_the_hills(kinematic):
    """30 calls of both routing schemes on the 70 x 130 hills with one lake that drains out of the network (its outlet has dir == 0):
    storage + (volume + inflow)*q + the cumulated outlet release is the same number before and after the take and before and after
    the release: the two lake calls contribute exactly 0, so the budget of a run with lakes moves only by the routing call's own
    float32 roundings (test_routing and test_channel count those).  The sums are math.fsum's, the correctly rounded value of the EXACT
    sum: equality of the exact sums is what is asserted."""
    ni, nj = CUT
    z = tsh.terrain(ni, nj, True)
    d, cells, outlet = hills_lake(ni, nj, z)
    ops = tc.kin_operands(ni, nj, "physical") if kinematic else trt.route_operands(ni, nj, "physical")
    ops["storage"] = np.abs(ops["storage"])
    ops["runoff_a"] = np.abs(ops["runoff_a"])
    ncell = ni * nj
    ident = np.arange(ncell, dtype=np.int32).reshape(nj, ni)
    if kinematic:
        ops["conv"] = np.where(ops["conv"] > 0, ops["conv"], F(0.02)).astype(F)
        x = tc._kblock(np_inmask(d), ident, ncell, ops)
    else:
        x = dict(inmask=np_inmask(d), col_index=ident, ncol=ncell, area=ops["area"], release=ops["release"], runoff_a=ops["runoff_a"],
                 runoff_b=ops["runoff_b"], scale=tc.SCALE)
    run = LakeRun(x, kinematic, [cells], lake_params(1, area=cells.size * DX * DY, weir_h=0.01, weir_l=30.0), [outlet], ops["storage"],
                  np.zeros((nj, ni), F))
    left, released = [], 0
    for n in range(30):
        run.route_call()
        assert run.out[run.cur].reshape(-1)[outlet] == 0 and (run.out[run.cur][run.members] == 0).all(), "members release +0"
        outs = d == 0
        outs.reshape(-1)[outlet] = False
        left += [float(v) for v in run.out[run.cur][outs]]               # what leaves at the other pits and the coast
        a = _exact_sum(run.S, list(run.vol) + list(run.inf), Q, left)
        run.take_call()
        b = _exact_sum(run.S, list(run.vol) + list(run.inf), Q, left)
        assert a == b, "the take contributes exactly 0"
        assert (run.S[run.members] < F(Q)).all()
        run.release_call(tc.DT)
        o = float(run.out[run.cur].reshape(-1)[outlet])
        c = _exact_sum(run.S, list(run.vol) + list(run.inf), Q, left + [o])
        assert b == c, "the release contributes exactly 0"
        left.append(o)
        released += o > 0                                                # it has left the network: nobody gathers from a cell without a direction
    assert released >= 20 and int(run.vol[0]) > 0


# ---------------------------------------------------------------------------------------------------------------- the physics
CHAIN_N = 10
CHAIN_DT = 60.0
CHAIN_AREA = 1.0e6


def chain(lakes, runoff):
    """A row of CHAIN_N cells draining east, every cell a linear reservoir that passes all it holds (release 1); runoff [mm/s] enters
    at cell 0.  lakes: [(first, last)] member ranges, the outlet the last member."""
    d = np.full((1, CHAIN_N), 1, np.uint8)
    d[0, -1] = 0
    ra = np.zeros(CHAIN_N, F)
    ra[0] = runoff
    x = dict(inmask=np_inmask(d), col_index=np.arange(CHAIN_N, dtype=np.int32).reshape(1, CHAIN_N), ncol=CHAIN_N,
             area=np.full((1, CHAIN_N), CHAIN_AREA, F), release=np.ones((1, CHAIN_N), F), runoff_a=ra, runoff_b=None,
             scale=float(F(F(CHAIN_DT) * F(1e-3))))
    return x, [np.arange(a, b + 1) for a, b in lakes], [b for a, b in lakes]


def test_steady_state():
    """Constant inflow into a chain with one lake: the outflow per call settles to the inflow per call and the level to
    weir_h + (Q/(c*l))^(2/3).
    The tolerance.  Per call the take moves V/q + d quanta with |d| < 1, since the cell keeps rem < q.  The release is n = floor(f(v0))
    with f smooth and of slope s = dt/tau quanta per quantum (tau = area / (dQ/dh), here about 590 s against dt = 60 s: s = 0.1).  With
    e = v0 - v*, f(v*) = V/q:  n = V/q + s*e - frac, 0 <= frac < 1, and e' = e - n + V/q + d' = (1 - s) e + frac + d', so once settled
    e lies in (-1/s, 2/s) and n - V/q = s*e - frac in (-2, 2): |o - V| < 2 q; the test allows 3 q, plus the 24-bit truncation, 2^-23 V,
    where n >= 2^24.  The level is the one the release was made from: Q(h) dt = V + s*e*q, a relative 2 q / V at most, so with
    Q ~ (h - weir_h)^(3/2): |h - h*| <= 2/3 (h* - weir_h) * 2 q / V; the test allows 2/3 (h* - weir_h) (4 q / V + 2^-23) + q/area + 1e-12.
    The transient has decayed by exp(-600*dt/tau) < 1e-26."""
    cl, weir_h, area = 17.0, 1.0, 1.0e4
    x, members, outlets = chain([(3, 5)], 5e-3)
    V = float(F(F(F(5e-3) * F(x["scale"])) * F(CHAIN_AREA)))              # the volume per call as the routing call makes it
    run = LakeRun(x, False, members, lake_params(1, area=area, weir_h=weir_h, weir_c=1.7, weir_l=10.0), outlets, np.zeros((1, CHAIN_N), F),
                  np.zeros((1, CHAIN_N), F))
    for _ in range(600):
        run.call(CHAIN_DT)
    tol_o = 3 * Q + 2.0 ** -23 * V
    hstar = weir_h + (V / CHAIN_DT / cl) ** (2.0 / 3.0)
    tol_h = 2.0 / 3.0 * (hstar - weir_h) * (4 * Q / V + 2.0 ** -23) + Q / area + 1e-12
    for _ in range(20):
        run.call(CHAIN_DT)
        o, h = float(run.outflow[0]), float(run.level[0])
        print("outflow %.6f of %.6f m3 per call (tolerance %.2g), level %.9f of %.9f m (tolerance %.2g)" % (o, V, tol_o, h, hstar, tol_h))
        assert abs(o - V) <= tol_o and abs(h - hstar) <= tol_h
    assert abs(V - 300.0) < 1e-3 and 0.4 < hstar - weir_h < 0.5


def _pulse(ncall, lakes, par):
    """A triangular flood pulse through the chain: per call what reaches the first lake and what the last outlet releases."""
    x, members, outlets = chain(lakes, 0.0)
    run = LakeRun(x, False, members, par, outlets, np.zeros((1, CHAIN_N), F), np.zeros((1, CHAIN_N), F))
    first = lakes[0][0]
    qin, qout = [], []
    for n in range(ncall):
        run.x["runoff_a"] = np.zeros(CHAIN_N, F)
        run.x["runoff_a"][0] = 2e-2 * max(0.0, 1.0 - abs(n - 20) / 15.0)
        run.call(CHAIN_DT)
        qin.append(float(run.out[1 - run.cur][0, first - 1]))            # gathered by the first member in this call
        qout.append(float(run.outflow[-1]))
    return np.array(qin), np.array(qout), run


def test_flood_pulse_is_lower_and_later():
    """A triangular pulse into a lake with a weir: the outlet's peak is lower and later than the inflow's, and all the water is
    accounted for."""
    qin, qout, run = _pulse(400, [(3, 5)], lake_params(1, area=2.0e4, weir_h=0.0, weir_l=5.0))
    assert qin.max() > 0 and 0.1 * qin.max() < qout.max() < 0.8 * qin.max()
    assert int(np.argmax(qout)) > int(np.argmax(qin)) + 3
    assert math.fsum(qin) == pytest.approx(math.fsum(qout) + float(run.vol[0]) * Q + float(run.S[0, 3:6].sum()), rel=1e-6)


def test_transparent_lake():
    """weir_h = 0 and a huge c*l: the lake passes everything it holds in each call, up to the 24-bit truncation (what is cut stays)."""
    x, members, outlets = chain([(3, 5)], 0.0)
    run = LakeRun(x, False, members, lake_params(1, weir_h=0.0, weir_l=1.0e12), outlets, np.zeros((1, CHAIN_N), F), np.zeros((1, CHAIN_N), F))
    seen = 0
    for n in range(60):
        run.x["runoff_a"] = np.zeros(CHAIN_N, F)
        run.x["runoff_a"][0] = (0.0, 3e-3, 3.0, 7e2)[n % 4]              # up to 4e10 quanta per call: far above 2^24
        held = int(run.vol[0])
        run.route_call()
        run.take_call()
        v0 = held + int(run.inf[0])
        run.release_call(CHAIN_DT)
        n_out = v0 - int(run.vol[0])
        sh = max(0, v0.bit_length() - 24)
        assert n_out == (v0 >> sh) << sh and int(run.vol[0]) < max(1, v0 >> 23) and float(run.outflow[0]) == n_out * Q
        seen += v0 >= 2 ** 24
    assert seen > 20 and run.diag[0] > 0


def test_cascade():
    """Two lakes in cascade: the pulse is attenuated twice (the second outlet peaks lower and later than the first), and with constant
    inflow both settle to the inflow."""
    par = lake_params(2, area=2.0e4, weir_h=0.0, weir_l=5.0)
    x, members, outlets = chain([(2, 3), (6, 7)], 0.0)
    run = LakeRun(x, False, members, par, outlets, np.zeros((1, CHAIN_N), F), np.zeros((1, CHAIN_N), F))
    q1, q2 = [], []
    for n in range(500):
        run.x["runoff_a"] = np.zeros(CHAIN_N, F)
        run.x["runoff_a"][0] = 2e-2 * max(0.0, 1.0 - abs(n - 20) / 15.0)
        run.call(CHAIN_DT)
        q1.append(float(run.outflow[0]))
        q2.append(float(run.outflow[1]))
    assert max(q2) < 0.9 * max(q1) and int(np.argmax(q2)) > int(np.argmax(q1)) + 3
    x, members, outlets = chain([(2, 3), (6, 7)], 5e-3)
    run = LakeRun(x, False, members, par, outlets, np.zeros((1, CHAIN_N), F), np.zeros((1, CHAIN_N), F))
    for _ in range(1500):
        run.call(CHAIN_DT)
    V = float(F(F(F(5e-3) * F(x["scale"])) * F(CHAIN_AREA)))
    assert abs(float(run.outflow[0]) - V) <= 3 * Q + 2.0 ** -23 * V and abs(float(run.outflow[1]) - V) <= 6 * Q + 2.0 ** -22 * V


# ---------------------------------------------------------------------------------------------------------------- decomposition
def corner_lake(ni, nj, d):
    """A lake of 6 x 6 cells across the corner of the 2 x 2 cut; its outlet is the first member whose downstream cell is no member."""
    jj, ii = np.meshgrid(np.arange(nj // 2 - 3, nj // 2 + 3), np.arange(ni // 2 - 3, ni // 2 + 3), indexing="ij")
    cells = (jj * ni + ii).reshape(-1)
    inside = np.zeros((nj, ni), bool)
    inside.reshape(-1)[cells] = True
    for c in cells:
        j, i = divmod(int(c), ni)
        k = int(d[j, i])
        if k and not inside[j + trt.DJ[k - 1], i + trt.DI[k - 1]]:
            return cells.astype(I64), int(c)
    raise AssertionError("no member drains out of the square")


def whole_and_parts(kinematic=False):
    """The whole 70 x 130 domain with the corner lake and its four parts (blocks = tile + ring inside the domain): (whole LakeRun
    arguments, per part a dict)."""
    ni, nj = CUT
    z = tsh.terrain(ni, nj, True)
    d = np_flow_dir(z, DX, DY)
    cells, outlet = corner_lake(ni, nj, d)
    ncell = ni * nj
    ident = np.arange(ncell, dtype=np.int32).reshape(nj, ni)
    if kinematic:
        ops = tc.kin_operands(ni, nj, "physical")
        x = tc._kblock(np_inmask(d), ident, ncell, ops)
        planes = ("area", "width", "length", "conv")
    else:
        ops = trt.route_operands(ni, nj, "physical")
        x = dict(inmask=np_inmask(d), col_index=ident, ncol=ncell, area=ops["area"], release=ops["release"], runoff_a=ops["runoff_a"],
                 runoff_b=ops["runoff_b"], scale=tc.SCALE)
        planes = ("area", "release")
    par = lake_params(1, area=cells.size * DX * DY, weir_h=0.001, weir_l=20.0)
    member = np.zeros((nj, ni), bool)
    member.reshape(-1)[cells] = True
    parts = []
    for tile, blk, dblk, owned in trt._parts(ni, nj, z, 2):
        xp = dict(x, inmask=np_inmask(dblk), col_index=np.where(owned, ident[blk], -2).astype(np.int32), **{k: x[k][blk] for k in planes})
        nib = owned.shape[1]
        mine = member[blk] & owned
        bcells = np.flatnonzero(mine.reshape(-1))
        gidx = ident[blk]
        oc = np.flatnonzero((gidx.reshape(-1) == outlet) & owned.reshape(-1))
        parts.append(dict(x=xp, tile=tile, blk=blk, owned=owned, cells=bcells, outlet=int(oc[0]) if oc.size else -1, nib=nib))
    return dict(ni=ni, nj=nj, z=z, d=d, x=x, ops=ops, cells=cells, outlet=outlet, par=par, member=member), parts


@pytest.mark.parametrize("compiled", [False, True])
def test_decomposition(compiled):
    """The four parts of 70 x 130 with a lake across the corner of the cut, through the restatements (and the compiled functions):
    per call the four partial inflow words sum to the whole's; after 20 calls storage, out and volume have 0 differing words.  The lake
    has members on all four parts and one part owns the outlet."""
    w, parts = whole_and_parts()
    ni, nj, ops = w["ni"], w["nj"], w["ops"]
    fns = dict(take=host_lake_take, release=host_lake_release, route=trt._host_route) if compiled else {}
    whole = LakeRun(w["x"], False, [w["cells"]], w["par"], [w["outlet"]], ops["storage"], ops["out"], **fns)
    runs = [LakeRun(p["x"], False, [p["cells"]], w["par"], [p["outlet"]], ops["storage"][p["blk"]], ops["out"][p["blk"]], **fns) for p in parts]
    assert all(p["cells"].size > 0 for p in parts) and sum(p["outlet"] >= 0 for p in parts) == 1
    assert sum(p["cells"].size for p in parts) == w["cells"].size
    G, GS = ops["out"].copy(), ops["storage"].copy()
    for _ in range(20):
        whole.route_call()
        whole.take_call()
        want = whole.inf.copy()
        whole.release_call(tc.DT)
        for r in runs:
            r.route_call()
            r.take_call()
        total = sum(r.inf for r in runs)
        same_words(total, want, "the partial inflow words")
        assert sum(int(r.inf[0]) > 0 for r in runs) >= 2
        for r in runs:
            r.inf = total.copy()                                         # the sum over the ranks
            r.release_call(tc.DT)
        for p, r in zip(parts, runs):
            G[p["tile"]] = r.out[r.cur][p["owned"]].reshape(G[p["tile"]].shape)
            GS[p["tile"]] = r.S[p["owned"]].reshape(G[p["tile"]].shape)
        for p, r in zip(parts, runs):
            r.out[r.cur] = G[p["blk"]].copy()                            # the exchange: the release is written before out travels
    assert trt._differ(GS, whole.S) + trt._differ(G, whole.out[whole.cur]) == 0
    for r in runs:
        same_words(r.vol, whole.vol, "volume")
    assert int(whole.vol[0]) > 0 and float(whole.outflow[0]) > 0


# ---------------------------------------------------------------------------------------------------------------- refusals and bindings
TAKE_PLANES = ("member_cell", "member_lake", "storage", "inflow")
REL_PLANES = ("volume", "inflow") + PARAMS + ("outlet_cell", "out_new", "level", "outflow", "diag")
REL_REQUIRED = REL_PLANES[:11]
CALLS = ("noahmp_hip_lake_take", "noahmp_hip_lake_release")
NL, NM, NC = 3, 6, 16                                                    # lakes, entries and cells of the refusal blocks


def _take_block(ptrs, **kw):
    b = abi.LakeTake()
    for k in TAKE_PLANES:
        setattr(b, k, ptrs[k])
    b.nmember, b.nlake, b.ncell, b.quantum = NM, NL, NC, Q
    for k, v in kw.items():
        setattr(b, k, v)
    return b


def _rel_block(ptrs, **kw):
    b = abi.LakeRelease()
    for k in REL_PLANES:
        setattr(b, k, ptrs[k])
    b.nlake, b.ncell, b.quantum, b.dt = NL, NC, Q, DT
    for k, v in kw.items():
        setattr(b, k, v)
    return b


BAD_QUANTA = (("zero", 0.0), ("three", 3.0), ("nan", float("nan")), ("inf", float("inf")), ("neg", -Q), ("small", 2.0 ** -41), ("large", 2.0 ** 21),
              ("nearly", 1.0 + 2.0 ** -52))


def refusal_probes(tp, rp):
    """[(site id, call, block or None)]: one probe per refusal site and per way into it."""
    out = [("take.null", CALLS[0], None)]
    for nm, kw in (("nmember.neg", dict(nmember=-1)), ("nmember.big", dict(nmember=2 ** 31)), ("nlake.neg", dict(nlake=-1)),
                   ("ncell.neg", dict(ncell=-1)), ("ncell.big", dict(ncell=2 ** 31))):
        out.append(("take." + nm, CALLS[0], _take_block(tp, **kw)))
    for f in TAKE_PLANES:
        out.append(("take.required." + f, CALLS[0], _take_block(tp, **{f: None})))
    for nm, v in BAD_QUANTA:
        out.append(("take.quantum." + nm, CALLS[0], _take_block(tp, quantum=v)))
    for off in (1, 4):
        out.append(("take.inflow.misaligned.%d" % off, CALLS[0], _take_block(tp, inflow=tp["inflow"] + off)))
    out.append(("take.alias.storage.member_cell", CALLS[0], _take_block(tp, storage=tp["member_cell"])))
    out.append(("take.alias.inflow.member_lake", CALLS[0], _take_block(tp, inflow=tp["member_lake"])))
    out.append(("take.overlap.storage.member_lake", CALLS[0], _take_block(tp, member_lake=tp["storage"] + 4 * (NC - 1))))
    out.append(("release.null", CALLS[1], None))
    for f in REL_REQUIRED:
        out.append(("release.required." + f, CALLS[1], _rel_block(rp, **{f: None})))
    for nm, kw in (("nlake.neg", dict(nlake=-1)), ("ncell.neg", dict(ncell=-1)), ("ncell.big", dict(ncell=2 ** 31))):
        out.append(("release." + nm, CALLS[1], _rel_block(rp, **kw)))
    for nm, v in BAD_QUANTA[:3]:
        out.append(("release.quantum." + nm, CALLS[1], _rel_block(rp, quantum=v)))
    for nm, v in (("zero", 0.0), ("neg", -300.0), ("nan", float("nan")), ("inf", float("inf"))):
        out.append(("release.dt." + nm, CALLS[1], _rel_block(rp, dt=v)))
    for f in ("volume", "inflow", "area", "orifice_a", "level"):
        out.append(("release.misaligned8." + f, CALLS[1], _rel_block(rp, **{f: rp[f] + 4})))
    for f, off in (("outlet_cell", 2), ("out_new", 1), ("outflow", 3), ("diag", 2)):
        out.append(("release.misaligned4." + f, CALLS[1], _rel_block(rp, **{f: rp[f] + off})))
    out.append(("release.same.words", CALLS[1], _rel_block(rp, inflow=rp["volume"])))
    for f in ("volume", "weir_c", "outlet_cell", "level", "outflow", "diag"):
        out.append(("release.alias.out_new." + f, CALLS[1], _rel_block(rp, out_new=rp[f])))
    out.append(("release.overlap.out_new.area", CALLS[1], _rel_block(rp, area=rp["out_new"] + 4 * (NC - 2))))
    return out


def _call(lib, fn, block):
    return getattr(lib, fn)(C.byref(block) if block is not None else None, None)


def _refusals(lib, tp, rp):
    """Every refusal: -105 and the full text of the fixture."""
    want = json.load(open(REFUSAL_FIXTURE))
    probes = refusal_probes(tp, rp)
    assert sorted(want) == sorted(p[0] for p in probes)
    for site, fn, block in probes:
        rc = _call(lib, fn, block)
        assert [rc, lib.noahmp_hip_last_error().decode()] == want[site], site
        assert rc == -105 and want[site][1].startswith(fn + ": "), site


def test_refusals_write_nothing():
    """Every refusal site of the two calls gives -105 and its full text (tests/golden/lakes_refusal_text.json) before anything is
    launched or read: the planes here are host memory that the calls must not touch, and they keep their poison."""
    lib = abi.load_library()
    tpl = {k: np.full(64, POISON, F8) for k in TAKE_PLANES}
    rpl = {k: np.full(64, POISON, F8) for k in REL_PLANES}
    _refusals(lib, {k: v.ctypes.data for k, v in tpl.items()}, {k: v.ctypes.data for k, v in rpl.items()})
    assert all((p == POISON).all() for p in list(tpl.values()) + list(rpl.values()))
    text = json.load(open(REFUSAL_FIXTURE))
    for site, word in (("take.nmember.big", "nmember"), ("take.nlake.neg", "nlake"), ("take.ncell.big", "ncell"), ("take.required.inflow", "inflow"),
                       ("take.quantum.three", "power of two"), ("take.inflow.misaligned.4", "aligned"), ("take.alias.storage.member_cell", "share"),
                       ("release.required.weir_l", "required"), ("release.dt.nan", "dt"), ("release.misaligned8.level", "8 bytes"),
                       ("release.misaligned4.diag", "4 bytes"), ("release.same.words", "different"), ("release.alias.out_new.weir_c", "share")):
        assert word in text[site][1], site
    assert len({tuple(v) for v in text.values()}) == 10 + 10


HEADER_LINES = (
    "#define NOAHMP_HIP_HAS_LAKES 1\n", "#define NOAHMP_HIP_ABI_MINOR 3\n", "typedef struct noahmp_lake_take {", "} noahmp_lake_take;",
    "typedef struct noahmp_lake_release {", "} noahmp_lake_release;",
    "int    noahmp_hip_lake_take(const noahmp_lake_take* t, void* stream);",
    "int    noahmp_hip_lake_release(const noahmp_lake_release* r, void* stream);",
    "if (!(s >= (float)q)) skip", "if (!(t < 0x1p62)) skip", "n = (int64)floor(t)", "storage[c] = (float)((double)s - (double)n*q)",
    "v0 = volume[l] + inflow[l];  inflow[l] = 0", "g = 19.6133*ho;  r = sqrt(g)", "if (v0 <= 0) n = 0; else if (n > v0) n = v0",
    "if (n >= 2^24) { sh = bit_length(n) - 24;  n = (n >> sh) << sh }", "volume[l] = v0 - n;  o = (float)((double)n*q)",
    "NOT built: evaporation and precipitation on the lake surface",
)


def test_bindings_carry_the_lake_calls():
    from tools import gen_abi
    for rel, text in (("include/noahmp_hip.h", gen_abi.c_header()), ("noahmp_amd/fortran/module_sf_noahmpdrv_hip.F90", gen_abi.fortran_shim())):
        assert open(os.path.join(ROOT, rel)).read() == text, rel
    hdr = open(HEADER).read()
    for word in HEADER_LINES:
        assert word in hdr, word
    assert "\n".join(gen_abi.lakes_header()) in hdr
    assert "noahmp_lake_take" not in gen_abi.ref_harness() and "noahmp_lake_take" not in gen_abi.shim_wrap()
    f90 = open(os.path.join(ROOT, "noahmp_amd", "fortran", "module_sf_noahmpdrv_hip.F90")).read()
    for word in tuple("bind(C, name='%s')" % c for c in CALLS) + ("type, bind(C) :: noahmp_lake_take ", "type, bind(C) :: noahmp_lake_release "):
        assert word in f90, word
    for sym in CALLS:
        assert sym in abi.EXPORTED_SYMBOLS
    assert [n for n, _ in abi.LakeTake._fields_] == ["member_cell", "member_lake", "nmember", "storage", "inflow", "nlake", "ncell", "quantum"]
    assert [n for n, _ in abi.LakeRelease._fields_] == list(REL_PLANES[:11]) + ["ncell", "level", "outflow", "diag", "nlake", "quantum", "dt"]
    from noahmp_amd.driver import Engine
    from noahmp_amd.parallel import Comm
    from noahmp_amd.routing import Lakes
    for name in ("lake_take_block", "lake_take", "lake_release_block", "lake_release"):
        assert callable(getattr(Engine, name))
    assert callable(Comm.reduce_sum_words) and callable(Lakes.from_fill)


def test_ctypes_mirrors_match_the_compiled_header(tmp_path):
    body, want = "", []
    for cname, cls in (("noahmp_lake_take", abi.LakeTake), ("noahmp_lake_release", abi.LakeRelease)):
        names = [n for n, _ in cls._fields_]
        body += 'printf(" %%zu", sizeof(%s));' % cname + "".join('printf(" %%zu", offsetof(%s, %s));' % (cname, n) for n in names)
        want += [C.sizeof(cls)] + [getattr(cls, n).offset for n in names]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "noahmp_hip.h"\nint main(){' + body +
                   'printf(" %d %d", NOAHMP_HIP_ABI_MINOR, NOAHMP_HIP_HAS_LAKES); return 0;}')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(v) for v in subprocess.check_output([str(exe)]).split()] == want + [3, 1]


def test_library_exports_the_lake_calls():
    if not os.path.exists(abi.LIB_PATH):
        from noahmp_amd import build as b
        b.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", abi.LIB_PATH]).decode()
    for sym in CALLS:
        assert " T %s\n" % sym in out, sym


@pytest.mark.skipif(tr._flang() is None, reason="no flang")
def test_generated_fortran_types_and_interfaces_compile(tmp_path):
    """The lakes part of the generated module compiles, and a caller of the two interfaces type-checks."""
    from tools import gen_abi
    text = "\n".join(["module lakes_abi_check", "  use iso_c_binding", "  implicit none"] + gen_abi.lakes_f90_types() + ["  interface"] +
                     gen_abi.lakes_f90_interfaces() +
                     ["  end interface", "contains", "  function go(planes) result(rc)", "    type(c_ptr), intent(in) :: planes(16)",
                      "    type(noahmp_lake_take) :: t", "    type(noahmp_lake_release) :: r", "    integer(c_int) :: rc",
                      "    t%member_cell = planes(1); t%member_lake = planes(2); t%nmember = 128_c_int64_t; t%storage = planes(3)",
                      "    t%inflow = planes(4); t%nlake = 2; t%ncell = 4096_c_int64_t; t%quantum = 2.0_c_double**(-10)",
                      "    rc = noahmp_hip_lake_take(t, c_null_ptr)",
                      "    r%volume = planes(5); r%inflow = planes(4); r%area = planes(6); r%weir_h = planes(7); r%weir_c = planes(8)",
                      "    r%weir_l = planes(9); r%orifice_h = planes(10); r%orifice_c = planes(11); r%orifice_a = planes(12)",
                      "    r%outlet_cell = planes(13); r%out_new = planes(14); r%ncell = 4096_c_int64_t; r%level = planes(15)",
                      "    r%outflow = planes(16); r%diag = c_null_ptr; r%nlake = 2; r%quantum = 2.0_c_double**(-10); r%dt = 300.0_c_double",
                      "    rc = noahmp_hip_lake_release(r, c_null_ptr)",
                      "  end function go", "end module lakes_abi_check", ""])
    f = tmp_path / "lakes_abi_check.f90"
    f.write_text(text)
    subprocess.check_call([tr._flang(), "-c", str(f), "-o", str(tmp_path / "lakes_abi_check.o"), "-J", str(tmp_path)], cwd=str(tmp_path))


# ---------------------------------------------------------------------------------------------------------------- host helpers
def test_from_fill():
    """A hand-made 12 x 9 terrain with two pits and one pit below min_cells: the labels follow the smallest cell index, the outlet is
    the member with the largest upstream sum, a tie goes to the smallest cell index; area = cells * cell area."""
    from noahmp_amd.routing import Lakes
    ni, nj = 12, 9
    filled = np.full((nj, ni), 100.0, F)
    raw = filled.copy()
    raw[1:3, 7:10] = 98.0                                                # six cells, found first: its smallest cell index is 1*12 + 7
    raw[3, 10] = 98.5                                                    # ... joined diagonally: 8-connected
    raw[5:8, 1:4] = 97.0                                                 # nine cells
    raw[6, 2] = 99.8                                                     # ... with an island shallower than min_depth
    raw[7, 8] = 95.0                                                     # one cell: below min_cells = 2
    raw[0, 0] = 99.6                                                     # too shallow
    up = np.ones((nj, ni), np.uint64)
    up[2, 9], up[3, 10] = 40, 40                                         # a tie: the smaller cell index wins
    up[7, 3] = 2 ** 40
    up[6, 2] = 2 ** 50                                                   # the island is no member
    lake_id, outlet_ij, area = Lakes.from_fill(raw, filled, up, 0.5, min_cells=2, cell_area=250.0)
    want = np.zeros((nj, ni), np.int32)
    want[1:3, 7:10] = 1
    want[3, 10] = 1
    want[5:8, 1:4] = 2
    want[6, 2] = 0
    assert lake_id.dtype == np.int32 and (lake_id == want).all()
    assert outlet_ij.tolist() == [[9, 2], [3, 7]] and area.tolist() == [7 * 250.0, 8 * 250.0]
    lake_id, outlet_ij, area = Lakes.from_fill(raw, filled, up.astype(F8), 0.5, cell_area=1.0)
    assert int(lake_id.max()) == 3 and lake_id[7, 8] == 3 and outlet_ij.tolist() == [[9, 2], [3, 7], [8, 7]] and area.tolist() == [7.0, 8.0, 1.0]
    lake_id, outlet_ij, area = Lakes.from_fill(raw, filled, up, 50.0)
    assert not lake_id.any() and outlet_ij.shape == (0, 2) and area.shape == (0,)
    snake = np.full((9, 40), 10.0)
    deep = snake.copy()
    for j in range(0, 9, 2):
        deep[j, :] = 0.0
    for n, j in enumerate(range(1, 9, 2)):
        deep[j, -1 if n % 2 == 0 else 0] = 0.0                           # one long winding component: many rounds of the labelling
    lake_id, outlet_ij, area = Lakes.from_fill(deep, snake, np.arange(360).reshape(9, 40), 1.0)
    assert int(lake_id.max()) == 1 and int((lake_id == 1).sum()) == 5 * 40 + 4 and outlet_ij.tolist() == [[39, 8]]


def test_set_lakes_raises_on_illegal_outlets():
    """set_lakes raises when an outlet on the tile is no member of its lake and when an outlet's downstream cell is a member of the same
    lake; an outlet without a direction is legal.  (The checks run before anything touches the device: the network here is a stand-in
    with host planes.)"""
    import types
    import torch
    from noahmp_amd.routing import Lakes
    d = np.array([[1, 1, 1, 0], [1, 1, 3, 0], [0, 0, 0, 0]], np.uint8)
    net = types.SimpleNamespace(dir=torch.from_numpy(d), ni=4, nj=3, i0=0, j0=0, block_shape=(3, 4), engine=None, torch=torch, after_launch=[],
                                held=None, release=None, _hold=lambda: None)
    lakes = Lakes.__new__(Lakes)
    lakes.ch, lakes.net, lakes.engine, lakes.torch, lakes.quantum = None, net, None, torch, Q
    lid = np.zeros((3, 4), np.int32)
    lid[0, 0:3] = 1
    with pytest.raises(ValueError, match="not a member"):
        lakes.set_lakes(lid, lake_params(1), [(3, 0)])
    with pytest.raises(ValueError, match="same lake"):
        lakes.set_lakes(lid, lake_params(1), [(1, 0)])
    with pytest.raises(ValueError, match="one entry per lake"):
        lakes.set_lakes(lid, lake_params(2), [(2, 0)])
    with pytest.raises(ValueError, match="power of two"):
        Lakes(net, quantum=3.0)


# ---------------------------------------------------------------------------------------------------------------- GPU
_dev = tr._dev
PAD = 3                                                                  # words in front of and behind a plane inside its poisoned pool


def _guarded(a, poison):
    """A device copy of `a` at an odd offset inside a poisoned pool: (pool, view)."""
    import torch
    a = np.ascontiguousarray(a)
    pool = torch.full((a.size + 2 * PAD,), poison, dtype=torch.from_numpy(a.reshape(-1)[:0].copy()).dtype, device="cuda")
    view = pool[PAD:PAD + a.size]
    if a.size:
        view.copy_(_dev(a.reshape(-1)))
    return pool, view


def _guards(pool, poison):
    h = pool.cpu().numpy()
    return bool((h[:PAD] == poison).all() and (h[h.size - PAD:] == poison).all())


@pytest.fixture(scope="module")
def engine_per_lane(tables):
    """The variant library: every lane of noahmp_hip_lake_take sends its own atomic."""
    from noahmp_amd.driver import Engine
    build_variant()                                                      # nothing to do where __graft_entry__.build() has run
    if not os.path.exists(LIB_PER_LANE):
        pytest.fail("%s missing: __graft_entry__.build() compiles it (-DNMP_LAKES_PER_LANE=1)" % LIB_PER_LANE)
    return Engine(tables[0], lib_path=LIB_PER_LANE)


@pytest.mark.gpu
@pytest.mark.parametrize("ni, nj", WINDOWS)
@pytest.mark.parametrize("form", ["reduced", "per lane"])
def test_gpu_take_equals_the_restatement(engine, engine_per_lane, form, ni, nj):
    """noahmp_hip_lake_take against np_lake_take in every word of storage and inflow, the cases of the host test: sorted and padded
    lists (uniform waves: the butterfly and the LDS path), shuffled lists (mixed waves: per-lane atomics), lists with -1 and out-of-range
    entries, the empty list and no lakes; both forms of the kernel.  storage and inflow sit at an odd offset inside poisoned pools whose
    guard words keep the poison."""
    import torch
    eng = engine if form == "reduced" else engine_per_lane
    for what, mc, ml, s, inf, q, want in take_cases(ni, nj):
        spool, sd = _guarded(s, POISON)
        ipool, idev = _guarded(np.concatenate([inf, np.zeros(1, I64)]), -77)      # 8-byte words: any offset is aligned; one spare word
        idev = idev[:inf.size]
        torch.cuda.synchronize()
        eng.lake_take(eng.lake_take_block(_dev(mc), _dev(ml), sd, idev, q))
        eng.stream_sync()
        same_words(sd.cpu().numpy().reshape(nj, ni), want[0], what + ": storage")
        same_words(idev.cpu().numpy(), want[1], what + ": inflow")
        assert _guards(spool, POISON) and _guards(ipool, -77) and int(ipool[PAD + inf.size].item()) == 0, what + ": guard words"


@pytest.mark.gpu
@pytest.mark.parametrize("ni, nj", WINDOWS)
def test_gpu_release_equals_the_restatement(engine, ni, nj):
    """noahmp_hip_lake_release against np_lake_release in every word of volume, inflow, out_new, level, outflow and diag, the cases of
    the host test (diag starts at 3: the call accumulates and never zeroes); the guard words keep the poison, and what is not given
    is not written."""
    import torch
    for what, par, vol, inf, oc, plane, lev, ofl, dg, q, dt, want in release_cases(ni, nj):
        nl = vol.size
        pools = dict(vol=_guarded(vol, -77), inf=_guarded(inf, -77), out=_guarded(plane, POISON), lev=_guarded(lev if lev is not None else np.zeros(nl, F8), POISON),
                     ofl=_guarded(ofl if ofl is not None else np.full(nl, POISON, F), POISON),
                     dg=_guarded((dg if dg is not None else np.array([3], U32)).view(np.int32), 77))
        pd = {k: _dev(par[k]) for k in PARAMS}
        torch.cuda.synchronize()
        b = engine.lake_release_block(pools["vol"][1], pools["inf"][1], pd, _dev(oc), pools["out"][1], q, dt, level=pools["lev"][1] if lev is not None else None,
                                      outflow=pools["ofl"][1] if ofl is not None else None, diag=pools["dg"][1] if dg is not None else None)
        engine.lake_release(b)
        engine.stream_sync()
        host = {k: v[1].cpu().numpy() for k, v in pools.items()}
        got = (host["vol"], host["inf"], host["out"].reshape(nj, ni), host["lev"] if lev is not None else None, host["ofl"] if ofl is not None else None,
               host["dg"].view(U32) if dg is not None else None)
        assert_release(got, want, what)
        for k, poison in (("vol", -77), ("inf", -77), ("out", POISON), ("lev", POISON), ("ofl", POISON), ("dg", 77)):
            assert _guards(pools[k][0], poison), what + ": guard words of " + k
        assert lev is not None or (host["lev"] == 0).all()
        assert ofl is not None or (host["ofl"] == POISON).all()
        assert dg is not None or int(host["dg"][0]) == 3


def _two_lakes(kinematic):
    """The whole 70 x 130 domain with two lakes: the 6 x 6 lake at the centre and the pit lake that drains out of the network."""
    w, parts = whole_and_parts(kinematic)
    ni, nj = w["ni"], w["nj"]
    _, pit_cells, pit_outlet = hills_lake(ni, nj, w["z"])
    assert not set(pit_cells.tolist()) & set(w["cells"].tolist())
    lake_id = np.zeros((nj, ni), np.int32)
    lake_id.reshape(-1)[w["cells"]] = 1
    lake_id.reshape(-1)[pit_cells] = 2
    par = lake_params(2, area=[w["cells"].size * DX * DY, pit_cells.size * DX * DY], weir_h=[0.001, 0.0005], weir_l=[20.0, 5.0],
                      orifice_h=[0.0, NEVER], orifice_a=[0.5, 0.0])
    outlets = [w["outlet"], pit_outlet]
    w.update(lake_id=lake_id, par2=par, members=[w["cells"], pit_cells], outlets=outlets,
             outlet_ij=[(c % ni, c // ni) for c in outlets])
    return w, parts


def _restated_steps(w, kinematic, nstep, nsub, dt, length=None, conv=None, record=None):
    """nstep steps of nsub calls through the restatements; record receives per call (out plane, inflow words after the take)."""
    x = dict(w["x"], scale=float(F(dt) * F(1e-3)) / nsub)
    if kinematic:
        x.update(length=length, conv=conv, dt=dt / nsub)
    run = LakeRun(x, kinematic, w["members"], w["par2"], w["outlets"], w["ops"]["storage"], w["ops"]["out"])
    for _ in range(nstep * nsub):
        run.route_call()
        run.take_call()
        words = run.inf.copy()
        run.release_call(dt / nsub)
        if record is not None:
            record.append((run.out[run.cur].copy(), words))
    return run


def _store(ops, ni, nj, tile=None, perm=None):
    import types
    ra, rb = ops["runoff_a"].reshape(nj, ni), ops["runoff_b"].reshape(nj, ni)
    if tile is not None:
        ra, rb = ra[tile], rb[tile]
    tnj, tni = ra.shape
    ra, rb = ra.reshape(-1), rb.reshape(-1)
    kw = {}
    if perm is not None:
        ra, rb = ra[perm], rb[perm]
        kw["sort_perm"] = _dev(perm.astype(np.int32))
    return types.SimpleNamespace(ni=tni, nj=tnj, a=dict(runsfxy=_dev(ra), runsbxy=_dev(rb)), **kw)


def _flow(engine, w, kinematic, z_win, origin, blk, lake_tile, tile_origin, manning=None, late=False):
    """A FlowNetwork (and ChannelFlow) of a tile with its Lakes attached; late: the planes are set again AFTER set_lakes."""
    from noahmp_amd.routing import ChannelFlow, FlowNetwork, Lakes
    ops = w["ops"]
    nj_t, ni_t = lake_tile.shape
    net = FlowNetwork(engine, ni_t, nj_t)
    net.set_terrain(_dev(z_win), DX, DY, origin=origin)
    net.set_area(_dev(ops["area"][blk]))
    net.set_input_columns(None)
    net.storage.copy_(_dev(ops["storage"][blk]))
    for o in net.out:
        o.copy_(_dev(ops["out"][blk]))
    ch = None
    if kinematic:
        ch = ChannelFlow(net)
        ch.set_geometry(_dev(ops["width"][blk]), _dev(manning[blk]), smin=tc.SMIN, height=_dev(z_win))
    else:
        net.set_release(_dev(ops["release"][blk]))
    lakes = Lakes(ch if kinematic else net)
    lakes.set_lakes(lake_tile, w["par2"], w["outlet_ij"], tile_origin=tile_origin)
    if late:
        if kinematic:
            ch.set_geometry(_dev(ops["width"][blk]), _dev(manning[blk]), smin=tc.SMIN, height=_dev(z_win))
        else:
            net.set_release(_dev(ops["release"][blk]))
            net.set_velocity(0.5, 600.0)
            assert float(net.release[net.held].abs().max().item()) == 0.0
            net.set_release(_dev(ops["release"][blk]))
    held = net.held
    assert int(held.sum().item()) == int((lake_tile > 0).sum())
    assert float((ch.conv if kinematic else net.release)[held].abs().max().item()) == 0.0, "the members hold their water"
    lakes.attach()
    lakes.attach()
    assert len(net.after_launch) == 1
    return net, ch, lakes


def _channel_planes(w):
    ni, nj = w["ni"], w["nj"]
    n = np.random.default_rng(8).uniform(0.03, 0.08, (nj, ni)).astype(F)
    length, conv, _ = tc.np_flow_channel(w["d"], n, DX, DY, tc.SMIN, height=w["z"])
    return n, length, conv


@pytest.mark.gpu
@pytest.mark.parametrize("kinematic", [False, True])
def test_gpu_lakes_on_the_steps(engine, kinematic):
    """Lakes attached to FlowNetwork.step and to ChannelFlow.step on the 70 x 130 hills with two lakes (one drains out of the network),
    10 steps with nsub = 2, set_release / set_velocity / set_geometry called again after set_lakes: storage, out, volume, level, outflow
    and the emptied count have 0 differing words against the restatement.  The list is sorted by lake and padded to whole waves.  A
    permuted col_index (follow) changes no word.  After detach() the words stay as they are."""
    import torch
    w, _ = _two_lakes(kinematic)
    ni, nj, ops = w["ni"], w["nj"], w["ops"]
    nstep, nsub, dt = 10, 2, 2 * tc.DT
    n = length = conv = None
    if kinematic:
        n, length, conv = _channel_planes(w)
    run = _restated_steps(w, kinematic, nstep, nsub, dt, length, conv)
    whole = (slice(None), slice(None))
    perm = np.random.default_rng(5).permutation(ni * nj)
    for name, p in (("identity", None), ("followed", perm)):
        net, ch, lakes = _flow(engine, w, kinematic, w["z"], (0, 0), whole, w["lake_id"], (0, 0), manning=n, late=True)
        mc, ml = lakes.member_cell.cpu().numpy(), lakes.member_lake.cpu().numpy()
        assert mc.size == 64 + 64 and (ml[:64][mc[:64] >= 0] == 0).all() and (ml[64:][mc[64:] >= 0] == 1).all() and (mc[36:64] == -1).all()
        assert sorted(mc[mc >= 0].tolist()) == sorted(w["members"][0].tolist() + w["members"][1].tolist())
        store = _store(ops, ni, nj, perm=p)
        if p is not None:
            (ch or net).follow(store)
        torch.cuda.synchronize()
        step = ch.step if kinematic else net.step
        for _ in range(nstep):
            step(store, dt, nsub=nsub)
        engine.stream_sync()
        same_words(net.storage.cpu().numpy(), run.S, name + ": storage")
        same_words(net.out[net.cur].cpu().numpy(), run.out[run.cur], name + ": out")
        same_words(lakes.volume.cpu().numpy(), run.vol, name + ": volume")
        same_words(lakes.level().cpu().numpy(), run.level, name + ": level")
        same_words(lakes.outflow().cpu().numpy(), run.outflow, name + ": outflow")
        assert lakes.emptied() == int(run.diag[0]) and (lakes.inflow.cpu().numpy() == 0).all()
        same_words(lakes.volume_m3(), run.vol.astype(F8) * Q, name + ": volume_m3")
    assert (run.vol > 0).all() and (run.outflow > 0).all()
    lakes.detach()
    assert net.after_launch == []
    before = lakes.volume.clone()
    step(store, dt, nsub=nsub)
    engine.stream_sync()
    assert torch.equal(lakes.volume, before) and float(net.storage[net.held].max().item()) >= Q, "detached: the members hold what reaches them"


class _PartsComm:
    """A stand-in for Comm in one process, in the manner of test_channel._RingFromOwners: exchange_halo copies the ring of out from the
    whole-domain plane of the same call; reduce_sum_words returns the whole-domain inflow words of the same call, both recorded from
    the restatement, and keeps this part's own partial words."""

    def __init__(self, record, blk, ring, partial):
        self.record, self.blk, self.ring, self.partial, self.calls, self.sums = record, blk, ring, partial, 0, 0

    def exchange_halo(self, planes, geom):
        import torch
        assert len(planes) == 1 and geom == "geom"
        planes[0].copy_(torch.where(self.ring, _dev(self.record[self.calls][0][self.blk]), planes[0]))
        self.calls += 1

    def reduce_sum_words(self, words):
        assert self.sums == self.calls, "take, sum, release, then the exchange"
        self.partial[self.sums] = self.partial[self.sums] + words.cpu().numpy()
        self.sums += 1
        return _dev(self.record[self.sums - 1][1])


@pytest.mark.gpu
@pytest.mark.parametrize("kinematic", [False, True])
def test_gpu_decomposition(engine, kinematic):
    """The four parts of 70 x 130 through Lakes with a stand-in comm, ten steps = 20 calls: storage, out (ring included) and volume have
    0 differing words against the whole-domain restatement, and the parts' own partial inflow words add up to the whole's in every
    call.  The centre lake has members on all four parts; every rank makes the same release, one owns the outlet."""
    import torch
    w, _ = _two_lakes(kinematic)
    ni, nj, ops = w["ni"], w["nj"], w["ops"]
    nstep, nsub, dt = 10, 2, 2 * tc.DT
    n = length = conv = None
    if kinematic:
        n, length, conv = _channel_planes(w)
    record = []
    run = _restated_steps(w, kinematic, nstep, nsub, dt, length, conv, record)
    partial = [np.zeros(2, I64) for _ in record]
    owners = 0
    for (tile, win, idx), (_, blk, bidx) in zip(tsh._cuts(ni, nj, 2), tsh._cuts(ni, nj, 1)):
        tj, ti = tile
        net, ch, lakes = _flow(engine, w, kinematic, w["z"][win], (ti.start - win[1].start, tj.start - win[0].start), blk, w["lake_id"][tile],
                               (ti.start, tj.start), manning=n)
        oc = lakes.outlet_cell.cpu().numpy()
        owners += int((oc >= 0).sum())
        assert int((lakes.member_cell >= 0).sum().item()) == int((w["lake_id"][tile] > 0).sum()) > 0
        comm = _PartsComm(record, blk, _dev(bidx < 0), partial)
        store = _store(ops, ni, nj, tile=tile)
        torch.cuda.synchronize()
        step = ch.step if kinematic else net.step
        for _ in range(nstep):
            step(store, dt, nsub=nsub, comm=comm, geom="geom")
        engine.stream_sync()
        torch.cuda.synchronize()
        assert comm.calls == comm.sums == nstep * nsub
        same_words(net.tile_view(net.storage).cpu().numpy(), run.S[tile], "part %s: storage" % (tile,))
        same_words(net.out[net.cur].cpu().numpy(), run.out[run.cur][blk], "part %s: out, ring included" % (tile,))
        same_words(lakes.volume.cpu().numpy(), run.vol, "part %s: volume" % (tile,))
        same_words(lakes.outflow().cpu().numpy(), run.outflow, "part %s: outflow" % (tile,))
    assert owners == 2
    for got, (_, want) in zip(partial, record):
        same_words(got, want, "the parts' partial inflow words")
    assert (run.vol > 0).all()


@pytest.mark.gpu
def test_gpu_refusals_launch_nothing(engine):
    """The refusals with device planes: -105, the full texts of the fixture, and every plane keeps its poison.  Counts of 0 return 0
    and write nothing."""
    import torch
    fl = torch.full((len(TAKE_PLANES) + len(REL_PLANES), 64), POISON, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    tp = {k: fl[n].data_ptr() for n, k in enumerate(TAKE_PLANES)}
    rp = {k: fl[len(TAKE_PLANES) + n].data_ptr() for n, k in enumerate(REL_PLANES)}
    _refusals(engine.lib, tp, rp)
    for kw in (dict(nmember=0), dict(nlake=0), dict(ncell=0)):
        assert _call(engine.lib, CALLS[0], _take_block(tp, **kw)) == 0
    assert _call(engine.lib, CALLS[1], _rel_block(rp, nlake=0)) == 0
    engine.stream_sync()
    torch.cuda.synchronize()
    assert (fl.cpu().numpy() == POISON).all()


@pytest.mark.gpu
def test_gpu_state_dict_round_trip(engine):
    """state_dict / load_state_dict carry the volume words: a run continued from the restart state (the network's and the lakes') equals
    the uninterrupted one in every word; set_volume_m3 sets floor(v / q) words; another quantum is refused."""
    import torch
    w, _ = _two_lakes(False)
    ni, nj, ops = w["ni"], w["nj"], w["ops"]
    dt = 2 * tc.DT
    whole = (slice(None), slice(None))
    store = _store(ops, ni, nj)
    net, _, lakes = _flow(engine, w, False, w["z"], (0, 0), whole, w["lake_id"], (0, 0))
    torch.cuda.synchronize()
    for _ in range(3):
        net.step(store, dt, nsub=2)
    lstate = lakes.state_dict()                                          # waits for the launches; FlowNetwork.state_dict leaves that to the caller
    state = net.state_dict()
    assert lstate["volume"].dtype == torch.int64 and int(lstate["volume"].min().item()) > 0
    for _ in range(3):
        net.step(store, dt, nsub=2)
    engine.stream_sync()
    want = (net.storage.cpu().numpy(), net.out[net.cur].cpu().numpy(), lakes.volume.cpu().numpy())
    net2, _, lakes2 = _flow(engine, w, False, w["z"], (0, 0), whole, w["lake_id"], (0, 0))
    net2.load_state_dict(state)
    lakes2.load_state_dict(lstate)
    for _ in range(3):
        net2.step(store, dt, nsub=2)
    engine.stream_sync()
    for g, x, nm in zip((net2.storage.cpu().numpy(), net2.out[net2.cur].cpu().numpy(), lakes2.volume.cpu().numpy()), want, ("storage", "out", "volume")):
        same_words(g, x, "continued from the restart state: " + nm)
    lakes2.set_volume_m3([1234.5678, 0.0])
    assert lakes2.volume.cpu().numpy().tolist() == [int(math.floor(1234.5678 / Q)), 0] and lakes2.volume_m3()[0] == math.floor(1234.5678 / Q) * Q
    with pytest.raises(ValueError, match="quantum"):
        lakes2.load_state_dict(dict(lstate, quantum=2 * Q))


DAM_SHARE = 0.2                                                          # of the undammed peak: the release per call of a lake that holds the whole flood
VALLEY_STEPS = 60                                                     # routing-only steps after the three engine steps


def _valley_run(engine, tables, dam):
    """Three engine steps of the 35 x 67 mixed tile at a rainy hour in the valley terrain, each followed by ChannelFlow.step(nsub=2), then
    VALLEY_STEPS steps of routing alone with the runoff planes zeroed.  dam: None, or a function (net, ch) -> Lakes called before the
    first step.  Returns per CALL the release of every cell of the block (numpy), and (net, ch, lakes)."""
    import torch
    from noahmp_amd import synth
    from noahmp_amd.routing import ChannelFlow, FlowNetwork
    T, tb = tables
    s = synth.mixed_small(tb, ni=trt.ENG_NI, nj=trt.ENG_NJ)
    synth.first_step_fixups(s)
    synth.diurnal_forcing(s, 11, t_offset=s.t_offset)
    d = s.to_device("cuda:0")
    torch.cuda.synchronize()
    height = tsv._valley()
    net = FlowNetwork(engine, trt.ENG_NI, trt.ENG_NJ)
    net.set_terrain(_dev(height), DX, DX, origin=(trt.ENG_MARGIN, 0))
    ch = ChannelFlow(net)
    ch.set_geometry(20.0, 0.05, height=_dev(height))
    lakes = dam(net, ch) if dam is not None else None
    series = []

    def grab(out_new, dt_sub, comm, stream):                              # after the lakes' hook: what every cell released in this call
        engine.stream_sync(stream)
        series.append(out_new.cpu().numpy().copy())

    net.after_launch.append(grab)
    for it in range(1, trt.ENG_STEPS + 1 + VALLEY_STEPS):
        if it <= trt.ENG_STEPS:
            st = engine.noahmplsm(d, it, 2000, 180.0)
            assert st.code == 0
        elif it == trt.ENG_STEPS + 1:
            d.a["runsfxy"].zero_()
            d.a["runsbxy"].zero_()
            torch.cuda.synchronize()
        ch.step(d, d.cfg.dt, nsub=2)
    engine.stream_sync()
    return np.stack(series), d.cfg.dt / 2, net, ch, lakes


@pytest.mark.gpu
def test_gpu_engine_run_in_a_valley_with_a_dam(engine, tables):
    """An engine run in the valley terrain, as test_channel's, with a dam: the gauge below the lake sees a lower, later peak than the
    same run without the lake, and the water is all accounted for.
    The run without the lake comes first and sizes the dam from what it saw at the outlet cell: Qp the largest release per call and W
    the sum of all releases plus what the member cells still hold at the end, which is all the water that entered the member cells (the
    kinematic wave has no backwater: upstream of the lake both runs are the same).  The lake is a reservoir of ONE cell, the outlet
    cell behind the dam: it gets the cell's area A and a weir with c*l = DAM_SHARE Qp / (dt (W/A)^(3/2)), DAM_SHARE = 0.2: holding ALL the
    water of the flood it would release 0.2 Qp per call, so its peak lies below 0.2 Qp whatever the timing, and the explicit step is
    stable (its slope is at most 0.3 Qp/W < 1 per call).  A level pool peaks where inflow = outflow, on the falling limb of its inflow:
    while the inflow exceeds 0.2 Qp the volume still grows.  (A lake of several cells along the stem also SAVES the calls the flood needs
    to cross them, one per cell where the cells are capped as in this steep valley, and the flood here lasts only about five calls: with
    three members and this weir the release at the dam peaked two calls after the undammed cell's, but the gauge, which also collects
    two hillslopes of its own, showed its peak in the same call.  Lakes of many cells are what the other tests run.)  The gauge is the
    cell below the outlet; what reaches it from its own hillslopes is the same in both runs.  (The issue words the comparison as 'the
    same run with detach()'; detached members still hold their water, so the run compared with is the one without set_lakes, and
    detach() is covered by test_gpu_lakes_on_the_steps.)"""
    from noahmp_amd.routing import Lakes
    plain, dts, net, ch, _ = _valley_run(engine, tables, None)
    d = net.dir.cpu().numpy()
    njb, nib = d.shape
    acc = net.upstream_cells().cpu().numpy().view(U32).astype(I64)
    tile = np.zeros(d.shape, bool)
    tile[net.j0:net.j0 + net.nj, net.i0 + 2:net.i0 + net.ni - 2] = True

    def down(j, i):
        k = int(d[j, i])
        return (j + trt.DJ[k - 1], i + trt.DI[k - 1]) if k else None

    cand = []
    for j, i in np.argwhere(tile & (d > 0)):
        g = down(j, i)
        if g is not None and 0 <= g[0] < njb and tile[g] and d[g] > 0 and plain[:, j, i].max() > 0:
            cand.append((int(acc[j, i]), -int(j), -int(i)))
    assert cand, "a channel cell with a downstream cell on the tile"
    _, mj, mi = max(cand)
    oj, oi = -mj, -mi
    gauge = down(oj, oi)
    at_outlet = plain[:, oj, oi].astype(F8)
    still = float(net.storage[oj, oi].item())                            # what has entered the cell and not yet left it
    qp, wsum = float(at_outlet.max()), float(at_outlet.sum()) + still
    assert qp > 0 and int(np.argmax(plain[:, gauge[0], gauge[1]])) < plain.shape[0] - 10, "the flood has passed the gauge before the run ends"
    area = DX * DX
    cl = DAM_SHARE * qp / (dts * (wsum / area) ** 1.5)

    def dam(net2, ch2):
        lake_id = np.zeros((net2.nj, net2.ni), np.int32)
        lake_id[oj - net2.j0, oi - net2.i0] = 1
        lakes = Lakes(ch2)
        lakes.set_lakes(lake_id, lake_params(1, area=area, weir_h=0.0, weir_c=cl, weir_l=1.0), [(oi - net2.i0, oj - net2.j0)])
        lakes.attach()
        return lakes

    dammed, _, net2, ch2, lakes = _valley_run(engine, tables, dam)
    g_plain, g_dam = plain[:, gauge[0], gauge[1]].astype(F8), dammed[:, gauge[0], gauge[1]].astype(F8)
    print("gauge %s below the outlet %s: peak %.6g m3 per call at call %d without the lake, %.6g at call %d with it; Qp %.6g, W %.6g, c*l %.4g"
          % (gauge, (oj, oi), g_plain.max(), int(np.argmax(g_plain)), g_dam.max(), int(np.argmax(g_dam)), qp, wsum, cl))
    assert g_dam.max() < g_plain.max() and int(np.argmax(g_dam)) > int(np.argmax(g_plain))
    assert dammed[:, oj, oi].max() <= DAM_SHARE * qp * (1 + 2.0 ** -16), "the bound the dam was sized for (2^-16: the float32 roundings of 126 routing calls)"
    assert int(np.argmax(dammed[:, oj, oi])) > int(np.argmax(at_outlet)), "at the dam itself"
    held = lakes.volume_m3()[0] + float(net2.storage[net2.held].double().sum().item())
    released = float(dammed[:, oj, oi].astype(F8).sum())
    assert held >= 0 and released > 0.05 * wsum and released + held <= wsum * (1 + 2.0 ** -16)
