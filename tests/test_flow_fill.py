"""Depression filling and flat resolution for the D8 network on the device (noahmp_hip_flow_fill_init, noahmp_hip_flow_fill;
nmp_dev_flow_fill.hpp; DepressionFill, FlowNetwork.set_terrain(fill=...), FlowNetwork.set_terrain_filled).

No reference routine stands behind the calls; the contract is the text in include/noahmp_hip.h.  np_fill_init and np_fill_pass restate it in
numpy, one rounded float32 operation per line; np_fill_fixed_point iterates the pass to the surface W*, and priority_flood makes the same
surface by an independent method (a heap, Barnes et al. 2014).  W* is unique and every order of updates reaches it, so everything is
compared bit for bit (test_regrid.assert_same): init and the pinned pass per call, the tiled kernel at its fixed point and, per call, by
the five invariants the header text pins it with.  No tolerance appears anywhere."""
import ctypes as C
import functools
import heapq
import os
import re
import subprocess

import numpy as np
import pytest

from noahmp_amd import abi
import test_regrid as tr
import test_routing as trt
import test_shadow as tsh
from test_regrid import F, assert_same, nasty
from test_routing import DX, DY, assert_same_bytes, neighbour, np_flow_dir, np_inmask

ROOT = tr.ROOT
CSRC = tr.CSRC
SRC = os.path.join(ROOT, "tests", "host_emul", "flow_fill_check.hip")
LIB = os.path.join(ROOT, "tests", "host_emul", "libflow_fill_check.so")
HEADER = os.path.join(ROOT, "include", "noahmp_hip.h")
U32 = np.uint32
INF = F(np.inf)
POISON = 7.0
EPS = F(1e-3)


def header_macro(name):
    m = re.search(r"^#define %s\s+(-?\d+)" % name, open(HEADER).read(), re.M)
    assert m, "%s is not in include/noahmp_hip.h" % name
    return int(m.group(1))


def _macro_or(name, default):
    try:
        return header_macro(name)
    except AssertionError:                                               # collection must not fail on a tree without the feature; the tests do
        return default


TI, TJ = _macro_or("NOAHMP_FLOW_FILL_TILE_I", 64), _macro_or("NOAHMP_FLOW_FILL_TILE_J", 32)
CAP = _macro_or("NOAHMP_FLOW_FILL_MAX_SWEEPS", 1024)
CUT = (70, 130)
# (ni, nj): a lone cell, one row, one column, the 64 / 65 lane boundary, exactly one tile and one cell more and less in each direction, 2 x 5 tiles
WINDOWS = [(1, 1), (7, 1), (1, 7), (3, 3), (65, 5), (67, 35), (TI, TJ), (TI + 1, TJ), (TI - 1, TJ), (TI, TJ + 1), (TI, TJ - 1), CUT]
SWEEPS = (2, 7, 64, CAP)
OUTLET = dict(w=1, e=2, s=4, n=8)
RING = dict(w=16, e=32, s=64, n=128)
ALL_OUTLET = 15


def side_flags(outlet_sides="wesn", ring_sides=""):
    return sum(OUTLET[s] for s in outlet_sides) | sum(RING[s] for s in ring_sides)


# ---------------------------------------------------------------------------------------------------------------- the restatement
def np_up(m):
    """The smallest float32 greater than m, on the bits: NaN -> m, +inf -> +inf, +-0 -> bits 1, b - 1 for a negative m, b + 1 for a positive."""
    m = np.asarray(m, F)
    shape = m.shape
    b = np.atleast_1d(m).view(U32)
    mag = b & U32(0x7FFFFFFF)
    step = np.where((b & U32(0x80000000)) != 0, b - U32(1), b + U32(1)).astype(U32)
    out = np.where(mag == 0, U32(1), step).astype(U32)
    out = np.where((mag > U32(0x7F800000)) | (b == U32(0x7F800000)), b, out).astype(U32)
    return out.view(F).reshape(shape)


def np_lift(m, eps):
    with np.errstate(all="ignore"):
        a = (np.asarray(m, F) + F(eps)).astype(F)
        u = np_up(m)
        return np.where(u > a, u, a).astype(F)                           # max(a, up(m)) = (up > a) ? up : a


def np_fill_init(z, outlet=None, flags=ALL_OUTLET):
    """(fixed, w_old) of noahmp_hip_flow_fill_init."""
    nj, ni = z.shape
    jj, ii = np.meshgrid(np.arange(nj), np.arange(ni), indexing="ij")
    side = (ii == 0) * 1 | (ii == ni - 1) * 2 | (jj == 0) * 4 | (jj == nj - 1) * 8
    ring = (side & (flags >> 4)) != 0
    out = np.isnan(z) | ((side & flags & 15) != 0)
    if outlet is not None:
        out = out | (outlet != 0)
    for k in range(1, 9):
        v, inside = neighbour(np.isnan(z), k, False)
        out = out | (inside & v)
    fixed = np.where(ring, 2, np.where(out, 1, 0)).astype(np.uint8)
    w = np.where(fixed == 1, z, INF).astype(F)
    return fixed, w


def np_neighbour_min(w):
    m = np.full(w.shape, INF, F)
    with np.errstate(all="ignore"):
        for k in range(1, 9):
            v, inside = neighbour(w, k, INF)
            m = np.where(inside & (v < m), v, m).astype(F)               # min(m, v) = (v < m) ? v : m: a NaN never wins
    return m


def np_fill_pass(z, fixed, w_old, eps):
    """One pinned call: (w_new, changed)."""
    with np.errstate(all="ignore"):
        m = np_neighbour_min(w_old)
        a = (m + F(eps)).astype(F)
        u = np_up(m)
        l = np.where(u > a, u, a).astype(F)
        cand = np.where(l > z, l, z).astype(F)
        wn = np.where(cand < w_old, cand, w_old).astype(F)
    wn = np.where(fixed != 0, w_old, wn).astype(F)
    return wn, int((wn.view(U32) != w_old.view(U32)).any())


def np_fill_fixed_point(z, fixed, w0, eps, max_pass=None):
    """The pass iterated until it changes nothing: (W*, passes made, the last one included)."""
    max_pass = int((fixed == 0).sum()) + 1 if max_pass is None else max_pass
    w = w0
    for n in range(1, max_pass + 1):
        w, changed = np_fill_pass(z, fixed, w, eps)
        if not changed:
            return w, n
    raise AssertionError("the Jacobi iteration needs more than free cells + 1 passes")


def priority_flood(z, fixed, w0, eps):
    """Priority-flood + epsilon with a heap, an independent method: pop the lowest known cell, give every neighbour not yet known
    max(z, lift(w of the popped cell)).  Cells no outlet reaches keep +inf.  Scalar float32 arithmetic through the same np_lift."""
    nj, ni = z.shape
    w = np.where(fixed != 0, w0, INF).astype(F)
    known = fixed != 0
    heap = [(float(w[j, i]), j, i) for j, i in zip(*np.nonzero(known)) if not np.isnan(w[j, i])]
    heapq.heapify(heap)
    while heap:
        v, j, i = heapq.heappop(heap)
        l = np_lift(F(v), eps)[()]
        for k in range(8):
            jn, i_n = j + trt.DJ[k], i + trt.DI[k]
            if 0 <= jn < nj and 0 <= i_n < ni and not known[jn, i_n]:
                known[jn, i_n] = True
                w[jn, i_n] = l if l > z[jn, i_n] else z[jn, i_n]
                heapq.heappush(heap, (float(w[jn, i_n]), jn, i_n))
    return w


# ---------------------------------------------------------------------------------------------------------------- terrains
def serpentine(ni, nj):
    """Walls of 1000 m on every odd column of a plain at 0, open at the top (i % 4 == 1) or at the bottom (i % 4 == 3): one corridor
    of about ni/2 * nj cells that crosses the rows j = TILE_J, 2 TILE_J, ... in every leg and the columns i = TILE_I, ... once each.  All
    four sides are closed walls; the only outlet is the caller's, at cell (0, 0)."""
    z = np.zeros((nj, ni), F)
    for i in range(1, ni, 2):
        z[:, i] = 1000.0
        z[nj - 1 if i % 4 == 1 else 0, i] = 0.0
    outlet = np.zeros((nj, ni), np.uint8)
    outlet[0, 0] = 1
    return z, outlet


@functools.lru_cache(maxsize=None)
def cases(ni, nj):
    """[(name, height, eps, outlet plane or None, flags)]; the planes are read-only and shared."""
    r = np.random.default_rng(9000 + 17 * ni + nj)
    hills = tsh.terrain(ni, nj, (ni, nj) == CUT)
    out = [("hills", hills, EPS, None, ALL_OUTLET)]
    out.append(("hills rounded to 10 m", (np.round(hills / F(10.0)) * F(10.0)).astype(F), EPS, None, ALL_OUTLET))
    plain = np.zeros((nj, ni), F)
    if ni >= 5 and nj >= 5:
        plain[nj // 3:2 * nj // 3 + 1, ni // 3:2 * ni // 3 + 1] = -50.0
    out.append(("plain at 0 with a basin", plain, EPS, None, ALL_OUTLET))
    out.append(("hills + 2000 m, eps 1e-6", (hills + F(2000.0)).astype(F), F(1e-6), None, ALL_OUTLET))
    metres = np.floor(hills).astype(F)
    metres[r.random((nj, ni)) < 0.02] = np.nan
    if ni >= 7 and nj >= 7:
        metres[nj // 2 - 1:nj // 2 + 2, ni // 2 - 2:ni // 2 + 2] = np.nan      # a lake
    out.append(("integer metres with NaN cells", metres, EPS, None, ALL_OUTLET))
    out.append(("nasty", nasty(r, ni * nj).reshape(nj, ni), EPS, None, ALL_OUTLET))
    o = np.zeros((nj, ni), np.uint8)
    o[nj // 2, ni // 2] = 3
    out.append(("a caller outlet, E and N closed", (np.round(hills / F(10.0)) * F(10.0)).astype(F), EPS, o, side_flags("ws")))
    z, o = serpentine(ni, nj)
    out.append(("serpentine", z, EPS, o, 0))
    for c in out:
        for a in c[1:4:2]:
            if a is not None:
                a.setflags(write=False)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def solved(ni, nj):
    """{name: (fixed, w0, W*, passes)} of cases(ni, nj): made once, shared by every test, never written."""
    out = {}
    for name, z, eps, outlet, flags in cases(ni, nj):
        fixed, w0 = np_fill_init(z, outlet, flags)
        ws, passes = np_fill_fixed_point(z, fixed, w0, eps)
        for a in (fixed, w0, ws):
            a.setflags(write=False)
        out[name] = (fixed, w0, ws, passes)
    return out


# ---------------------------------------------------------------------------------------------------------------- CPU
def build():
    """The host checker: nmp_dev_flow_fill.hpp compiled for the CPU.  Needs nothing of the engine library."""
    deps = [SRC, os.path.join(CSRC, "nmp_dev_flow_fill.hpp"), os.path.join(CSRC, "nmp_dev_routing.hpp"), HEADER]
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
    lib.fill_up_values.argtypes = [I, V, V]
    lib.fill_lift_values.argtypes = [I, V, Fl, V]
    lib.fill_init_cells.argtypes = [I, I, V, V, V, V, I]
    lib.fill_pass_cells.argtypes = [I, I, V, V, V, V, Fl]
    lib.fill_pass_cells.restype = I
    lib.fill_up_values.restype = lib.fill_lift_values.restype = lib.fill_init_cells.restype = None
    return lib


_p = trt._p
_c = trt._c


def host_init(z, outlet, flags):
    z = _c(z)
    nj, ni = z.shape
    fixed, w = np.full(z.shape, 99, np.uint8), np.full(z.shape, POISON, F)
    _host().fill_init_cells(ni, nj, _p(z), _p(_c(outlet, np.uint8)) if outlet is not None else None, _p(fixed), _p(w), int(flags))
    return fixed, w


def host_pass(z, fixed, w_old, eps):
    z, fixed, w_old = _c(z), _c(fixed, np.uint8), _c(w_old)
    nj, ni = z.shape
    wn = np.full(z.shape, POISON, F)
    changed = _host().fill_pass_cells(ni, nj, _p(z), _p(fixed), _p(w_old), _p(wn), float(eps))
    return wn, changed


UP_CASES = [(0.0, 2.0 ** -149), (-0.0, 2.0 ** -149), (2.0 ** -149, 2.0 ** -148), (-2.0 ** -149, -0.0), (1e-40, None), (-3e-42, None),
            (2.0 ** -126, 2.0 ** -126 + 2.0 ** -149), (1.0, 1.0 + 2.0 ** -23), (-1.0, -1.0 + 2.0 ** -24), (2000.0, 2000.0 + 2.0 ** -13),
            (float(np.finfo(F).max), np.inf), (-float(np.finfo(F).max), None), (np.inf, np.inf), (-np.inf, -float(np.finfo(F).max)), (-812.5, None)]


def test_up_and_lift():
    """up() at +-0, denormals, FLT_MAX, negative values and -inf: the restatement gives the values known by hand, np.nextafter agrees
    with it everywhere (it is the same function), and the compiled per-cell function equals both in every bit, the sign of -0 included.
    lift is strictly above every finite m and takes the up() branch where eps is lost in the sum."""
    m = np.array([a for a, b in UP_CASES], F)
    got = np_up(m)
    for (a, want), g in zip(UP_CASES, got):
        if want is not None:
            assert g.view(U32) == F(want).view(U32), (a, g, want)
    assert np_up(np.array([-2.0 ** -149], F)).view(U32)[0] == 0x80000000      # -0, not +0: b - 1
    fin = m[np.isfinite(m) & (np.abs(m) > F(2.0 ** -149))]                # nextafter's zero has no pinned sign
    with np.errstate(over="ignore"):
        assert_same(np_up(fin), np.nextafter(fin, INF), "np_up against nextafter")
    nan = np.array([np.nan], F)
    assert np_up(nan).view(U32)[0] == nan.view(U32)[0]
    r = np.random.default_rng(5)
    many = np.concatenate([m, nasty(r, 4000), r.integers(0, 2 ** 32, 4000, dtype=np.uint64).astype(U32).view(F)]).astype(F)
    out = np.full(many.shape, POISON, F)
    _host().fill_up_values(many.size, _p(many), _p(out))
    assert (out.view(U32) == np_up(many).view(U32)).all()                  # NaN payloads included
    for eps in (EPS, F(1e-6), F(1e-30)):
        want = np_lift(many, eps)
        _host().fill_lift_values(many.size, _p(many), float(eps), _p(out))
        ok = ~np.isnan(many)
        assert_same(out[ok], want[ok], "lift, eps %g" % eps)
        f = np.isfinite(many)
        assert (want[f] > many[f]).all()
    assert np_lift(F(2000.0), F(1e-6)) == np_up(F(2000.0)) and np_lift(F(1.0), EPS) == F(F(1.0) + EPS)


@pytest.mark.parametrize("ni, nj", WINDOWS)
def test_fixed_point_equals_priority_flood(ni, nj):
    """np_fill_fixed_point (the pass iterated) and priority_flood (a heap) give the same surface in every bit on every terrain; the
    surface is a fixed point of the pass, lies on or above the terrain, and keeps outlets and NaN cells as they are."""
    for (name, z, eps, outlet, flags), (fixed, w0, ws, passes) in zip(cases(ni, nj), solved(ni, nj).values()):
        what = "%dx%d %s" % (ni, nj, name)
        assert_same(priority_flood(z, fixed, w0, eps), ws, what)
        again, changed = np_fill_pass(z, fixed, ws, eps)
        assert changed == 0
        assert_same(again, ws, what + ": a fixed point")
        free = fixed == 0
        assert (ws[free] >= z[free]).all(), what
        assert_same(ws[~free], z[~free], what + ": outlets and NaN cells")
        assert passes <= free.sum() + 1


def np_steps_to_exit(d, nstep):
    """Where every cell is after following directions for at least nstep steps (pointer doubling): flat cell indices."""
    nj, ni = d.shape
    idx = np.arange(ni * nj).reshape(nj, ni)
    dj = np.array((0,) + trt.DJ)[d]
    di = np.array((0,) + trt.DI)[d]
    nxt = ((idx // ni + dj) * ni + (idx % ni + di)).ravel()
    n = 1
    while n < nstep:
        nxt = nxt[nxt]
        n *= 2
    return nxt


def np_drained(z, fixed, eps):
    """The cells whose raw terrain already drains: outlets, and every free cell with a neighbour in the set that lies at least one lift
    below it (z(c) >= lift(z(n))).  By induction W* = z on the whole set: W*(n) = z(n) makes lift(M(c)) <= lift(z(n)) <= z(c)."""
    d = fixed == 1
    while True:
        zz = np.where(d, z, INF).astype(F)
        with np.errstate(all="ignore"):
            new = d | ((fixed == 0) & (z >= np_lift(np_neighbour_min(zz), eps)))
        if (new == d).all():
            return d
        d = new


def check_properties(what, z, fixed, ws, eps):
    """What the filled surface is for: noahmp_hip_flow_terrain's rule on it leaves direction 0 only at outlets, every path ends at one
    within ni*nj steps, W* >= z with equality wherever the raw terrain already drained, and fixed cells keep their bits."""
    nj, ni = z.shape
    d = np_flow_dir(ws, DX, DY)
    assert (fixed[d == 0] == 1).all(), "%s: %d cells without a direction are no outlets" % (what, (fixed[d == 0] != 1).sum())
    end = np_steps_to_exit(d, ni * nj)
    assert (d.ravel()[end] == 0).all() and (fixed.ravel()[end] == 1).all(), what + ": a path that does not end at an outlet"
    free = fixed == 0
    assert (ws[free] >= z[free]).all(), what
    drained = np_drained(z, fixed, eps)
    assert_same(ws[drained], z[drained], what + ": cells that drained already")
    assert_same(ws[fixed == 1], z[fixed == 1], what + ": outlets and NaN cells")
    return d


@pytest.mark.parametrize("ni, nj", WINDOWS)
def test_the_surface_drains(ni, nj):
    """The properties on the restated W*, every terrain; on the raw hills of 67 x 35 and 70 x 130 they fail (pits), which is what the
    feature is for."""
    for (name, z, eps, outlet, flags), (fixed, w0, ws, passes) in zip(cases(ni, nj), solved(ni, nj).values()):
        check_properties("%dx%d %s" % (ni, nj, name), z, fixed, ws, eps)
    if (ni, nj) in ((67, 35), CUT):
        name, z, eps, outlet, flags = cases(ni, nj)[0]
        fixed = solved(ni, nj)[name][0]
        raw = np_flow_dir(z, DX, DY)
        assert (fixed[raw == 0] != 1).any(), "raw hills without a pit"
        assert (np_drained(z, fixed, eps) & (fixed == 0)).any()


@pytest.mark.parametrize("ni, nj", WINDOWS)
def test_host_init_and_pass_equal_the_restatement(ni, nj):
    """nmp_dev_flow_fill.hpp compiled for the host: fixed and w of init, then w and the changed flag of every one of the first 12 calls and
    of the call at the fixed point, equal the restatement in every word, on every terrain."""
    for (name, z, eps, outlet, flags), (fixed, w0, ws, passes) in zip(cases(ni, nj), solved(ni, nj).values()):
        what = "%dx%d %s" % (ni, nj, name)
        hf, hw = host_init(z, outlet, flags)
        assert_same_bytes(hf, fixed, what + ": fixed")
        assert_same(hw, w0, what + ": w of init")
        w = w0
        for n in range(min(12, passes)):
            want, flag = np_fill_pass(z, fixed, w, eps)
            got, gflag = host_pass(z, fixed, w, eps)
            assert_same(got, want, "%s: call %d" % (what, n + 1))
            assert gflag == flag
            w = want
        got, gflag = host_pass(z, fixed, ws, eps)
        assert gflag == 0
        assert_same(got, ws, what + ": the fixed point")


def test_ring_sides_and_walls_of_init():
    """RING wins over everything else (a NaN cell, a caller outlet, the corner shared with an OUTLET side); a side with neither flag is
    a wall of free cells; a ring stays at +inf."""
    ni, nj = 9, 6
    z = tsh.terrain(ni, nj).copy()
    z[0, 0] = z[3, 0] = np.nan
    o = np.zeros((nj, ni), np.uint8)
    o[2, 0] = o[2, 4] = 1
    flags = side_flags("s", "wn")
    fixed, w = np_fill_init(z, o, flags)
    assert (fixed[:, 0] == 2).all() and (fixed[nj - 1, :] == 2).all() and (fixed[0, 1:] == 1).all()
    assert fixed[2, 4] == 1 and fixed[3, 1] == 1 and fixed[1:nj - 1, ni - 1].tolist() == [0] * (nj - 2)
    assert np.isinf(w[fixed == 2]).all() and np.isinf(w[fixed == 0]).all()
    hf, hw = host_init(z, o, flags)
    assert_same_bytes(hf, fixed, "fixed")
    assert_same(hw, w, "w")


# ---------------------------------------------------------------------------------------------------------------- refusals and bindings
PLANES = ("height", "outlet", "fixed", "w_old", "w_new", "changed")


def _fill_block(ptrs, ni=5, nj=3, **kw):
    b = abi.FlowFill()
    for k in PLANES:
        setattr(b, k, ptrs[k])
    b.ni, b.nj, b.eps, b.sweeps, b.flags = ni, nj, 1e-3, 1, ALL_OUTLET
    for k, v in kw.items():
        setattr(b, k, v)
    return b


REFUSALS = [(dict(ni=-1), "ni*nj"), (dict(nj=-1), "ni*nj"), (dict(ni=65536, nj=32768), "ni*nj"),
            (dict(eps=0.0), "normal float32"), (dict(eps=-1e-3), "eps"), (dict(eps=float("nan")), "eps"), (dict(eps=float("inf")), "eps"),
            (dict(eps=9e-31), "flow_terrain"), (dict(sweeps=0), "sweeps"), (dict(sweeps=-3), "sweeps"), (dict(sweeps=CAP + 1), str(CAP)),
            (dict(flags=1 | 16), "not both"), (dict(flags=8 | 128 | 2), "not both"), (dict(flags=256), "unknown"), (dict(flags=-1), "unknown")]


def _refusals(lib, ptrs):
    """Every refusal of both calls: -105 and a text that names the call and the rule."""
    err = lambda: lib.noahmp_hip_last_error().decode()                   # noqa: E731
    for fn, name, required in ((lib.noahmp_hip_flow_fill_init, "noahmp_hip_flow_fill_init", ("height", "fixed", "w_old")),
                               (lib.noahmp_hip_flow_fill, "noahmp_hip_flow_fill", ("height", "fixed", "w_old", "w_new", "changed"))):
        assert fn(None, None) == -105 and "NULL" in err() and name + ":" in err()
        for field in required:
            assert fn(C.byref(_fill_block(ptrs, **{field: None})), None) == -105 and "required" in err() and name + ":" in err(), field
        for kw, word in REFUSALS:
            assert fn(C.byref(_fill_block(ptrs, **kw)), None) == -105 and word in err() and name + ":" in err(), (kw, err())
    assert lib.noahmp_hip_flow_fill(C.byref(_fill_block(ptrs, w_new=ptrs["w_old"])), None) == -105 and "different" in err()
    assert lib.noahmp_hip_flow_fill(C.byref(_fill_block(ptrs, sweeps=CAP, w_new=ptrs["w_old"])), None) == -105


def test_refusals_write_nothing():
    """Every refusal returns -105 with text before anything is launched or read: the planes here are host memory that the calls must not
    touch, and they keep their poison."""
    lib = abi.load_library()
    planes = {k: np.full(15, POISON, F) for k in PLANES}
    _refusals(lib, {k: v.ctypes.data for k, v in planes.items()})
    assert all((p == POISON).all() for p in planes.values())


HEADER_LINES = (
    "#define NOAHMP_HIP_HAS_FLOW_FILL 1\n", "#define NOAHMP_HIP_ABI_MINOR 3\n", "#define NOAHMP_FLOW_FILL_TILE_I ", "#define NOAHMP_FLOW_FILL_TILE_J ",
    "#define NOAHMP_FLOW_FILL_MAX_SWEEPS ", "typedef struct noahmp_flow_fill {", "} noahmp_flow_fill;",
    "noahmp_hip_flow_fill_init(const noahmp_flow_fill* f, void* stream);", "noahmp_hip_flow_fill(const noahmp_flow_fill* f, void* stream);",
    "min(a, b) = (b < a) ? b : a;  max(a, b) = (b > a) ? b : a", "lift(m) = max(m + eps, up(m))", "+-0 -> the smallest subnormal",
    "W*(c) = max(z(c), lift(M(c)))", "W* is UNIQUE", "ANY chaotic relaxation", "RING wins over everything else",
    "a = m + eps;  l = max(a, up(m));  cand = max(height[c], l);  w_new[c] = min(w_old[c], cand)",
    "fixed cells are unchanged;  height <= w_new <= w_old at free cells;  w_new >= W*;  w_new <= the pinned form's result",
    "A call that changes nothing certifies w_old == W*", "No kernel waits for another workgroup", "carving / breaching, lakes",
    "conditions it first (noahmp_hip_flow_fill, below)") + tuple("#define NOAHMP_FILL_%s_%s " % (a, b) for a in ("OUTLET", "RING") for b in "WESN")
SYMBOLS = ("noahmp_hip_flow_fill_init", "noahmp_hip_flow_fill")
FIELDS = ["height", "outlet", "fixed", "w_old", "w_new", "changed", "ni", "nj", "eps", "sweeps", "flags"]


def test_bindings_regenerate_identically_with_the_fill_calls():
    from tools import gen_abi
    for rel, text in (("include/noahmp_hip.h", gen_abi.c_header()), ("oracle/ref_harness_gen.f90", gen_abi.ref_harness()),
                      ("noahmp_amd/fortran/module_sf_noahmpdrv_hip.F90", gen_abi.fortran_shim()),
                      ("tests/fortran/shim_wrap_gen.f90", gen_abi.shim_wrap())):
        assert open(os.path.join(ROOT, rel)).read() == text, rel
    hdr = open(HEADER).read()
    for word in HEADER_LINES:
        assert word in hdr, word
    assert "\n".join(gen_abi.flow_fill_header()) in hdr
    assert "noahmp_flow_fill" not in gen_abi.ref_harness()
    f90 = open(os.path.join(ROOT, "noahmp_amd", "fortran", "module_sf_noahmpdrv_hip.F90")).read()
    for word in ("bind(C, name='noahmp_hip_flow_fill_init')", "bind(C, name='noahmp_hip_flow_fill')", "type, bind(C) :: noahmp_flow_fill ",
                 "NOAHMP_FILL_RING_N = 128", "NOAHMP_FLOW_FILL_TILE_I = %d" % TI):
        assert word in f90, word
    for sym in SYMBOLS:
        assert sym in abi.EXPORTED_SYMBOLS
    assert [n for n, _ in abi.FlowFill._fields_] == FIELDS
    assert abi.FILL_FLAG == {"%s_%s" % (a, s): v for a, t in (("outlet", OUTLET), ("ring", RING)) for s, v in t.items()}
    assert (abi.FILL_TILE_I, abi.FILL_TILE_J, abi.FILL_MAX_SWEEPS) == (TI, TJ, CAP) and TI * TJ % 256 == 0


def test_ctypes_mirror_matches_the_compiled_header(tmp_path):
    names = [n for n, _ in abi.FlowFill._fields_]
    body = 'printf(" %zu", sizeof(noahmp_flow_fill));' + "".join('printf(" %%zu", offsetof(noahmp_flow_fill, %s));' % n for n in names)
    want = [C.sizeof(abi.FlowFill)] + [getattr(abi.FlowFill, n).offset for n in names]
    flags = ["NOAHMP_FILL_%s_%s" % (a, b) for a in ("OUTLET", "RING") for b in "WESN"]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "noahmp_hip.h"\nint main(){' + body +
                   'printf(" %d %d", NOAHMP_HIP_ABI_MINOR, NOAHMP_HIP_HAS_FLOW_FILL);' +
                   "".join('printf(" %%d", %s);' % f for f in flags) + " return 0;}")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert out == want + [3, 1] + [OUTLET[s] for s in "wesn"] + [RING[s] for s in "wesn"]


def test_library_exports_the_fill_calls():
    if not os.path.exists(abi.LIB_PATH):
        from noahmp_amd import build as b
        b.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", abi.LIB_PATH]).decode()
    for sym in SYMBOLS:
        assert " T %s\n" % sym in out, sym


@pytest.mark.skipif(tr._flang() is None, reason="no flang")
def test_generated_fortran_type_and_interfaces_compile(tmp_path):
    """The fill part of the generated module compiles, and a caller of the two interfaces type-checks."""
    from tools import gen_abi
    text = "\n".join(["module flow_fill_abi_check", "  use iso_c_binding", "  implicit none"] + gen_abi.flow_fill_f90_types() + ["  interface"] +
                     gen_abi.flow_fill_f90_interfaces() +
                     ["  end interface", "contains", "  function go(planes) result(rc)", "    type(c_ptr), intent(in) :: planes(6)",
                      "    type(noahmp_flow_fill) :: f", "    integer(c_int) :: rc",
                      "    f%height = planes(1); f%outlet = c_null_ptr; f%fixed = planes(3); f%w_old = planes(4); f%w_new = planes(5)",
                      "    f%changed = planes(6); f%ni = 64; f%nj = 8; f%eps = 1.0e-3; f%sweeps = NOAHMP_FLOW_FILL_MAX_SWEEPS",
                      "    f%flags = ior(NOAHMP_FILL_OUTLET_W, NOAHMP_FILL_RING_E)",
                      "    rc = noahmp_hip_flow_fill_init(f, c_null_ptr)", "    rc = noahmp_hip_flow_fill(f, c_null_ptr)",
                      "  end function go", "end module flow_fill_abi_check", ""])
    f = tmp_path / "flow_fill_abi_check.f90"
    f.write_text(text)
    subprocess.check_call([tr._flang(), "-c", str(f), "-o", str(tmp_path / "flow_fill_abi_check.o"), "-J", str(tmp_path)], cwd=str(tmp_path))


# ---------------------------------------------------------------------------------------------------------------- GPU
_dev = tr._dev


class _Gpu:
    """The device planes of one case at odd offsets inside poisoned pools, and the calls on them one by one."""

    def __init__(self, engine, z, eps, outlet, flags):
        import torch
        self.engine, self.torch = engine, torch
        nj, ni = z.shape
        self.shape, self.n = (nj, ni), ni * nj
        self.fpool, (w0, w1) = trt._pool(self.n, 2, torch.float32, POISON)
        self.bpool, (fx,) = trt._pool(self.n, 1, torch.uint8, 0xEE)
        self.ipool, (ch,) = trt._pool(1, 1, torch.int32, 77)
        self.w, self.fixed, self.changed, self.cur = [w0.view(nj, ni), w1.view(nj, ni)], fx.view(nj, ni), ch, 0
        self.z, self.outlet, self.eps, self.flags = _dev(z), _dev(outlet) if outlet is not None else None, float(eps), int(flags)
        torch.cuda.synchronize()

    def block(self, sweeps):
        return self.engine.flow_fill_block(self.z, self.fixed, self.w[self.cur], self.w[1 - self.cur], self.changed, self.eps, sweeps=sweeps,
                                           flags=self.flags, outlet=self.outlet)

    def init(self):
        self.engine.flow_fill_init(self.block(1))
        self.engine.stream_sync()
        return self.fixed.cpu().numpy(), self.w[self.cur].cpu().numpy()

    def call(self, sweeps):
        """One call: (w_new, changed)."""
        self.changed.zero_()
        self.torch.cuda.synchronize()
        self.engine.flow_fill(self.block(sweeps))
        self.engine.stream_sync()
        self.cur = 1 - self.cur
        return self.w[self.cur].cpu().numpy(), int(self.changed.item())

    def guards_ok(self):
        return trt._guards_ok(self.fpool, self.n, POISON) and trt._guards_ok(self.bpool, self.n, 0xEE) and trt._guards_ok(self.ipool, 1, 77)


@pytest.mark.gpu
@pytest.mark.parametrize("ni, nj", WINDOWS)
def test_gpu_pinned_form_equals_the_restatement(engine, ni, nj):
    """fixed and w after noahmp_hip_flow_fill_init and after each of the first 3 calls with sweeps = 1, and the changed flag of each,
    equal the restatement in every word, on every terrain; a call at the fixed point leaves the flag alone; guard words keep their poison."""
    for (name, z, eps, outlet, flags), (fixed, w0, ws, passes) in zip(cases(ni, nj), solved(ni, nj).values()):
        what = "%dx%d %s" % (ni, nj, name)
        g = _Gpu(engine, z, eps, outlet, flags)
        gf, gw = g.init()
        assert_same_bytes(gf, fixed, what + ": fixed")
        assert_same(gw, w0, what + ": w of init")
        w = w0
        for n in range(3):
            want, flag = np_fill_pass(z, fixed, w, eps)
            got, gflag = g.call(1)
            assert_same(got, want, "%s: call %d" % (what, n + 1))
            assert gflag == flag, what
            w = want
        g.w[g.cur].copy_(_dev(ws))
        got, gflag = g.call(1)
        assert gflag == 0
        assert_same(got, ws, what + ": the fixed point")
        assert g.guards_ok(), what


def check_call(what, z, fixed, ws, eps, w_old, w_new, flag):
    """The five invariants that pin one call of the tiled form."""
    free = fixed == 0
    assert_same(w_new[~free], w_old[~free], what + ": fixed cells")
    assert (z[free] <= w_new[free]).all() and (w_new[free] <= w_old[free]).all(), what + ": height <= w_new <= w_old"
    assert (w_new[free] >= ws[free]).all(), what + ": w_new >= W*"
    jac, _ = np_fill_pass(z, fixed, w_old, eps)
    assert (w_new[free] <= jac[free]).all(), what + ": w_new <= the pinned form's result"
    assert flag == int((w_new.view(U32) != w_old.view(U32)).any()), what + ": changed"


@pytest.mark.gpu
@pytest.mark.parametrize("sweeps", SWEEPS)
@pytest.mark.parametrize("ni, nj", WINDOWS)
def test_gpu_tiled_form(engine, ni, nj, sweeps):
    """The tiled kernel, every terrain: after EVERY call the five invariants hold against the restatement's W* and its pinned pass; at
    convergence the plane equals W* in every word; calls <= free cells + 1; never more calls than the Jacobi iteration needs passes."""
    for (name, z, eps, outlet, flags), (fixed, w0, ws, passes) in zip(cases(ni, nj), solved(ni, nj).values()):
        what = "%dx%d %s sweeps %d" % (ni, nj, name, sweeps)
        g = _Gpu(engine, z, eps, outlet, flags)
        gf, w = g.init()
        assert_same_bytes(gf, fixed, what + ": fixed")
        bound = int((fixed == 0).sum()) + 1
        calls = 0
        while True:
            new, flag = g.call(sweeps)
            calls += 1
            check_call("%s, call %d" % (what, calls), z, fixed, ws, eps, w, new, flag)
            w = new
            if not flag:
                break
            assert calls < bound, what + ": more calls than free cells + 1"
        assert_same(w, ws, what + ": the fixed point")
        assert calls <= passes, "%s: %d calls, the Jacobi iteration needs %d" % (what, calls, passes)
        assert g.guards_ok(), what


def _fill(engine, z, eps, outlet, flags, sweeps, **kw):
    from noahmp_amd.routing import DepressionFill
    f = DepressionFill(engine)
    sides = lambda t: "".join(s for s in "wesn" if flags & t[s])          # noqa: E731
    f.begin(_dev(z), eps, outlet=_dev(outlet) if outlet is not None else None, outlet_sides=sides(OUTLET), ring_sides=sides(RING))
    f.run(sweeps=sweeps, **kw)
    return f


@pytest.mark.gpu
def test_gpu_serpentine_tiled_needs_fewer_calls(engine):
    """On the serpentine of 70 x 130 (2 x 5 tiles, a corridor of about 4 500 cells) DepressionFill.run reaches W* with sweeps = 1 and
    with sweeps = 64, and the tiled form needs strictly fewer calls.  run() raises when max_call is too small."""
    ni, nj = CUT
    name, z, eps, outlet, flags = cases(ni, nj)[-1]
    fixed, w0, ws, passes = solved(ni, nj)[name]
    assert name == "serpentine" and passes > 1000
    pinned = _fill(engine, z, eps, outlet, flags, 1, check=64)
    tiled = _fill(engine, z, eps, outlet, flags, 64)
    assert_same(pinned.surface.cpu().numpy(), ws, "pinned")
    assert_same(tiled.surface.cpu().numpy(), ws, "tiled")
    assert pinned.free_cells == int((fixed == 0).sum())
    assert passes <= pinned.calls < passes + 64, (pinned.calls, passes)
    assert tiled.calls < pinned.calls, "calls to the fixed point: tiled (sweeps = 64) %d, pinned %d" % (tiled.calls, pinned.calls)
    with pytest.raises(RuntimeError, match="still changing"):
        _fill(engine, z, eps, outlet, flags, 1, max_call=10)


@pytest.mark.gpu
@pytest.mark.parametrize("ni, nj", [(67, 35), (TI, TJ), CUT])
def test_gpu_properties_of_the_filled_surface(engine, ni, nj):
    """On the GPU's own result (DepressionFill with the default sweeps), every terrain: noahmp_hip_flow_terrain leaves direction 0 only
    at cells with fixed == 1, every path ends at one within ni*nj steps, W* >= z with equality where the raw terrain drained already,
    outlets and NaN cells keep their bits."""
    import torch
    for (name, z, eps, outlet, flags), (fixed, w0, ws, passes) in zip(cases(ni, nj), solved(ni, nj).values()):
        what = "%dx%d %s" % (ni, nj, name)
        f = _fill(engine, z, eps, outlet, flags, None)
        got = f.surface.cpu().numpy()
        assert_same(got, ws, what)
        assert_same_bytes(f.fixed.cpu().numpy(), fixed, what + ": fixed")
        assert 1 <= f.calls <= f.free_cells + 1
        d = torch.full(z.shape, 99, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        engine.flow_terrain(engine.flow_terrain_block(f.surface, d, DX, DY))
        engine.stream_sync()
        assert_same_bytes(d.cpu().numpy(), check_properties(what, z, fixed, got, eps), what + ": dir of the filled plane")


def _ring_sides(tile, blk):
    (tj, ti), (bj, bi) = tile, blk
    return "".join(s for s, yes in (("w", bi.start < ti.start), ("e", bi.stop > ti.stop), ("s", bj.start < tj.start), ("n", bj.stop > tj.stop)) if yes)


class _RingFromWhole:
    """A stand-in for Comm in one process, in the manner of test_routing._RingFromWhole: exchange_halo copies the ring of the plane from a
    whole-domain plane, ENQUEUED ONLY on torch's current stream; agree_any returns its argument.  sources: the whole-domain planes, one
    per phase; a phase ends when agree_any hears that nothing changed."""

    def __init__(self, sources, blk, ring):
        self.sources, self.blk, self.ring, self.calls, self.phase = sources, blk, ring, 0, 0

    def exchange_halo(self, planes, geom):
        import torch
        assert len(planes) == 1 and geom == "geom"
        planes[0].copy_(torch.where(self.ring, self.sources[self.phase][self.blk], planes[0]))
        self.calls += 1

    def agree_any(self, flag):
        if not flag:
            self.phase += 1
        return flag


@pytest.mark.gpu
def test_gpu_decomposition(engine):
    """70 x 130 cut 2 x 2, one process: four DepressionFill objects on their blocks (the tile plus a 1-cell ring where there is a
    neighbour: RING sides, the others OUTLET), the rings copied between them by slicing after every round until no part changes: every
    part equals the whole in every word, ring included.  Then run(comm=stand-in) per part with the ring taken from the whole's W* on a
    side stream, and set_terrain_filled per part: dir and inmask of the whole on the tile's cells."""
    import torch
    from noahmp_amd.routing import DepressionFill, FlowNetwork
    ni, nj = CUT
    name, z, eps, outlet, flags = cases(ni, nj)[0]
    fixed, w0, ws, passes = solved(ni, nj)[name]
    parts = []
    for (tile, blk, bidx) in tsh._cuts(ni, nj, 1):
        f = DepressionFill(engine)
        ring = _ring_sides(tile, blk)
        assert len(ring) == 2
        f.begin(_dev(z[blk]), eps, outlet_sides="".join(s for s in "wesn" if s not in ring), ring_sides=ring)
        own = (slice(tile[0].start - blk[0].start, tile[0].stop - blk[0].start), slice(tile[1].start - blk[1].start, tile[1].stop - blk[1].start))
        assert ((f.fixed.cpu().numpy() == 2) == (bidx < 0)).all()
        parts.append((f, tile, blk, own, _dev(bidx < 0), ring))
    G = torch.full((nj, ni), float("inf"), dtype=torch.float32, device="cuda")
    rounds = 0
    while True:
        for f, tile, blk, own, ring_mask, ring in parts:
            G[tile] = f.surface[own]
        for f, tile, blk, own, ring_mask, ring in parts:
            f.surface.copy_(torch.where(ring_mask, G[blk], f.surface))    # the exchange: the ring from the owners
        torch.cuda.synchronize()
        rounds += 1
        if not any([f.relax(1) for f, *_ in parts]):                     # every part makes its call, then the flags are agreed on
            break
        assert rounds <= passes + 1, "more rounds than the Jacobi iteration of the whole needs passes"
    for f, tile, blk, own, ring_mask, ring in parts:
        assert_same(f.surface.cpu().numpy(), ws[blk], "part %s after %d rounds, ring included" % (tile, rounds))
    whole_w = _dev(ws)
    dwant = np_flow_dir(ws, DX, DY)
    mwant = np_inmask(dwant)
    whole_d = _dev(dwant.astype(F))
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    for f0, tile, blk, own, ring_mask, ring in parts:
        comm = _RingFromWhole([whole_w, whole_d], blk, ring_mask)
        f = DepressionFill(engine)
        f.begin(_dev(z[blk]), eps, outlet_sides="".join(s for s in "wesn" if s not in ring), ring_sides=ring)
        with torch.cuda.stream(side):
            f.run(comm=comm, geom="geom")
        engine.stream_sync()
        torch.cuda.synchronize()
        assert comm.calls == f.calls >= 2 and comm.phase == 1
        assert_same(f.surface.cpu().numpy(), ws[blk], "run(comm) of part %s" % (tile,))
        tj, ti = tile
        net = FlowNetwork(engine, ti.stop - ti.start, tj.stop - tj.start)
        comm = _RingFromWhole([whole_w, whole_d], blk, ring_mask)
        with torch.cuda.stream(side):
            net.set_terrain_filled(_dev(z[blk]), DX, DY, eps, origin=(own[1].start, own[0].start), comm=comm, geom="geom")
        engine.stream_sync()
        torch.cuda.synchronize()
        assert comm.calls == net.fill_calls + 1
        assert_same(net.filled.cpu().numpy(), ws[blk], "filled block of part %s" % (tile,))
        assert_same_bytes(net.tile_view(net.dir).cpu().numpy(), dwant[tile], "dir of part %s" % (tile,))
        assert_same_bytes(net.tile_view(net.inmask).cpu().numpy(), mwant[tile], "inmask of part %s" % (tile,))
        assert_same_bytes(net.dir.cpu().numpy(), dwant[blk], "dir of part %s, ring included" % (tile,))
    with pytest.raises(ValueError, match="comm"):
        net.set_terrain_filled(_dev(z[blk]), DX, DY, eps, origin=(own[1].start, own[0].start))


@pytest.mark.gpu
def test_gpu_through_flownetwork(engine):
    """67 x 35 hills.  set_terrain(fill=eps), release = 1, unit input: out converges to the upstream count, the counts at the cells
    without a direction add up to the number of cells, and every such cell is an outlet.  The same with fill=None has cells without a
    direction that are no outlets, and gives the planes of the unfilled path: dir, inmask and area of the existing restatement."""
    import types
    import torch
    from noahmp_amd.routing import FlowNetwork
    ni, nj = 67, 35
    name, z, eps, outlet, flags = cases(ni, nj)[0]
    fixed, w0, ws, passes = solved(ni, nj)[name]
    raw = FlowNetwork(engine, ni, nj)
    raw.set_terrain(_dev(z), DX, DY, fill=None)
    draw = np_flow_dir(z, DX, DY)
    assert raw.filled is None
    assert_same_bytes(raw.dir.cpu().numpy(), draw, "fill=None: dir")
    assert_same_bytes(raw.inmask.cpu().numpy(), np_inmask(draw), "fill=None: inmask")
    assert (raw.area.cpu().numpy() == F(DX * DY)).all()
    assert (fixed[draw == 0] != 1).any()
    net = FlowNetwork(engine, ni, nj)
    net.set_terrain(_dev(z), DX, DY, fill=float(eps))
    assert_same(net.filled.cpu().numpy(), ws, "net.filled")
    d = np_flow_dir(ws, DX, DY)
    assert_same_bytes(net.dir.cpu().numpy(), d, "dir")
    assert (fixed[d == 0] == 1).all()
    acc = net.upstream_cells(max_pass=ni * nj).cpu().numpy().view(U32)
    want, npass = trt.np_upstream(np_inmask(d))
    assert_same(acc, want, "upstream_cells on the filled network")
    assert int(acc[d == 0].astype(np.int64).sum()) == ni * nj
    net.set_area(1.0)
    net.set_release(1.0)
    net.set_input_columns(None)
    one = torch.ones(ni * nj, dtype=torch.float32, device="cuda")
    store = types.SimpleNamespace(ni=ni, nj=nj, a=dict(runsfxy=one))
    torch.cuda.synchronize()
    for _ in range(npass):
        net.step(store, 1000.0, fields=("runsfxy",))                     # scale = fl(1000 * fl(1e-3)) = 1.0: one unit per cell and call
    engine.stream_sync()
    out = net.out[net.cur].cpu().numpy()
    assert_same(out, acc.astype(F), "out after %d calls against the upstream count" % npass)
    assert float(out[d == 0].astype(np.float64).sum()) == ni * nj


@pytest.mark.gpu
def test_gpu_refusals_launch_nothing(engine):
    """The refusals with device planes: -105, text, and every plane keeps its poison."""
    import torch
    fl = torch.full((6, 15), POISON, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    _refusals(engine.lib, {k: fl[n].data_ptr() for n, k in enumerate(PLANES)})
    engine.stream_sync()
    torch.cuda.synchronize()
    assert (fl.cpu().numpy() == POISON).all()
    # an empty window is no refusal and writes nothing
    b = _fill_block({k: fl[n].data_ptr() for n, k in enumerate(PLANES)}, nj=0)
    assert engine.lib.noahmp_hip_flow_fill_init(C.byref(b), None) == 0 and engine.lib.noahmp_hip_flow_fill(C.byref(b), None) == 0
    b.sweeps = 7
    assert engine.lib.noahmp_hip_flow_fill(C.byref(b), None) == 0
    engine.stream_sync()
    assert (fl.cpu().numpy() == POISON).all()
