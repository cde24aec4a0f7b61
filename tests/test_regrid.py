"""Forcing regrid: coarse forcing records -> the model grid's planes on the device (noahmp_regrid.hip, nmp_dev_regrid.hpp).

No reference routine stands behind the calls (the reference reads forcing already on the model grid, netcdf_io:1140): the contract is the
text in include/noahmp_hip.h.  np_plan / np_regrid below restate that text in numpy -- float64 index arithmetic, float32 weights and
values, one rounding per operation -- and everything is compared with them bit for bit (NaN equals NaN, no element may differ): the
per-cell functions compiled for the host, the plan kernel, the regrid kernel on both of its paths, permuted plans, and a two-step engine
run fed through ForcingRegrid against the same run fed with fine records made by the restatement."""
import ctypes as C
import functools
import math
import os
import subprocess

import numpy as np
import pytest

from noahmp_amd import abi, synth

F, D = np.float32, np.float64
HUGE = np.float32(3.40282347e+38)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "noahmp_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host_emul", "regrid_check.hip")
LIB = os.path.join(ROOT, "tests", "host_emul", "libregrid_check.so")
BIL, NEAR = 0, 1


# ---------------------------------------------------------------------------------------------------------------- the restatement
def source(nx, ny, lon0, lat0, dlon, dlat, periodic_x=False):
    g = abi.RegridSource()
    g.nx, g.ny, g.lon0, g.lat0, g.dlon, g.dlat, g.periodic_x = nx, ny, lon0, lat0, dlon, dlat, int(periodic_x)
    return g


def _search(x, y, nx, ny, per, v, radius):
    ri, rj = int(math.floor(x + 0.5)), int(math.floor(y + 0.5))
    best, bestd = -1, None
    for j in range(rj - radius, rj + radius + 1):
        if j < 0 or j >= ny:
            continue
        for ii in range(ri - radius, ri + radius + 1):
            if per:
                i = ii % nx
            elif ii < 0 or ii >= nx:
                continue
            else:
                i = ii
            idx = j * nx + i
            if not v[idx]:
                continue
            dx = abs(D(i) - x)
            if per:
                dx = min(dx, D(nx) - dx)
            dy = D(j) - y
            d = dx * dx + dy * dy
            if best < 0 or d < bestd or (d == bestd and idx < best):
                best, bestd = idx, d
    return best


def np_plan(xlat, xlon, g, valid=None, radius=0):
    """The header text of noahmp_hip_regrid_plan_latlon.  Returns (plan int32 [6, n]: base, near, w0..w3 as bits; unfilled)."""
    xlat, xlon = np.asarray(xlat, F).ravel(), np.asarray(xlon, F).ravel()
    n, nx, ny, per = xlat.size, int(g.nx), int(g.ny), bool(g.periodic_x)
    plan = np.zeros((6, n), np.int32)
    plan[0:2] = -1
    wts = plan[2:].view(F)
    v = None if valid is None else np.asarray(valid, np.uint8).ravel()
    with np.errstate(all="ignore"):
        fx = (xlon.astype(D) - D(g.lon0)) / D(g.dlon)
        if per:
            fx = fx - np.floor(fx / D(nx)) * D(nx)
            fx = np.where(fx < 0, fx + D(nx), fx)
            fx = np.where(fx >= nx, fx - D(nx), fx)
            inx = (fx >= 0) & (fx < nx)
        else:
            inx = (fx >= -0.5) & (fx <= nx - 0.5)
        fy = (xlat.astype(D) - D(g.lat0)) / D(g.dlat)
        inside = inx & (fy >= -0.5) & (fy <= ny - 0.5)
    zero, one, half = F(0), F(1), F(0.5)
    for c in np.nonzero(inside)[0]:
        x, y = fx[c], fy[c]
        if not per:
            x = min(max(x, D(0)), D(nx - 1))
        y = min(max(y, D(0)), D(ny - 1))
        j0 = min(int(math.floor(y)), ny - 2)
        i0 = int(math.floor(x)) if per else min(int(math.floor(x)), nx - 2)
        i1 = 0 if (per and i0 == nx - 1) else i0 + 1
        j1 = j0 + 1
        tx, ty = F(x - D(i0)), F(y - D(j0))
        ux, uy = one - tx, one - ty
        w = [ux * uy, tx * uy, ux * ty, tx * ty]
        idx = [j0 * nx + i0, j0 * nx + i1, j1 * nx + i0, j1 * nx + i1]
        ok = [True] * 4 if v is None else [bool(v[i]) for i in idx]
        base, found, replaced = idx[0], -1, False
        if not all(ok):
            w = [wk if o else zero for wk, o in zip(w, ok)]
            s = ((w[0] + w[1]) + w[2]) + w[3]
            if s > 0:
                w = [wk / s for wk in w]
            else:
                found = _search(x, y, nx, ny, per, v, radius)
                base, replaced = found, True
        pk = int(tx > half) + 2 * int(ty > half)
        if ok[pk]:
            near = idx[pk]
        elif any(ok):
            bk = -1
            for k in range(4):
                if ok[k] and (bk < 0 or w[k] > w[bk]):
                    bk = k
            near = idx[bk]
        else:
            near = found
        if replaced:
            w = [one if found >= 0 else zero, zero, zero, zero]
        plan[0, c], plan[1, c] = base, near
        for k in range(4):
            wts[k, c] = w[k]
    return plan, int((plan[0] < 0).sum())


def np_regrid(plan, g, src, mode, adjust=None, scale=0.0, fill=-999.0):
    """The header text of noahmp_hip_forcing_regrid for one entry.  plan: int32 [6, n]; src: flat float32 (may be longer than nx*ny)."""
    n, nx, per = plan.shape[1], int(g.nx), bool(g.periodic_x)
    nxny = nx * int(g.ny)
    wts = plan[2:].view(F)
    out = np.empty(n, F)
    scale, fill = F(scale), F(fill)
    with np.errstate(all="ignore"):
        for c in range(n):
            if mode == BIL:
                b = int(plan[0, c])
                if b < 0 or b >= nxny:
                    out[c] = fill
                    continue
                c1 = b + 1 - nx if (per and b % nx == nx - 1) else b + 1
                idx = [b, c1, b + nx, c1 + nx]
                w = [wts[k, c] for k in range(4)]
                if any(w[k] != 0 and idx[k] >= nxny for k in range(1, 4)):
                    out[c] = fill
                    continue
                v = None
                for k in range(4):
                    if w[k] == 0:
                        continue                              # never read
                    p = w[k] * src[idx[k]]
                    v = p if v is None else v + p
                if v is None:
                    v = F(0)
            else:
                nr = int(plan[1, c])
                if nr < 0 or nr >= nxny:
                    out[c] = fill
                    continue
                v = src[nr]
            if adjust is not None:
                p = scale * adjust[c]
                v = v + p
            out[c] = v
    return out


def assert_same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype.itemsize == 4 and b.dtype.itemsize == 4, (what, a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype == F and b.dtype == F:
        bad = ~((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b)))
    else:
        bad = a.view(np.uint32) != b.view(np.uint32)
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError("%s: %d of %d values differ, first at %s: %r vs %r" % (what, bad.sum(), bad.size, i, a[i], b[i]))


def assert_same_plan(got, want, what):
    for k, nm in enumerate(abi.REGRID_PLANES):
        if k < 2:
            assert_same(got[k], want[k], "%s: plane %s" % (what, nm))
        else:
            assert_same(got[k].view(F), want[k].view(F), "%s: plane %s" % (what, nm))


def nasty(r, n):
    """Random float32 values that contain NaN, +-Inf, -0.0, zeros and denormals."""
    x = (r.standard_normal(n) * 10.0 ** r.integers(-3, 4, n)).astype(F)
    special = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-40, -3e-42, HUGE, -HUGE], dtype=F)
    at = r.random(n) < 0.25
    x[at] = special[r.integers(0, len(special), int(at.sum()))]
    return x


# ---------------------------------------------------------------------------------------------------------------- the cases
SOURCES = {
    "plain": source(7, 5, -100.0, 30.0, 0.5, 0.25),                     # every coordinate below is exact in float32
    "north_first": source(7, 5, -100.0, 31.0, 0.5, -0.25),              # rows from north to south
    "periodic": source(8, 4, 0.0, -60.0, 45.0, 40.0, True),
}
TARGETS = [(64, 4), (67, 5), (1, 1)]
MASKS = ["none", "random", "all_invalid", "one_valid"]


def targets(name, ni, nj):
    """xlat, xlon (nj, ni) float32: the special points first, random ones behind them."""
    g = SOURCES[name]
    nx, ny = g.nx, g.ny
    r = np.random.default_rng(ni * 100 + nj + len(name))
    n = ni * nj
    up = lambda a: np.nextafter(F(a), F(np.inf))
    dn = lambda a: np.nextafter(F(a), F(-np.inf))
    X = lambda f: F(g.lon0 + f * g.dlon)
    Y = lambda f: F(g.lat0 + f * g.dlat)
    if name == "periodic":
        pts = [(Y(1), F(359.9)), (Y(1), F(0.1)), (Y(1), F(-0.1)), (Y(1.5), F(337.5)), (Y(0), F(315.0)), (Y(2), F(360.0)), (Y(3), F(-180.0)),
               (Y(3), F(180.0)), (Y(0.25), F(720.5)), (Y(1), F(-360.0)), (Y(1), dn(0.0)), (Y(1), dn(360.0)), (Y(-0.5), F(10.0)),
               (dn(Y(-0.5)), F(10.0)), (Y(ny - 0.5), F(350.0)), (up(Y(ny - 0.5)), F(350.0)), (Y(ny - 1), F(90.0)), (F(np.nan), F(1.0)),
               (Y(1), F(np.inf)), (Y(1), F(np.nan)), (Y(1.5), F(-22.5)), (Y(1.5), F(22.5))]
        lon = np.where(r.random(n) < 0.5, r.uniform(-180.0, 180.0, n), r.uniform(0.0, 360.0, n)).astype(F)
        lat = (g.lat0 + r.uniform(-0.7, ny - 0.3, n) * g.dlat).astype(F)
    else:
        s = 1.0 if g.dlat > 0 else -1.0
        pts = [(Y(1), X(-1)), (Y(1), X(nx + 0.25)), (Y(-1), X(2)), (Y(ny), X(2)),                        # outside
               (Y(1), X(-0.5)), (Y(1), dn(X(-0.5))), (Y(1), X(nx - 0.5)), (Y(1), up(X(nx - 0.5))),          # on and beyond the +-0.5 limits
               (Y(-0.5), X(3)), (Y(ny - 0.5), X(3)), (F(Y(-0.5) - s * 1e-3), X(3)), (F(Y(ny - 0.5) + s * 1e-3), X(3)),
               (Y(0), X(0)), (Y(2), X(3)), (Y(ny - 1), X(nx - 1)), (Y(ny - 1), X(0)), (Y(0), X(nx - 1)),     # centres, last row / column
               (Y(1.5), X(nx - 1)), (Y(ny - 1), X(2.5)), (Y(-0.25), X(-0.25)), (Y(ny - 0.75), X(nx - 0.75)),  # fraction 1, the outer half cells
               (Y(1.5), X(2.5)), (Y(1.75), X(2.25)), (F(np.nan), X(1)), (Y(1), F(np.inf)), (Y(1), F(-np.inf))]
        lon = (g.lon0 + r.uniform(-0.8, nx - 0.2, n) * g.dlon).astype(F)
        lat = (g.lat0 + r.uniform(-0.8, ny - 0.2, n) * g.dlat).astype(F)
    k = min(n, len(pts))
    at = r.permutation(n)[:k] if n > len(pts) else np.arange(k)
    for p, (la, lo) in zip(at, pts[:k]):
        lat[p], lon[p] = la, lo
    return lat.reshape(nj, ni), lon.reshape(nj, ni)


def mask(name, kind, seed=0):
    g = SOURCES[name]
    m = g.nx * g.ny
    r = np.random.default_rng(31 + seed)
    if kind == "none":
        return None
    if kind == "random":
        return (r.random(m) >= 0.30).astype(np.uint8)
    v = np.zeros(m, np.uint8)
    if kind == "one_valid":
        v[int(r.integers(0, m))] = 1
    return v


@functools.lru_cache(maxsize=None)
def plan_case(name, ni, nj, kind, radius):
    """(xlat, xlon, valid, plan, unfilled) of one case: the restatement is computed once and shared by the CPU and GPU tests."""
    xlat, xlon = targets(name, ni, nj)
    v = mask(name, kind)
    plan, unfilled = np_plan(xlat, xlon, SOURCES[name], v, radius)
    for a in (xlat, xlon, plan):
        a.setflags(write=False)
    return xlat, xlon, v, plan, unfilled


def plan_cases():
    return [(name, ni, nj) for name in SOURCES for ni, nj in TARGETS]


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_the_cases_cover_what_they_are_meant_to():
    """The restated plans of the 64 x 4 cases contain every branch of the contract."""
    _, _, _, p, unf = plan_case("plain", 64, 4, "none", 0)
    w = p[2:].view(F)
    assert 0 < unf < 256 and (p[0] >= 0).sum() > 100
    assert (w[1] == 1).any() and (w[3] == 1).any() and (w[0] == 1).any()          # fraction exactly 1, cell centres
    assert ((w[0] > 0) & (w[1] > 0) & (w[2] > 0) & (w[3] > 0)).any()
    _, _, v, p, unf2 = plan_case("plain", 64, 4, "random", 2)
    w = p[2:].view(F)
    assert unf2 >= unf and ((w == 0).sum(0)[p[0] >= 0] > 0).any()                    # dropped corners, renormalised
    assert ((w[0] == 1) & (w[1:] == 0).all(0) & (p[0] >= 0) & (v[np.maximum(p[0], 0)] == 1)).any()
    _, _, _, p, unf3 = plan_case("plain", 64, 4, "all_invalid", 2)
    assert unf3 == 256 and (p[0:2] == -1).all() and (p[2:] == 0).all()
    _, _, v, p, unf4 = plan_case("plain", 64, 4, "one_valid", 2)
    the = int(np.flatnonzero(v)[0])
    w = p[2:].view(F)
    assert 0 < unf4 < 256 and ((p[0] == the) & (w[0] == 1) & (p[1] == the)).any()    # the search found the one valid cell
    _, xlon, _, p, unf5 = plan_case("periodic", 64, 4, "none", 0)
    seam = (p[0] % 8 == 7) & (p[0] >= 0)
    assert seam.any() and (xlon.ravel()[seam] < 0).any() and (xlon.ravel()[seam] > 300).any()   # the seam from both conventions


def test_identity_on_cell_centres():
    """Targets exactly on source cell centres receive the source's bits: -0.0, NaN, denormals included."""
    r = np.random.default_rng(5)
    for name, g in SOURCES.items():
        jj, ii = np.meshgrid(np.arange(g.ny), np.arange(g.nx), indexing="ij")
        xlat, xlon = (g.lat0 + jj * g.dlat).astype(F), (g.lon0 + ii * g.dlon).astype(F)
        plan, unf = np_plan(xlat, xlon, g)
        assert unf == 0
        src = nasty(r, g.nx * g.ny)
        src[:9] = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-40, -3e-42, HUGE, -HUGE], dtype=F)
        for mode in (BIL, NEAR):
            assert_same(np_regrid(plan, g, src, mode), src, "identity %s mode %d" % (name, mode))
        lib = _host()
        out = np.zeros(src.size, F)
        hp = np.zeros_like(plan)
        lib.regrid_plan(xlat.ctypes.data, xlon.ctypes.data, src.size, C.byref(g), None, 0, hp.ctypes.data)
        for mode in (BIL, NEAR):
            lib.regrid_values(hp.ctypes.data, src.size, C.byref(g), src.ctypes.data, out.ctypes.data, None, 0.0, -999.0, mode, None)
            assert_same(out, src, "host identity %s mode %d" % (name, mode))


def test_decomposition_plan_of_a_sub_tile_is_the_sub_block():
    """Each rank plans its own tile against the one global source: the plan of a sub-tile is the sub-block of the whole grid's plan."""
    for name in SOURCES:
        xlat, xlon = targets(name, 67, 5)
        v = mask(name, "random")
        whole, _ = np_plan(xlat, xlon, SOURCES[name], v, 2)
        whole = whole.reshape(6, 5, 67)
        lib = _host()
        for j0, j1, i0, i1 in ((0, 5, 0, 31), (0, 5, 31, 67), (1, 4, 13, 50)):
            sub, unf = np_plan(xlat[j0:j1, i0:i1], xlon[j0:j1, i0:i1], SOURCES[name], v, 2)
            want = np.ascontiguousarray(whole[:, j0:j1, i0:i1]).reshape(6, -1)
            assert_same_plan(sub, want, "%s sub-tile" % name)
            assert unf == (want[0] < 0).sum()
            la, lo = np.ascontiguousarray(xlat[j0:j1, i0:i1]), np.ascontiguousarray(xlon[j0:j1, i0:i1])
            hp = np.zeros_like(want)
            assert lib.regrid_plan(la.ctypes.data, lo.ctypes.data, la.size, C.byref(SOURCES[name]), v.ctypes.data, 2, hp.ctypes.data) == unf
            assert_same_plan(hp, want, "%s host sub-tile" % name)


def build():
    deps = [SRC, os.path.join(CSRC, "nmp_dev_regrid.hpp"), os.path.join(ROOT, "include", "noahmp_hip.h")]
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
    lib.regrid_plan.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.POINTER(abi.RegridSource), C.c_void_p, C.c_int, C.c_void_p]
    lib.regrid_plan.restype = C.c_long
    lib.regrid_values.argtypes = [C.c_void_p, C.c_long, C.POINTER(abi.RegridSource), C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float,
                                  C.c_int, C.c_void_p]
    lib.regrid_values.restype = None
    return lib


@pytest.mark.parametrize("name, ni, nj", plan_cases())
def test_host_compilation_of_the_plan_equals_numpy(name, ni, nj):
    """nmp_dev_regrid.hpp::regrid_plan_cell compiled for the host against the restatement, on the shapes of the GPU test."""
    lib = _host()
    for kind in MASKS:
        for radius in (0, 2):
            xlat, xlon, v, want, unf = plan_case(name, ni, nj, kind, radius)
            got = np.full_like(want, 7)
            n = lib.regrid_plan(xlat.ctypes.data, xlon.ctypes.data, ni * nj, C.byref(SOURCES[name]), v.ctypes.data if v is not None else None,
                                radius, got.ctypes.data)
            assert_same_plan(got, want, "%s %dx%d mask %s radius %d" % (name, ni, nj, kind, radius))
            assert n == unf


def value_cases(r, g, ncell):
    """A plan with every kind of column in it (restated plans of masked targets, plus hand-made columns), nasty sources."""
    nxny = g.nx * g.ny
    name = [k for k, s in SOURCES.items() if s is g][0]
    ni = ncell
    xlat, xlon = targets(name, ni, 1)
    plan, _ = np_plan(xlat, xlon, g, mask(name, "random", seed=ncell), 2)
    plan = plan.copy()
    w = plan[2:].view(F)
    hand = r.permutation(ncell)[:min(12, ncell)]
    for q, c in enumerate(hand):
        if q % 4 == 0:                                       # one corner only, on the last cell of the source
            plan[0, c], plan[1, c] = nxny - 1, nxny - 1
            w[:, c] = (1, 0, 0, 0)
        elif q % 4 == 1:                                     # no corner left
            plan[0, c] = 0
            w[:, c] = 0
        elif q % 4 == 2:                                     # weights that are not a partition of one, a negative zero among them
            plan[0, c] = int(r.integers(0, nxny - g.nx - 1))
            w[:, c] = (F(-0.0), F(2.5), F(-1.25), F(1e-40))
        else:                                                # the seam column (periodic) or the end of a row
            plan[0, c] = 2 * g.nx - 1
            w[:, c] = (0.25, 0.25, 0.25, 0.25)
    return plan, nasty(r, nxny)


@pytest.mark.parametrize("name", list(SOURCES))
def test_host_compilation_of_the_value_equals_numpy_and_reads_no_dropped_corner(name):
    lib = _host()
    g = SOURCES[name]
    r = np.random.default_rng(41)
    for ncell in (256, 335, 1):
        plan, src = value_cases(r, g, ncell)
        adjust = nasty(r, ncell)
        for mode in (BIL, NEAR):
            for adj, scale in ((None, 0.0), (adjust, -0.0065)):
                got = np.full(ncell, 7.0, F)
                reads = np.zeros(g.nx * g.ny, np.int32)
                lib.regrid_values(plan.ctypes.data, ncell, C.byref(g), src.ctypes.data, got.ctypes.data, adj.ctypes.data if adj is not None else None,
                                  scale, -999.0, mode, reads.ctypes.data)
                assert_same(got, np_regrid(plan, g, src, mode, adj, scale, -999.0), "%s n=%d mode %d" % (name, ncell, mode))
                if mode == BIL:                              # exactly the corners of non-zero weight were read
                    want = np.zeros_like(reads)
                    nx, nxny = g.nx, g.nx * g.ny
                    for c in range(ncell):
                        b = int(plan[0, c])
                        if b < 0 or b >= nxny:
                            continue
                        c1 = b + 1 - nx if (g.periodic_x and b % nx == nx - 1) else b + 1
                        idx = [b, c1, b + nx, c1 + nx]
                        ww = plan[2:, c].view(F)
                        if any(ww[k] != 0 and idx[k] >= nxny for k in range(1, 4)):
                            continue
                        for k in range(4):
                            if ww[k] != 0:
                                want[idx[k]] += 1
                    assert np.array_equal(reads, want)


def test_products_are_rounded_before_the_sums():
    """Never an FMA: a value whose fused and unfused results differ, through the host compilation."""
    lib = _host()
    g = SOURCES["plain"]
    plan = np.zeros((6, 1), np.int32)
    w = plan[2:].view(F)
    w[:, 0] = (F(1.0), F(1.0) + F(2.0) ** -12, 0, 0)
    src = np.zeros(35, F)
    src[0], src[1] = F(-1.0), F(1.0) + F(2.0) ** -12
    exact = float(w[0, 0]) * float(src[0]) + float(w[1, 0]) * float(src[1])         # what an FMA of the second product would keep: 2^-11 + 2^-24
    got = np.zeros(1, F)
    lib.regrid_values(plan.ctypes.data, 1, C.byref(g), src.ctypes.data, got.ctypes.data, None, 0.0, 0.0, BIL, None)
    want = np_regrid(plan, g, src, BIL)
    assert got[0] == want[0] == F(2.0) ** -11 and float(got[0]) != exact
    adj = np.array([src[1]], F)                                                      # src[near] + scale * adjust = -1 + (1 + 2^-12)^2
    lib.regrid_values(plan.ctypes.data, 1, C.byref(g), src.ctypes.data, got.ctypes.data, adj.ctypes.data, float(w[1, 0]), 0.0, NEAR, None)
    assert got[0] == np_regrid(plan, g, src, NEAR, adj, w[1, 0])[0] == F(2.0) ** -11


def test_bindings_regenerate_identically():
    """include/noahmp_hip.h, the Fortran types and interfaces and oracle/ref_harness_gen.f90 are what tools/gen_abi.py makes of
    abi_spec.py, with the regrid in them; NOAHMP_HIP_ABI_VERSION and the reference wrapper are untouched."""
    from tools import gen_abi
    for rel, text in (("include/noahmp_hip.h", gen_abi.c_header()), ("oracle/ref_harness_gen.f90", gen_abi.ref_harness()),
                      ("noahmp_amd/fortran/module_sf_noahmpdrv_hip.F90", gen_abi.fortran_shim()),
                      ("tests/fortran/shim_wrap_gen.f90", gen_abi.shim_wrap())):
        assert open(os.path.join(ROOT, rel)).read() == text, rel
    hdr = open(os.path.join(ROOT, "include", "noahmp_hip.h")).read()
    for word in ("noahmp_regrid_source", "noahmp_regrid_entry", "noahmp_hip_regrid_plan_size(", "noahmp_hip_regrid_plan_latlon(",
                 "noahmp_hip_forcing_regrid(", "NOAHMP_REGRID_BILINEAR", "NOAHMP_REGRID_NEAREST", "#define NOAHMP_HIP_ABI_VERSION 1\n"):
        assert word in hdr, word
    assert "noahmp_regrid" not in gen_abi.ref_harness()
    f90 = open(os.path.join(ROOT, "noahmp_amd", "fortran", "module_sf_noahmpdrv_hip.F90")).read()
    for name in ("noahmp_hip_regrid_plan_size", "noahmp_hip_regrid_plan_latlon", "noahmp_hip_forcing_regrid"):
        assert "bind(C, name='%s')" % name in f90, name
        assert name in abi.EXPORTED_SYMBOLS
    assert "type, bind(C) :: noahmp_regrid_source" in f90 and "type, bind(C) :: noahmp_regrid_entry" in f90
    assert (abi.REGRID_MODE["bilinear"], abi.REGRID_MODE["nearest"]) == (BIL, NEAR)
    assert abi.REGRID_PLANES == ("base", "near", "w0", "w1", "w2", "w3")


def test_ctypes_mirror_matches_the_compiled_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "noahmp_hip.h"\nint main(){'
                   'printf("%zu %zu %zu %zu %zu %zu %zu ", sizeof(noahmp_regrid_source), offsetof(noahmp_regrid_source, ny),'
                   'offsetof(noahmp_regrid_source, lon0), offsetof(noahmp_regrid_source, lat0), offsetof(noahmp_regrid_source, dlon),'
                   'offsetof(noahmp_regrid_source, dlat), offsetof(noahmp_regrid_source, periodic_x));'
                   'printf("%zu %zu %zu %zu %zu %zu %d", sizeof(noahmp_regrid_entry), offsetof(noahmp_regrid_entry, dst),'
                   'offsetof(noahmp_regrid_entry, adjust), offsetof(noahmp_regrid_entry, scale), offsetof(noahmp_regrid_entry, fill),'
                   'offsetof(noahmp_regrid_entry, mode), NOAHMP_REGRID_MAX_ENTRIES); return 0;}')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    S, E = abi.RegridSource, abi.RegridEntry
    assert out == [C.sizeof(S), S.ny.offset, S.lon0.offset, S.lat0.offset, S.dlon.offset, S.dlat.offset, S.periodic_x.offset,
                   C.sizeof(E), E.dst.offset, E.adjust.offset, E.scale.offset, E.fill.offset, E.mode.offset, 32]


def test_library_exports_the_regrid():
    if not os.path.exists(abi.LIB_PATH):
        from noahmp_amd import build as b
        b.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", abi.LIB_PATH]).decode()
    for name in ("noahmp_hip_regrid_plan_size", "noahmp_hip_regrid_plan_latlon", "noahmp_hip_forcing_regrid"):
        assert " T " + name in out, name


def _flang():
    for c in ("/opt/rocm/lib/llvm/bin/flang", "/opt/rocm/bin/amdflang"):
        if os.path.exists(c):
            return c
    return None


@pytest.mark.skipif(_flang() is None, reason="no flang")
def test_generated_fortran_types_and_interfaces_compile(tmp_path):
    """The regrid part of the generated module -- types, constants, interfaces -- compiles, and a caller of it type-checks."""
    from tools import gen_abi
    text = "\n".join(["module regrid_abi_check", "  use iso_c_binding", "  implicit none"] + gen_abi.regrid_f90_types() + ["  interface"] +
                     gen_abi.regrid_f90_interfaces() + ["  end interface", "contains", "  function go(plan, ncell, planes) result(rc)",
                                                        "    type(c_ptr), value :: plan", "    integer(c_int64_t), value :: ncell",
                                                        "    type(c_ptr), intent(in) :: planes(2)", "    type(noahmp_regrid_source) :: g",
                                                        "    type(noahmp_regrid_entry) :: e(1)", "    integer(c_int64_t) :: words",
                                                        "    integer(c_int32_t) :: unfilled", "    integer(c_int) :: rc",
                                                        "    g%nx = 464; g%ny = 224; g%lon0 = -124.9375d0; g%lat0 = 25.0625d0",
                                                        "    g%dlon = 0.125d0; g%dlat = 0.125d0; g%periodic_x = 0",
                                                        "    rc = noahmp_hip_regrid_plan_size(64, 8, words)",
                                                        "    rc = noahmp_hip_regrid_plan_latlon(planes(1), planes(2), 64, 8, g, c_null_ptr, 4, plan, words, unfilled, c_null_ptr)",
                                                        "    e(1)%src = planes(1); e(1)%dst = planes(2); e(1)%adjust = c_null_ptr",
                                                        "    e(1)%scale = 0.0; e(1)%fill = -1.e33; e(1)%mode = NOAHMP_REGRID_BILINEAR",
                                                        "    rc = noahmp_hip_forcing_regrid(plan, ncell, g, 1, e, c_null_ptr)",
                                                        "  end function go", "end module regrid_abi_check", ""])
    f = tmp_path / "regrid_abi_check.f90"
    f.write_text(text)
    subprocess.check_call([_flang(), "-c", str(f), "-o", str(tmp_path / "regrid_abi_check.o"), "-J", str(tmp_path)], cwd=str(tmp_path))


# ---------------------------------------------------------------------------------------------------------------- GPU
def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("name, ni, nj", plan_cases())
def test_gpu_plan_kernel_equals_numpy(engine, name, ni, nj):
    """noahmp_hip_regrid_plan_latlon against the restatement: every plane bit for bit, and the unfilled count."""
    import torch
    g = SOURCES[name]
    for kind in MASKS:
        for radius in (0, 2):
            xlat, xlon, v, want, unf = plan_case(name, ni, nj, kind, radius)
            plan, got_unf = engine.regrid_plan(_dev(xlat), _dev(xlon), g, valid=_dev(v) if v is not None else None, search_radius=radius)
            assert plan.numel() == 6 * ni * nj + 1
            got = plan[:6 * ni * nj].cpu().numpy().reshape(6, ni * nj)
            assert_same_plan(got, want, "%s %dx%d mask %s radius %d" % (name, ni, nj, kind, radius))
            assert got_unf == unf and int(plan[-1].item()) == unf
    torch.cuda.synchronize()


def _entries_case(r, g, ncell, n):
    """n entries over one plan: both modes, with and without adjust, differing scales and fills."""
    plan, _ = value_cases(r, g, ncell)
    nxny = g.nx * g.ny
    srcs = [nasty(r, nxny) for _ in range(n)]
    adjs = [nasty(r, ncell) if f % 3 != 1 else None for f in range(n)]
    modes = [NEAR if f % 4 == 3 else BIL for f in range(n)]
    scales = [F(-0.0065) if f % 2 else F(1.5) for f in range(n)]
    fills = [F(-999.0 - f) for f in range(n)]
    want = [np_regrid(plan, g, srcs[f], modes[f], adjs[f], scales[f], fills[f]) for f in range(n)]
    return plan, srcs, adjs, modes, scales, fills, want


def _run(engine, g, plan_d, ncell, srcs, dsts, adjs, modes, scales, fills):
    import torch
    torch.cuda.synchronize()
    engine.forcing_regrid(plan_d, ncell, g, [(srcs[f], dsts[f], modes[f], adjs[f], float(scales[f]), float(fills[f])) for f in range(len(srcs))])
    engine.stream_sync()


@pytest.mark.gpu
@pytest.mark.parametrize("name, ncell, n", [("plain", 256, 1), ("plain", 256, 8), ("north_first", 256, 32), ("periodic", 256, 8),
                                             ("plain", 335, 8), ("periodic", 335, 32), ("periodic", 1, 1), ("plain", 4, 8), ("plain", 1028, 32)])
def test_gpu_regrid_kernel_equals_numpy_on_both_paths(engine, name, ncell, n):
    """noahmp_hip_forcing_regrid against the restatement: n = 1, 8, 32 entries of both modes, with and without adjust, NaN / Inf / -0.0 /
    denormal sources.  256, 4 and 1028 columns take the four-columns-per-thread path (1028: a second, ragged workgroup), 335 and 1 the
    one-column path; the same call into destinations offset by one float takes the one-column path and must give the same bits."""
    import torch
    g = SOURCES[name]
    r = np.random.default_rng(1000 * n + ncell)
    plan, srcs, adjs, modes, scales, fills, want = _entries_case(r, g, ncell, n)
    plan_d = _dev(plan.reshape(-1))
    srcs_d = [_dev(s) for s in srcs]
    adjs_d = [_dev(a) if a is not None else None for a in adjs]
    pool = torch.full((n, ncell + 8), 7.0, dtype=torch.float32, device="cuda")
    for off in (0, 1):
        pool.fill_(7.0)
        dsts = [pool[f, 4 + off:4 + off + ncell] for f in range(n)] if ncell % 4 == 0 else [pool[f, off:off + ncell] for f in range(n)]
        if ncell % 4 == 0:
            assert all(d.data_ptr() % 16 == 4 * off for d in dsts)                       # offset 0: aligned, offset 1: not
        _run(engine, g, plan_d, ncell, srcs_d, dsts, adjs_d, modes, scales, fills)
        for f in range(n):
            assert_same(dsts[f].cpu().numpy(), want[f], "%s ncell %d entry %d of %d, offset %d" % (name, ncell, f, n, off))
        h = pool.cpu().numpy()
        lo = (4 + off) if ncell % 4 == 0 else off
        assert (h[:, :lo] == 7.0).all() and (h[:, lo + ncell:] == 7.0).all()            # nothing written beside the planes


@pytest.mark.gpu
def test_gpu_refusals_launch_nothing(engine):
    """n = 33 gives -107, a NULL plane or a mode out of range -105, with text; the destinations are unchanged."""
    import torch
    g = SOURCES["plain"]
    lib = engine.lib
    ncell = 256
    plan, _ = np_plan(*targets("plain", 64, 4), g)
    plan_d = _dev(plan.reshape(-1))
    src = _dev(nasty(np.random.default_rng(2), 35))
    dst = torch.full((33, ncell), 7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def call(n, e, grid=g, p=plan_d.data_ptr()):
        rc = lib.noahmp_hip_forcing_regrid(p, ncell, C.byref(grid), n, e, None)
        engine.stream_sync()
        return rc, lib.noahmp_hip_last_error().decode()
    e = engine.regrid_entries([(src, dst[f], "bilinear", None, 0.0, -1.0) for f in range(32)])
    e33 = (abi.RegridEntry * 33)()
    for f in range(33):
        e33[f].src, e33[f].dst, e33[f].mode = src.data_ptr(), dst[f].data_ptr(), BIL
    rc, msg = call(33, e33)
    assert rc == -107 and "entries" in msg
    rc, msg = call(-1, e)
    assert rc == -107
    for bad, what in (("mode", 2), ("mode", -1), ("src", None), ("dst", None)):
        keep = getattr(e[5], bad)
        setattr(e[5], bad, what)
        rc, msg = call(32, e)
        assert rc == -105 and "entry 5" in msg, (bad, rc, msg)
        setattr(e[5], bad, keep)
    rc, msg = call(32, e, p=None)
    assert rc == -105 and "plan" in msg
    rc, msg = call(32, e, grid=source(1, 5, 0.0, 0.0, 1.0, 1.0))
    assert rc == -105 and "nx" in msg
    assert (dst.cpu().numpy() == 7.0).all()
    rc, msg = call(0, e)
    assert rc == 0 and (dst.cpu().numpy() == 7.0).all()
    # the plan call: a source grid, a radius or a workspace that cannot be
    xl = _dev(np.zeros((4, 64), F))
    unf = C.c_int32(-5)
    for grid, radius, words in ((source(7, 1, 0.0, 0.0, 1.0, 1.0), 2, plan_d.numel() + 1), (source(7, 5, 0.0, 0.0, 0.0, 1.0), 2, plan_d.numel() + 1),
                                (g, 17, plan_d.numel() + 1), (g, -1, plan_d.numel() + 1), (g, 2, plan_d.numel())):
        ws = torch.zeros(plan_d.numel() + 1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        rc = lib.noahmp_hip_regrid_plan_latlon(xl.data_ptr(), xl.data_ptr(), 64, 4, C.byref(grid), None, radius, ws.data_ptr(), words,
                                               C.byref(unf), None)
        assert rc == -105 and unf.value == -5 and (ws.cpu().numpy() == 0).all(), (radius, words, rc)
    rc, msg = call(32, e)
    assert rc == 0
    want = np_regrid(plan, g, src.cpu().numpy(), BIL, fill=-1.0)
    assert_same(dst[31].cpu().numpy(), want, "after the refusals")


@pytest.mark.gpu
@pytest.mark.parametrize("ncell", [256, 255])
def test_gpu_hand_made_plan_cannot_read_outside_the_source(engine, ncell):
    """base = nx*ny, near = nx*ny, negative indices, and corners of non-zero weight behind the last row give fill.  The source tensor has 64
    spare words behind it (filled with a value no source cell has), so an implementation without the check reads them and fails the
    comparison instead of faulting."""
    import torch
    for name in ("plain", "periodic"):
        g = SOURCES[name]
        nx, nxny = g.nx, g.nx * g.ny
        r = np.random.default_rng(ncell)
        plan, _ = value_cases(r, g, ncell)
        w = plan[2:].view(F)
        bad = r.permutation(ncell)[:40]
        for q, c in enumerate(bad):
            kind = q % 8
            if kind == 0:
                plan[0, c] = plan[1, c] = nxny
            elif kind == 1:
                plan[0, c] = plan[1, c] = -1
            elif kind == 2:
                plan[0, c] = plan[1, c] = -(2 ** 31)
            elif kind == 3:
                plan[0, c] = plan[1, c] = 2 ** 31 - 1
            elif kind == 4:                                  # last row: corners 2 and 3 lie behind the source
                plan[0, c], plan[1, c] = nxny - nx + 1, nxny + 3
                w[:, c] = (0.25, 0.25, 0.25, 0.25)
            elif kind == 5:                                  # last cell: corner 1 (not periodic) / corners 2, 3 lie behind it
                plan[0, c], plan[1, c] = nxny - 1, nxny + 63
                w[:, c] = (0.5, 0.5, 0, 0) if not g.periodic_x else (0.5, 0, 0, 0.5)
            elif kind == 6:                                  # the same cells with the outside corners dropped: safe, not filled
                plan[0, c], plan[1, c] = nxny - nx + 1, nxny - 1
                w[:, c] = (0.75, 0.25, 0, 0)
            else:
                plan[0, c], plan[1, c] = nxny + 17, nxny + 17
                w[:, c] = (1, 0, 0, 0)
        src = np.full(nxny + 64, 12345.0, F)
        src[:nxny] = r.uniform(-5.0, 5.0, nxny).astype(F)
        adj = r.uniform(-1.0, 1.0, ncell).astype(F)
        want = [np_regrid(plan, g, src, BIL, None, 0.0, -77.0), np_regrid(plan, g, src, NEAR, adj, 2.0, -78.0),
                np_regrid(plan, g, src, BIL, adj, 2.0, np.nan)]
        assert all((x == F(-77.0)).sum() >= 25 for x in want[:1]) and not any((np.abs(x) > 100).any() for x in want[:2])
        src_d = _dev(src)
        dst = torch.full((3, ncell + 8), 7.0, dtype=torch.float32, device="cuda")
        dsts = [dst[f, :ncell] for f in range(3)]
        adj_d = _dev(adj)
        _run(engine, g, _dev(plan.reshape(-1)), ncell, [src_d[:nxny]] * 3, dsts, [None, adj_d, adj_d], [BIL, NEAR, BIL], [0.0, 2.0, 2.0],
             [-77.0, -78.0, np.nan])
        for f in range(3):
            assert_same(dsts[f].cpu().numpy(), want[f], "%s hand-made plan, entry %d" % (name, f))


@pytest.mark.gpu
def test_gpu_column_order_permuted_plan_gives_the_permuted_result(engine):
    """The six plan planes and the adjust plane of a 64 x 8 tile, permuted by a random permutation with noahmp_hip_gather_fields, give the
    permuted result of the tile-order call: the regrid knows nothing about column order."""
    import torch
    ni, nj = 64, 8
    n = ni * nj
    r = np.random.default_rng(77)
    for name in ("plain", "periodic"):
        g = SOURCES[name]
        xlat, xlon = targets(name, ni, nj)
        v = mask(name, "random")
        plan, unf = engine.regrid_plan(_dev(xlat), _dev(xlon), g, valid=_dev(v), search_radius=2)
        perm = r.permutation(n).astype(np.int32)
        perm_d = _dev(perm)
        adj = _dev(nasty(r, n))
        srcs = [_dev(nasty(r, g.nx * g.ny)) for _ in range(4)]
        modes, adjs = [BIL, NEAR, BIL, NEAR], [adj, adj, None, None]
        tile = [torch.full((n,), 7.0, dtype=torch.float32, device="cuda") for _ in range(4)]
        _run(engine, g, plan, n, srcs, tile, adjs, modes, [0.5] * 4, [-9.0] * 4)
        pplan = torch.zeros_like(plan)
        padj = torch.zeros_like(adj)
        torch.cuda.synchronize()
        engine.gather([pplan[k * n:(k + 1) * n] for k in range(6)] + [padj], [plan[k * n:(k + 1) * n] for k in range(6)] + [adj], perm_d, ni, nj)()
        engine.stream_sync()
        out = [torch.full((n,), 7.0, dtype=torch.float32, device="cuda") for _ in range(4)]
        _run(engine, g, pplan, n, srcs, out, [padj if a is not None else None for a in adjs], modes, [0.5] * 4, [-9.0] * 4)
        hplan = plan[:6 * n].cpu().numpy().reshape(6, n)
        for f in range(4):
            t = tile[f].cpu().numpy()
            assert_same(t, np_regrid(hplan, g, srcs[f].cpu().numpy(), modes[f], adj.cpu().numpy() if adjs[f] is not None else None, 0.5, -9.0),
                        "%s tile order, entry %d" % (name, f))
            assert_same(out[f].cpu().numpy(), t[perm], "%s permuted, entry %d" % (name, f))


# ---- the chain: coarse records -> ForcingRegrid.record -> forcing_interpolate_prep -> noahmplsm, two steps
COARSE = dict(t=(283.0, 291.0), q=(5e-3, 7e-3), u=(2.0, 4.0), v=(0.0, 2.0), p=(9.4e4, 9.6e4), lw=(320.0, 340.0), sw=(500.0, 800.0),
              pcp=(0.0, 5e-4), fpar=(0.3, 0.9), lai=(0.5, 4.0))


def _chain(engine, tables, feed, sort=False):
    """Two steps of a 64 x 8 synthetic tile.  feed(k, names) -> dict of fine device planes of coarse record k (k = 0, 1, 2)."""
    import torch
    T, tb = tables
    ni, nj = 64, 8
    s = synth.mixed_small(tb, ni=ni, nj=nj)
    synth.first_step_fixups(s)
    synth.diurnal_forcing(s, 12, t_offset=s.t_offset)
    d = s.to_device("cuda:0")
    lon = _dev(CHAIN_LON)
    rain = torch.zeros((nj, ni), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    if sort:
        engine.sort_store(d)
        feed.follow(d)
        lon = lon.reshape(-1)[d.sort_perm.long()].reshape(nj, ni).contiguous()
        torch.cuda.synchronize()
    for it in (1, 2):
        ra, rb = feed(it - 1), feed(it)
        torch.cuda.synchronize()
        jul = engine.forcing_interpolate_prep(d, ra, rb, 1800, 10800, rain, lon, 171, 18, 30 * (it - 1), 0, scale_vegfra=True, first_step=(it == 1))
        st = engine.noahmplsm(d, it, 2000, jul)
        assert st.code == 0
    return d


CHAIN_SRC = source(6, 5, -100.5, 34.5, 0.25, 0.25)
_jj, _ii = np.meshgrid(np.arange(8), np.arange(64), indexing="ij")
CHAIN_LAT = (34.6 + 0.1 * _jj + 0.001 * _ii).astype(F)
CHAIN_LON = (-100.4 + 0.017 * _ii - 0.003 * _jj).astype(F)


@pytest.mark.gpu
def test_gpu_chain_equals_the_chain_fed_with_restated_fine_records(engine, tables):
    """Two coarse records through ForcingRegrid.record, forcing_interpolate_prep and noahmplsm for two steps, against the same chain fed
    with fine records made by the restatement and uploaded: every INOUT and OUT array bit-identical.  T carries a lapse-rate adjustment,
    precipitation is taken from the nearest cell.  The same through a sorted store (ForcingRegrid.follow) returns the same columns."""
    import torch
    from noahmp_amd.regrid import ForcingRegrid
    from tools.compare import exact_check
    g = CHAIN_SRC
    r = np.random.default_rng(9)
    names = list(COARSE)
    coarse = [{k: r.uniform(lo, hi, g.nx * g.ny).astype(F).reshape(g.ny, g.nx) for k, (lo, hi) in COARSE.items()} for _ in range(3)]
    z_src = r.uniform(200.0, 900.0, g.nx * g.ny).astype(F).reshape(g.ny, g.nx)
    z_model = r.uniform(100.0, 1500.0, (8, 64)).astype(F)
    plan, unf = np_plan(CHAIN_LAT, CHAIN_LON, g)
    assert unf == 0
    adj = z_model.ravel() - np_regrid(plan, g, z_src.ravel(), BIL)
    modes = {"pcp": "nearest"}

    def restated(k):
        out = {}
        for nm in names:
            a, sc = (adj, F(-0.0065)) if nm == "t" else (None, 0.0)
            out[nm] = _dev(np_regrid(plan, g, coarse[k][nm].ravel(), NEAR if nm in modes else BIL, a, sc, np.nan).reshape(8, 64))
        return out
    ref = _chain(engine, tables, restated).to_host()

    rg = ForcingRegrid(engine, _dev(CHAIN_LAT), _dev(CHAIN_LON), g)
    assert rg.unfilled == 0
    rg.set_adjust("t", _dev(z_model) - rg.regrid_plane(_dev(z_src)), scale=-0.0065)
    cd = [{k: _dev(v) for k, v in c.items()} for c in coarse]
    torch.cuda.synchronize()
    seen = []

    class Feed:
        def __call__(self, k):
            rec = rg.record(cd[k], modes=modes)
            seen.append(rec)
            return rec
        follow = staticmethod(rg.follow)
    got = _chain(engine, tables, Feed()).to_host()
    ok, lines = exact_check(ref, got)
    assert ok, "\n".join(lines)
    assert seen[0]["t"].data_ptr() == seen[2]["t"].data_ptr() != seen[1]["t"].data_ptr()      # two sets, used alternately
    assert_same(seen[3]["t"].cpu().numpy(), restated(2)["t"].cpu().numpy(), "record 2")

    # the sorted layout: the same columns at other positions
    rg2 = ForcingRegrid(engine, _dev(CHAIN_LAT), _dev(CHAIN_LON), g)
    rg2.set_adjust("t", _dev(z_model) - rg2.regrid_plane(_dev(z_src)), scale=-0.0065)

    class Feed2:
        def __call__(self, k):
            return rg2.record(cd[k], modes=modes)
        follow = staticmethod(rg2.follow)
    ds = _chain(engine, tables, Feed2(), sort=True)
    perm = ds.sort_perm.cpu().numpy()
    hs = ds.to_host()
    for k in ("tsk", "hfx", "tgxy", "smois", "t2mvxy"):
        x, y = np.asarray(ref.a[k]), np.asarray(hs.a[k])
        if x.ndim == 3:
            x, y = np.moveaxis(x, 1, 0).reshape(x.shape[1], -1), np.moveaxis(y, 1, 0).reshape(y.shape[1], -1)
            assert_same(y, x[:, perm], "sorted chain " + k)
        else:
            assert_same(y.ravel(), x.ravel()[perm], "sorted chain " + k)
