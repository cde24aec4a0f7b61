"""Runoff routing on the device: D8 directions, upstream bytes, upstream counts and cell-to-cell linear reservoirs (noahmp_hip_flow_terrain,
noahmp_hip_flow_inmask, noahmp_hip_flow_accumulate, noahmp_hip_route_runoff; nmp_dev_routing.hpp).

No reference routine stands behind the calls; the contract is the text in include/noahmp_hip.h.  np_flow_dir, np_inmask, np_accumulate and
np_route restate it in numpy, one rounded float32 operation per line.  Everything is compared with the restatement bit for bit
(test_regrid.assert_same: equal bits, or both NaN): the per-cell functions compiled for the host in both forms of the neighbour loads, the
four kernels of the library and of the variant library that loads only the set bits' neighbours, and engine runs through FlowNetwork.  A tolerance
appears only in the budget checks; where it comes from is counted there."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from noahmp_amd import abi
import test_regrid as tr
import test_shadow as tsh
import test_skyview as tsv
from test_regrid import F, assert_same, nasty

ROOT = tr.ROOT
CSRC = tr.CSRC
SRC = os.path.join(ROOT, "tests", "host_emul", "routing_check.hip")
LIB = os.path.join(ROOT, "tests", "host_emul", "librouting_check.so")
LIB_MASKED = os.path.join(CSRC, "variants", "lib_route_masked.so")        # the library with -DNMP_ROUTE_LOAD_ALL=0
WINDOWS = [(1, 1), (7, 1), (1, 7), (3, 3), (65, 5), (67, 35)]             # (ni, nj): a lone cell, one row, one column, the 64 / 65 lane boundary
CUT = (70, 130)                                                          # cut 2 x 2
DX, DY = 1000.0, 1500.0                                                  # dx != dy
POISON = 7.0
EPS = 2.0 ** -24
U32 = np.uint32
DI = (1, 1, 0, -1, -1, -1, 0, 1)                                          # neighbour k = 1..8 at index k-1: E NE N NW W SW S SE
DJ = (0, 1, 1, 1, 0, -1, -1, -1)
NOT_OWNED = (-2, -5, -2 ** 31)                                            # and every value >= ncol


def opp(k):
    return ((k + 3) & 7) + 1


# ---------------------------------------------------------------------------------------------------------------- the restatement
def neighbour(a, k, fill=0):
    """(plane of neighbour k's values, fill where it lies outside the window; the mask of the cells whose neighbour k lies inside)."""
    nj, ni = a.shape
    di, dj = DI[k - 1], DJ[k - 1]
    out = np.full(a.shape, fill, a.dtype)
    inside = np.zeros(a.shape, bool)
    j0, j1, i0, i1 = max(0, -dj), nj - max(0, dj), max(0, -di), ni - max(0, di)
    if j1 > j0 and i1 > i0:
        out[j0:j1, i0:i1] = a[j0 + dj:j1 + dj, i0 + di:i1 + di]
        inside[j0:j1, i0:i1] = True
    return out, inside


def np_inverse_distances(dx, dy):
    dx, dy = F(dx), F(dy)
    inv_x = F(F(1.0) / dx)
    inv_y = F(F(1.0) / dy)
    dx2 = F(dx * dx)
    dy2 = F(dy * dy)
    d2 = F(dx2 + dy2)
    d = F(np.sqrt(d2))
    inv_d = F(F(1.0) / d)
    return inv_x, inv_y, inv_d


def np_slopes(height, dx, dy):
    """s of the header text per k (list of 8 planes) and the inside masks."""
    z = np.asarray(height, F)
    inv_x, inv_y, inv_d = np_inverse_distances(dx, dy)
    out = []
    with np.errstate(all="ignore"):
        for k in range(1, 9):
            zn, inside = neighbour(z, k)
            inv = (inv_y if k in (3, 7) else inv_x) if k & 1 else inv_d
            drop = z - zn
            s = drop * inv
            assert s.dtype == F
            out.append((s, inside))
    return out


def np_flow_dir(height, dx, dy):
    """noahmp_hip_flow_terrain over a window."""
    z = np.asarray(height, F)
    best = np.zeros(z.shape, np.uint8)
    sbest = np.zeros(z.shape, F)
    with np.errstate(all="ignore"):
        for k, (s, inside) in enumerate(np_slopes(z, dx, dy), start=1):
            win = inside & (s > sbest)
            best = np.where(win, np.uint8(k), best)
            sbest = np.where(win, s, sbest)
    return best.astype(np.uint8)


def np_inmask(dirp):
    """noahmp_hip_flow_inmask over a window."""
    d = np.asarray(dirp, np.uint8)
    m = np.zeros(d.shape, np.uint8)
    for k in range(1, 9):
        dn, inside = neighbour(d, k)
        m |= np.where(inside & (dn == opp(k)), np.uint8(1 << (k - 1)), np.uint8(0)).astype(np.uint8)
    return m


def np_accumulate(inmask, acc_old):
    """One pass of noahmp_hip_flow_accumulate: (acc_new, changed)."""
    m = np.asarray(inmask, np.uint8)
    old = np.asarray(acc_old, U32)
    new = np.ones(m.shape, U32)
    for k in range(1, 9):
        an, inside = neighbour(old, k)
        new = (new + np.where(inside & ((m >> (k - 1)) & 1).astype(bool), an, U32(0))).astype(U32)
    return new, int((new != old).any())


def np_upstream(inmask, max_pass=100000):
    """Passes until nothing changes: (acc, passes made, the last one included)."""
    acc = np.ones(np.asarray(inmask).shape, U32)
    for p in range(1, max_pass + 1):
        acc, changed = np_accumulate(inmask, acc)
        if not changed:
            return acc, p
    raise AssertionError("no fixed point")


def np_route(x, out_old, out_new, storage):
    """One call of noahmp_hip_route_runoff over the window of x (a dict of the block's members): (storage', out_new')."""
    m = np.asarray(x["inmask"], np.uint8)
    col = np.asarray(x["col_index"], np.int64)
    ncol = int(x["ncol"])
    owned = (col >= -1) & (col < ncol)
    local = owned & (col >= 0)
    scale = F(x["scale"])
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
        o = s1 * np.asarray(x["release"], F)
        snew = s1 - o
    assert all(t.dtype == F for t in (q, xs, v, sv, s1, o, snew))
    return np.where(owned, snew, storage).astype(F), np.where(owned, o, out_new).astype(F)


def np_run(x, storage, out, nstep):
    """nstep calls, ping-ponging two out planes that both start as `out` (cells that are not owned keep what they hold)."""
    planes = [np.array(out, F), np.array(out, F)]
    storage = np.array(storage, F)
    cur = 0
    for _ in range(nstep):
        storage, planes[1 - cur] = np_route(x, planes[cur], planes[1 - cur], storage)
        cur = 1 - cur
    return storage, planes[cur]


# ---------------------------------------------------------------------------------------------------------------- the inputs
DX_TIE, DY_TIE = 3.0, 4.0                                                # distances 3, 4, 5: 3*fl(1/3) = 4*fl(1/4) = 5*fl(1/5) = 1.0f


def staircase():
    """A 3 x 3 patch per pair k1 < k2 of neighbours, 4 cells apart on a plain of 60 m: neighbour k1 and k2 lie m * their distance lower,
    so both have s = m exactly and the pair ties; the other neighbours are level.  Returns (height, [(i, j, k1, k2)])."""
    pairs = [(a, b) for a in range(1, 9) for b in range(a + 1, 9)]
    assert len(pairs) == 28
    ni, nj = 7 * 4 + 1, 4 * 4 + 1
    z = np.full((nj, ni), 60.0, F)
    where = []
    length = lambda k: (DY_TIE if k in (3, 7) else DX_TIE) if k & 1 else 5.0      # noqa: E731
    for n, (k1, k2) in enumerate(pairs):
        i, j = 2 + 4 * (n % 7), 2 + 4 * (n // 7)
        m = 1 + n % 3
        for k in (k1, k2):
            z[j + DJ[k - 1], i + DI[k - 1]] = 60.0 - m * length(k)
        where.append((i, j, k1, k2))
    return z, where


def terrain_cases(ni, nj):
    """(name, height, dx, dy)."""
    out = [("hills", tsh.terrain(ni, nj), DX, DY), ("hills dx=dy", tsh.terrain(ni, nj), DX, DX), ("plain", np.full((nj, ni), 812.5, F), DX, DY),
           ("plain -0", np.full((nj, ni), -0.0, F), DX, DY), ("nasty", tsv.terrain_of(ni, nj, "nasty"), DX, DY)]
    return out


def random_dir(ni, nj, seed=0):
    """Directions with bytes above 8 among them."""
    r = np.random.default_rng(100 + ni * 13 + nj + seed)
    d = r.integers(0, 9, (nj, ni)).astype(np.uint8)
    wild = r.random((nj, ni)) < 0.2
    d[wild] = r.choice(np.array([9, 13, 16, 128, 200, 255], np.uint8), int(wild.sum()))
    return d


def col_indices(ni, nj):
    """(name, col_index plane, ncol): identity, a permutation, and a mix with cells without local input and cells that are not owned."""
    ncell = ni * nj
    r = np.random.default_rng(ni * 1000 + nj)
    ident = np.arange(ncell, dtype=np.int32).reshape(nj, ni)
    perm = r.permutation(ncell).astype(np.int32).reshape(nj, ni)
    mix = perm.copy()
    pick = r.random((nj, ni))
    mix[pick < 0.2] = -1
    bad = (pick >= 0.2) & (pick < 0.45)
    mix[bad] = r.choice(np.array(NOT_OWNED + (ncell, ncell + 3, 2 ** 31 - 1), np.int64), int(bad.sum())).astype(np.int32)
    return [("identity", ident, ncell), ("permutation", perm, ncell), ("mix", mix, ncell)]


def route_operands(ni, nj, which, seed=0):
    """area, release, storage, out, runoff_a, runoff_b of a window and its ni*nj columns: physical or with NaN / Inf / denormal words."""
    ncell = ni * nj
    r = np.random.default_rng(4000 + ncell + len(which) + seed)
    phys = dict(area=r.uniform(0.5e6, 1.5e6, (nj, ni)).astype(F), release=r.uniform(0.0, 1.0, (nj, ni)).astype(F),
                storage=r.uniform(0.0, 5.0e3, (nj, ni)).astype(F), out=r.uniform(0.0, 2.0e3, (nj, ni)).astype(F),
                runoff_a=r.uniform(0.0, 2.0e-3, ncell).astype(F), runoff_b=r.uniform(0.0, 1.0e-3, ncell).astype(F))
    phys["release"][r.random((nj, ni)) < 0.1] = 0.0
    phys["release"][r.random((nj, ni)) < 0.1] = 1.0
    if which == "physical":
        return phys
    nas = {k: nasty(r, v.size).reshape(v.shape) for k, v in phys.items()}
    pick = {k: r.random(v.shape) < 0.3 for k, v in phys.items()}
    return {k: np.where(pick[k], nas[k], phys[k]).astype(F) for k in phys}


def hills_network(ni, nj):
    d = np_flow_dir(tsh.terrain(ni, nj), DX, DY)
    return d, np_inmask(d)


# ---------------------------------------------------------------------------------------------------------------- CPU
def build():
    """The host checker: nmp_dev_routing.hpp compiled for the CPU.  Needs nothing of the engine library."""
    deps = [SRC, os.path.join(CSRC, "nmp_dev_routing.hpp"), os.path.join(ROOT, "include", "noahmp_hip.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off",
                               "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), SRC, "-o", LIB])


def build_variant():
    """The variant library that loads only the set bits' neighbours: one translation unit compiled again, linked with the library's others."""
    from noahmp_amd import build as b
    b.build_unit_variant("noahmp_routing.hip", ["-DNMP_ROUTE_LOAD_ALL=0"], LIB_MASKED)


@functools.lru_cache(maxsize=None)
def _host():
    build()
    try:
        import torch  # noqa: F401  (map torch's HIP runtime first, noahmp_amd/abi.py::load_library)
    except ImportError:
        pass
    lib = C.CDLL(LIB)
    V, Fl, I = C.c_void_p, C.c_float, C.c_int
    lib.flow_inverse_distances.argtypes = [Fl, Fl, V]
    lib.flow_terrain_cells.argtypes = [I, I, V, Fl, Fl, V]
    lib.flow_inmask_cells.argtypes = [I, I, V, V]
    lib.flow_accumulate_passes.argtypes = [I, I, V, V, V, I, V]
    lib.flow_accumulate_passes.restype = I
    lib.route_cells.argtypes = [I, I, V, V, V, V, V, V, V, V, V, Fl, C.c_long, I]
    lib.flow_inverse_distances.restype = lib.flow_terrain_cells.restype = lib.flow_inmask_cells.restype = lib.route_cells.restype = None
    return lib


def _p(a):
    return a.ctypes.data if a is not None else None


def _c(a, dtype=F):
    return np.ascontiguousarray(a, dtype)


def host_flow_dir(height, dx, dy):
    z = _c(height)
    nj, ni = z.shape
    d = np.full(z.shape, 99, np.uint8)
    _host().flow_terrain_cells(ni, nj, _p(z), float(dx), float(dy), _p(d))
    return d


def host_inmask(dirp):
    d = _c(dirp, np.uint8)
    nj, ni = d.shape
    m = np.full(d.shape, 0xEE, np.uint8)
    _host().flow_inmask_cells(ni, nj, _p(d), _p(m))
    return m


def host_accumulate(inmask, acc, npass):
    m = _c(inmask, np.uint8)
    nj, ni = m.shape
    a, b = _c(acc, U32).copy(), np.zeros(m.shape, U32)
    changed = np.zeros(max(npass, 1), U32)
    which = _host().flow_accumulate_passes(ni, nj, _p(m), _p(a), _p(b), int(npass), _p(changed))
    return (a, b)[which], changed[:npass]


def host_run(x, storage, out, nstep, load_all):
    m = _c(x["inmask"], np.uint8)
    nj, ni = m.shape
    col, area, rel = _c(x["col_index"], np.int32), _c(x["area"]), _c(x["release"])
    ra = _c(x["runoff_a"])
    rb = _c(x["runoff_b"]) if x.get("runoff_b") is not None else None
    planes = [_c(out).copy(), _c(out).copy()]
    storage = _c(storage).copy()
    cur = 0
    for _ in range(nstep):
        _host().route_cells(ni, nj, _p(m), _p(col), _p(area), _p(rel), _p(storage), _p(planes[cur]), _p(planes[1 - cur]), _p(ra), _p(rb),
                            float(x["scale"]), int(x["ncol"]), int(load_all))
        cur = 1 - cur
    return storage, planes[cur]


def test_neighbour_numbering_and_inverse_distances():
    """k = 1..8 is E, NE, N, NW, W, SW, S, SE with j towards north, and opp(k) = ((k+3) & 7) + 1; the host's three reciprocal distances
    are the restated ones (3, 4, 5: every product with its own distance is exactly 1)."""
    from noahmp_amd.abi_spec import FLOW_NEIGHBOURS
    assert [(k, di, dj) for k, di, dj, _ in FLOW_NEIGHBOURS] == [(k, DI[k - 1], DJ[k - 1]) for k in range(1, 9)]
    assert abi.FLOW_DI == DI and abi.FLOW_DJ == DJ
    for k in range(1, 9):
        o = opp(k)
        assert (DI[o - 1], DJ[o - 1]) == (-DI[k - 1], -DJ[k - 1]) and 1 <= o <= 8
    for dx, dy in ((DX, DY), (DX_TIE, DY_TIE), (1.0, 1.0), (90.0, 30.0)):
        got = np.zeros(3, F)
        _host().flow_inverse_distances(dx, dy, _p(got))
        assert_same(got, np.array(np_inverse_distances(dx, dy), F), "inverse distances %g %g" % (dx, dy))
    ix, iy, idg = np_inverse_distances(DX_TIE, DY_TIE)
    assert F(F(3.0) * ix) == 1 and F(F(4.0) * iy) == 1 and F(F(5.0) * idg) == 1
    # a single lower neighbour k gives direction k: the offsets of the compiled functions are those of the table
    for k in range(1, 9):
        z = np.full((3, 3), 10.0, F)
        z[1 + DJ[k - 1], 1 + DI[k - 1]] = 9.0
        assert host_flow_dir(z, DX, DY)[1, 1] == k and np_flow_dir(z, DX, DY)[1, 1] == k
        m = host_inmask(host_flow_dir(z, DX, DY))
        assert m[1 + DJ[k - 1], 1 + DI[k - 1]] & (1 << (opp(k) - 1)), "the lower cell has the centre upstream, in the opposite direction"
        assert m[1, 1] == 0


@pytest.mark.parametrize("ni, nj", WINDOWS + [CUT])
def test_host_directions_equal_the_restatement(ni, nj):
    """flow_dir_cell compiled for the host against np_flow_dir: hills, dx = dy and dx != dy, plains (every direction 0), terrain with
    NaN / Inf / denormal words.  No cell points out of the window; every accepted direction descends strictly."""
    for name, z, dx, dy in terrain_cases(ni, nj):
        want = np_flow_dir(z, dx, dy)
        assert_same_bytes(host_flow_dir(z, dx, dy), want, "%dx%d %s" % (ni, nj, name))
        assert want.max() <= 8
        if name.startswith("plain"):
            assert (want == 0).all()
        for k in range(1, 9):
            zn, inside = neighbour(z, k, fill=F(np.inf))
            assert inside[want == k].all()
            assert (z[want == k] > zn[want == k]).all(), "strict descent"
    if (ni, nj) == (67, 35):
        d = np_flow_dir(tsh.terrain(ni, nj), DX, DY)
        assert len(np.unique(d)) == 9 and 0.001 < (d == 0).mean() < 0.2, "the hills use every direction and have a few pits"


def assert_same_bytes(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    bad = a != b
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError("%s: %d of %d values differ, first at %s: %r vs %r" % (what, bad.sum(), bad.size, i, a[i], b[i]))


def test_staircase_ties_go_to_the_first_neighbour():
    """Every pair of neighbours ties somewhere (s equal in all bits and the largest of the cell); the direction is the smaller k."""
    z, where = staircase()
    slopes = np_slopes(z, DX_TIE, DY_TIE)
    want = np_flow_dir(z, DX_TIE, DY_TIE)
    for i, j, k1, k2 in where:
        s = [slopes[k - 1][0][j, i] for k in range(1, 9)]
        assert s[k1 - 1] == s[k2 - 1] == max(s) > 0 and sorted(s)[-3] == 0, (k1, k2, s)
        assert want[j, i] == k1
    assert_same_bytes(host_flow_dir(z, DX_TIE, DY_TIE), want, "staircase")


def test_a_nan_never_wins():
    z = np.array([[np.nan, np.nan, np.nan], [np.nan, 9, 8.5], [np.nan, np.inf, np.nan]], F)
    assert np_flow_dir(z, DX, DX)[1, 1] == 1 and host_flow_dir(z, DX, DX)[1, 1] == 1
    z = np.full((3, 3), np.nan, F)
    z[1, 1] = 3.0
    assert (np_flow_dir(z, DX, DX) == 0).all() and (host_flow_dir(z, DX, DX) == 0).all()
    z = np.full((3, 3), 1.0, F)
    z[1, 1] = np.nan                                                     # a NaN cell has no direction and nobody points at it
    assert (host_flow_dir(z, DX, DX) == 0).all()


@pytest.mark.parametrize("ni, nj", WINDOWS + [CUT])
def test_host_inmask_equals_the_restatement(ni, nj):
    """flow_inmask_cell against np_inmask on the hills' directions and on random bytes, values above 8 among them: those set no bit."""
    for name, d in (("hills", hills_network(ni, nj)[0]), ("random", random_dir(ni, nj))):
        want = np_inmask(d)
        assert_same_bytes(host_inmask(d), want, "%dx%d %s" % (ni, nj, name))
        legal = np.where(d > 8, 0, d).astype(np.uint8)
        assert_same_bytes(np_inmask(legal), want, "a byte above 8 counts as 0")
        assert int(np.unpackbits(want).sum()) == int((legal > 0).sum() - points_outside(legal)), "one bit per cell that points at a cell of the window"
    if ni * nj == 1:
        assert host_inmask(np.array([[3]], np.uint8))[0, 0] == 0


def points_outside(d):
    n = 0
    for k in range(1, 9):
        _, inside = neighbour(d, k)
        n += int(((d == k) & ~inside).sum())
    return n


@pytest.mark.parametrize("ni, nj", WINDOWS + [CUT])
def test_host_accumulate_equals_the_restatement(ni, nj):
    """One pass from a random plane, and passes up to the fixed point, against np_accumulate; the flag of every pass; a random inmask
    (bits that point out of the window are ignored); words near 2^32 wrap."""
    d, m = hills_network(ni, nj)
    r = np.random.default_rng(ni + 31 * nj)
    start = r.integers(0, 2 ** 32, (nj, ni), dtype=np.uint64).astype(U32)
    for name, mask in (("hills", m), ("random", r.integers(0, 256, (nj, ni)).astype(np.uint8))):
        want, flag = np_accumulate(mask, start)
        got, changed = host_accumulate(mask, start, 1)
        assert_same(got, want, "%dx%d %s: one pass" % (ni, nj, name))
        assert int(changed[0]) == flag
    acc, passes = np_upstream(m)
    got, changed = host_accumulate(m, np.ones((nj, ni), U32), passes)
    assert_same(got, acc, "%dx%d: %d passes" % (ni, nj, passes))
    assert list(changed) == [1] * (passes - 1) + [0]
    # strict descent: every cell drains through exactly one cell without a direction
    assert int(acc[d == 0].astype(np.int64).sum()) == ni * nj
    assert acc.min() == 1 and passes <= ni + nj
    print("%d x %d hills: %d passes, largest count %d, %d outlets" % (ni, nj, passes, acc.max(), (d == 0).sum()))


def _block(ni, nj, inmask, col, ncol, ops, rb=True, scale=3.6):
    return dict(inmask=inmask, col_index=col, ncol=ncol, area=ops["area"], release=ops["release"], runoff_a=ops["runoff_a"],
                runoff_b=ops["runoff_b"] if rb else None, scale=scale)


@pytest.mark.parametrize("ni, nj", WINDOWS + [CUT])
def test_host_route_equals_the_restatement(ni, nj):
    """route_cell compiled for the host, in BOTH forms of the neighbour loads, against np_route: 1, 2 and 25 steps, physical operands and
    operands with NaN / Inf / denormal words, runoff_b NULL and given, identity / permuted / mixed col_index (cells that are not owned keep
    the poison of out_new and their storage), the hills' inmask and random bytes."""
    d, m = hills_network(ni, nj)
    r = np.random.default_rng(ni * 7 + nj)
    wild = r.integers(0, 256, (nj, ni)).astype(np.uint8)
    big = ni * nj > 5000
    for which in ("physical", "nasty"):
        ops = route_operands(ni, nj, which)
        for cname, col, ncol in col_indices(ni, nj):
            for rb in (True, False):
                for mname, mask in (("hills", m), ("random", wild)):
                    if big and (mname == "random") != (cname == "mix"):
                        continue                                         # the large window: the two diagonal combinations
                    x = _block(ni, nj, mask, col, ncol, ops, rb)
                    for nstep in ((1, 25) if big else (1, 2, 25)):
                        what = "%dx%d %s %s rb %s mask %s, %d steps" % (ni, nj, which, cname, rb, mname, nstep)
                        ws, wo = np_run(x, ops["storage"], ops["out"], nstep)
                        for load_all in (0, 1):
                            gs, go = host_run(x, ops["storage"], ops["out"], nstep, load_all)
                            assert_same(gs, ws, what + ": storage, load_all %d" % load_all)
                            assert_same(go, wo, what + ": out, load_all %d" % load_all)
                    if cname == "mix":
                        c64 = col.astype(np.int64)
                        ring = (c64 < -1) | (c64 >= ncol)
                        assert ring.any() or ni * nj < 4
                        s1, o1 = np_route(x, ops["out"], np.full((nj, ni), POISON, F), ops["storage"])
                        assert_same(o1[ring], np.full(int(ring.sum()), POISON, F), "cells that are not owned keep the poison")
                        assert_same(s1[ring], ops["storage"][ring], "... and their storage")


def test_empty_store_and_cells_without_local_input():
    """ncol = 0 with every cell -1: no runoff plane is read (they are one element long here); v = 0 leaves -0 + 0 = +0."""
    ni, nj = 5, 3
    d, m = hills_network(ni, nj)
    ops = route_operands(ni, nj, "physical")
    ops["storage"] = np.full((nj, ni), -0.0, F)
    ops["out"] = np.zeros((nj, ni), F)
    x = _block(ni, nj, m, np.full((nj, ni), -1, np.int32), 0, dict(ops, runoff_a=np.full(1, np.nan, F), runoff_b=np.full(1, np.nan, F)))
    for load_all in (0, 1):
        gs, go = host_run(x, ops["storage"], ops["out"], 1, load_all)
        assert (gs.view(U32) == 0).all() and (go.view(U32) == 0).all()


# ---------------------------------------------------------------------------------------------------------------- exact identities
def _channel(n):
    d = np.full((1, n), 1, np.uint8)                                     # every cell drains east, the last one nowhere
    d[0, -1] = 0
    return d, np_inmask(d)


@pytest.mark.parametrize("load_all", (0, 1))
def test_a_pulse_moves_one_cell_per_call(load_all):
    """A straight channel with release = 1 and no input: the pulse is in out of cell t-1 after call t, leaves at the cell without a
    direction in call n, and nothing is left after that.  No tolerance."""
    n = 9
    d, m = _channel(n)
    one = np.ones((1, n), F)
    x = dict(inmask=m, col_index=np.full((1, n), -1, np.int32), ncol=0, area=one, release=one, runoff_a=np.zeros(1, F), runoff_b=None, scale=1.0)
    storage = np.zeros((1, n), F)
    storage[0, 0] = 5.0
    for t in range(1, n + 2):
        gs, go = host_run(x, storage, np.zeros((1, n), F), t, load_all)
        want = np.zeros((1, n), F)
        if t <= n:
            want[0, t - 1] = 5.0
        assert_same(go, want, "out after %d calls" % t)
        assert (gs == 0).all()
        ws, wo = np_run(x, storage, np.zeros((1, n), F), t)
        assert_same(wo, want, "restated out after %d calls" % t)


@pytest.mark.parametrize("ni, nj", [(67, 35), CUT])
def test_unit_input_gives_the_upstream_count(ni, nj):
    """release = 1, area = 1, unit input: after as many calls as the longest path has cells, out equals the upstream count converted to
    float, word for word (integers below 2^24), and stays."""
    d, m = hills_network(ni, nj)
    acc, passes = np_upstream(m)
    assert acc.max() < 2 ** 24
    one = np.ones((nj, ni), F)
    x = dict(inmask=m, col_index=np.arange(ni * nj, dtype=np.int32).reshape(nj, ni), ncol=ni * nj, area=one, release=one,
             runoff_a=np.ones(ni * nj, F), runoff_b=None, scale=1.0)
    zero = np.zeros((nj, ni), F)
    longest = passes                                                     # call t is exact for the cells whose longest path has t cells
    for load_all in (0, 1):
        gs, go = host_run(x, zero, zero, longest, load_all)
        assert_same(go, acc.astype(F), "out after %d calls" % longest)
        assert (gs == 0).all()
        _, go2 = host_run(x, zero, zero, longest + 3, load_all)
        assert_same(go2, acc.astype(F), "and it stays")
    if longest > 1:
        _, early = host_run(x, zero, zero, longest - 1, 0)
        assert (early != acc.astype(F)).any(), "one call fewer is not enough"


# ---------------------------------------------------------------------------------------------------------------- budget
# Where the bound of the budget checks comes from, counted from the rounded operations of the header text in units of 2^-24.  A rounding
# contributes at most one unit relative to its own result.
#   The input of a cell and call, v = ((a + b)*scale)*area: 3 roundings, so the float32 v is within 3 units of the v of exact arithmetic
#     on the same float32 operands (which is what the float64 side adds up).
#   The water of a cell and call, S' + o against S + v + q:
#     q: at most 8 terms, the first added to 0 exactly: 7 roundings, each relative to a partial sum <= s1   (operands >= 0)
#     sv = S + v: 1;  s1 = sv + q: 1;  o = s1*release is whatever it is: the SAME o leaves the storage and enters out;  S' = s1 - o: 1.
#     In all 10 units of s1 per cell and call.
#   The s1 of all cells of one call add up to the water in the network, which is at most what has been put in so far, I_t = t * I_1 with
#     constant input.  Over N calls: 10 * (1 + 2 + ... + N) * I_1 = 10 * (N + 1) / 2 units of I_N = N * I_1.
#   In all 3 + 5 * (N + 1) units of the total input: 258 for N = 50.
#   Against a float64 run of the same scheme, separately for the storage and for what has left: the rounding of o moves up to 1 unit of o
#     <= s1 between the two, and every perturbation stays a perturbation of at most its own size (the scheme is linear, non-negative and
#     loses nothing): 11 instead of 10, 3 + 5.5 * (N + 1): 284 for N = 50 (asserted as 284).
BUDGET_STEPS = 50
BUDGET_BOUND = 3 + 5 * (BUDGET_STEPS + 1)
SPLIT_BOUND = 284


def _run64(x, storage, nstep, outlets):
    """The scheme of the header text in float64 on the same float32 operands: (storage, what has left at the outlets, total input)."""
    m = x["inmask"]
    col = x["col_index"].astype(np.int64)
    ra, rb = x["runoff_a"].astype(np.float64), x["runoff_b"].astype(np.float64)
    v = (ra[col] + rb[col]) * float(F(x["scale"])) * x["area"].astype(np.float64)
    S = storage.astype(np.float64)
    rel = x["release"].astype(np.float64)
    out = np.zeros_like(S)
    left = 0.0
    for _ in range(nstep):
        q = np.zeros_like(S)
        for k in range(1, 9):
            on, inside = neighbour(out, k)
            q = q + np.where(inside & ((m >> (k - 1)) & 1).astype(bool), on, 0.0)
        s1 = (S + v) + q
        out = s1 * rel
        S = s1 - out
        left += out[outlets].sum()
    return S, left, v.sum() * nstep


@pytest.mark.parametrize("ni, nj", [(67, 35)])
def test_budget_on_the_hills(ni, nj):
    """50 calls with constant input on the hills: storage + what has left at the cells without a direction against the input, and both
    against a float64 run of the same scheme, under the bounds counted above.  The restatement measured 0.51 * 2^-24 of the input for the
    sum (bound 258) and 0.34 / 0.14 for the storage / what has left against float64 (bound 284)."""
    d, m = hills_network(ni, nj)
    outlets = d == 0
    ops = route_operands(ni, nj, "physical")
    rel = np.random.default_rng(5).uniform(0.05, 0.6, (nj, ni)).astype(F)
    x = dict(inmask=m, col_index=np.arange(ni * nj, dtype=np.int32).reshape(nj, ni), ncol=ni * nj, area=ops["area"], release=rel,
             runoff_a=ops["runoff_a"], runoff_b=ops["runoff_b"], scale=float(F(F(3600.0) * F(1e-3))))
    zero = np.zeros((nj, ni), F)
    left = 0.0
    planes, S, cur = [zero.copy(), zero.copy()], zero.copy(), 0
    for _ in range(BUDGET_STEPS):
        S, planes[1 - cur] = np_route(x, planes[cur], planes[1 - cur], S)
        cur = 1 - cur
        left += planes[cur][outlets].astype(np.float64).sum()
    gs, go = host_run(x, zero, zero, BUDGET_STEPS, 0)
    assert_same(gs, S, "compiled storage")
    assert_same(go, planes[cur], "compiled out")
    S64, left64, total = _run64(x, zero, BUDGET_STEPS, outlets)
    have = S.astype(np.float64).sum() + left
    in_flight = planes[cur][~outlets].astype(np.float64).sum()           # released in the last call and not yet gathered
    have += in_flight
    r_sum = abs(have - total) / total / EPS
    r_s = abs(S.astype(np.float64).sum() - S64.sum()) / total / EPS
    r_l = abs(left - left64) / total / EPS
    print("%d x %d, %d calls: input %.6g m3, (storage + in flight + left) - input = %.2f * 2^-24 of it (bound %d); against float64: storage %.2f,"
          " left %.2f (bound %d); %.0f %% has left" % (ni, nj, BUDGET_STEPS, total, r_sum, BUDGET_BOUND, r_s, r_l, SPLIT_BOUND, 100 * left / total))
    assert r_sum <= BUDGET_BOUND
    assert r_s <= SPLIT_BOUND and r_l <= SPLIT_BOUND
    assert 0.05 < left / total < 0.95, "water is both held and released"


@pytest.mark.parametrize("rel", (0.25, 0.6, 0.1))
def test_a_single_reservoir_decays_geometrically(rel):
    """One cell, no input: storage after n calls against S0 * (1 - r)^n in float64 (r the float32 number).  Per call o = s1*r is rounded
    once (one unit of o = r/(1-r) units of the new storage) and S' = s1 - o once (sv = S + 0 and s1 = sv + 0 are exact): 1 + r/(1-r) =
    1/(1-r) units per call, n/(1-r) after n calls, plus one for the second order and the float64 side (measured: 2.3, 0.1 and 2.7 units for r = 0.25, 0.6, 0.1)."""
    n = 50
    r32 = F(rel)
    x = dict(inmask=np.zeros((1, 1), np.uint8), col_index=np.full((1, 1), -1, np.int32), ncol=0, area=np.ones((1, 1), F),
             release=np.full((1, 1), r32, F), runoff_a=np.zeros(1, F), runoff_b=None, scale=1.0)
    s0 = np.full((1, 1), 1234.567, F)
    ws, wo = np_run(x, s0, np.zeros((1, 1), F), n)
    for load_all in (0, 1):
        gs, go = host_run(x, s0, np.zeros((1, 1), F), n, load_all)
        assert_same(gs, ws, "storage")
        assert_same(go, wo, "out")
    want = float(s0[0, 0]) * (1.0 - float(r32)) ** n
    bound = n / (1.0 - float(r32)) + 1
    err = abs(float(ws[0, 0]) / want - 1) / EPS
    print("r %g: %.2f * 2^-24 after %d calls (bound %.1f)" % (rel, err, n, bound))
    assert err <= bound


# ---------------------------------------------------------------------------------------------------------------- decomposition
def _parts(ni, nj, z, margin):
    """The 2 x 2 cut: per part the tile slices, the block slices (tile + 1-cell ring inside the domain), and dir on the block from a
    height window with `margin` cells (cells of the ring the window does not reach have no direction)."""
    out = []
    for tile, win, idx in tsh._cuts(ni, nj, margin):
        _, blk, bidx = [c for c in tsh._cuts(ni, nj, 1) if c[0] == tile][0]
        dw = np_flow_dir(z[win], DX, DY)
        dglob = np.zeros((nj, ni), np.uint8)
        seen = np.zeros((nj, ni), bool)
        dglob[win] = dw
        seen[win] = True
        out.append((tile, blk, np.where(seen[blk], dglob[blk], 0).astype(np.uint8), bidx >= 0))
    return out


def _cut_run(ni, nj, z, ops, margin, refresh, nstep, route=None):
    """nstep calls on the four parts; after every call the ring of out is refreshed from the owners (the exchange).  Returns the global
    storage and out planes put together from the tiles."""
    route = route or np_route
    gcol = np.arange(ni * nj, dtype=np.int32).reshape(nj, ni)
    parts = []
    for tile, blk, dblk, owned in _parts(ni, nj, z, margin):
        x = dict(inmask=np_inmask(dblk), col_index=np.where(owned, gcol[blk], -2).astype(np.int32), ncol=ni * nj, area=ops["area"][blk],
                 release=ops["release"][blk], runoff_a=ops["runoff_a"], runoff_b=ops["runoff_b"], scale=3.6)
        parts.append(dict(x=x, tile=tile, blk=blk, owned=owned, S=ops["storage"][blk].copy(), out=[ops["out"][blk].copy(), ops["out"][blk].copy()]))
    cur = 0
    G = ops["out"].copy()
    GS = ops["storage"].copy()
    for _ in range(nstep):
        for p in parts:
            p["S"], p["out"][1 - cur] = route(p["x"], p["out"][cur], p["out"][1 - cur], p["S"])
        cur = 1 - cur
        for p in parts:
            G[p["tile"]] = p["out"][cur][p["owned"]].reshape(G[p["tile"]].shape)
            GS[p["tile"]] = p["S"][p["owned"]].reshape(G[p["tile"]].shape)
        if refresh:
            for p in parts:
                p["out"][cur] = G[p["blk"]].copy()
    return GS, G


def _host_route(x, out_old, out_new, storage):
    m = _c(x["inmask"], np.uint8)
    nj, ni = m.shape
    s, o = _c(storage).copy(), _c(out_new).copy()
    col, area, rel, old = _c(x["col_index"], np.int32), _c(x["area"]), _c(x["release"]), _c(out_old)      # alive until the call returns
    ra, rb = _c(x["runoff_a"]), _c(x["runoff_b"])
    _host().route_cells(ni, nj, _p(m), _p(col), _p(area), _p(rel), _p(s), _p(old), _p(o), _p(ra), _p(rb), float(x["scale"]), int(x["ncol"]), 0)
    return s, o


def _differ(a, b):
    return int((a.view(U32) != b.view(U32)).sum())


def test_decomposition():
    """70 x 130 cut 2 x 2, directions from height windows with a margin of 2 cells, the ring of out refreshed from the neighbours' owned
    cells after every call: after 20 calls no word of storage and out differs from the undecomposed run, restated and compiled.  With
    margin 0 for the directions, or without the refresh, words differ: the test can fail."""
    ni, nj = CUT
    z = tsh.terrain(ni, nj, True)
    ops = route_operands(ni, nj, "physical")
    d = np_flow_dir(z, DX, DY)
    x = dict(inmask=np_inmask(d), col_index=np.arange(ni * nj, dtype=np.int32).reshape(nj, ni), ncol=ni * nj, area=ops["area"],
             release=ops["release"], runoff_a=ops["runoff_a"], runoff_b=ops["runoff_b"], scale=3.6)
    ws, wo = np_run(x, ops["storage"], ops["out"], 20)
    for tile, blk, dblk, owned in _parts(ni, nj, z, 2):
        assert_same_bytes(dblk, d[blk], "margin 2: dir on the tile plus ring is the whole domain's")
    count = {}
    for name, margin, refresh in (("margin 2", 2, True), ("margin 0", 0, True), ("no refresh", 2, False)):
        gs, go = _cut_run(ni, nj, z, ops, margin, refresh, 20)
        count[name] = _differ(gs, ws) + _differ(go, wo)
    print("differing words of storage and out after 20 calls: %r" % count)
    assert count["margin 2"] == 0
    assert count["margin 0"] > 0 and count["no refresh"] > 0
    gs, go = _cut_run(ni, nj, z, ops, 2, True, 20, route=_host_route)
    assert _differ(gs, ws) + _differ(go, wo) == 0, "compiled parts"


@pytest.mark.parametrize("ni, nj", [(65, 5), (67, 35)])
def test_column_order(ni, nj):
    """The same run with a permuted col_index and the runoff planes permuted with it gives the same window planes."""
    d, m = hills_network(ni, nj)
    ops = route_operands(ni, nj, "physical")
    ncell = ni * nj
    ident = np.arange(ncell, dtype=np.int32).reshape(nj, ni)
    x = _block(ni, nj, m, ident, ncell, ops)
    ws, wo = np_run(x, ops["storage"], ops["out"], 10)
    perm = np.random.default_rng(3).permutation(ncell)                   # position p of the store holds tile column perm[p]
    inv = np.empty(ncell, np.int32)
    inv[perm] = np.arange(ncell, dtype=np.int32)
    xp = dict(x, col_index=inv.reshape(nj, ni), runoff_a=ops["runoff_a"][perm], runoff_b=ops["runoff_b"][perm])
    for load_all in (0, 1):
        gs, go = host_run(xp, ops["storage"], ops["out"], 10, load_all)
        assert_same(gs, ws, "storage")
        assert_same(go, wo, "out")


# ---------------------------------------------------------------------------------------------------------------- refusals and bindings
def _ft_block(z, d, **kw):
    b = abi.FlowTerrain()
    b.height, b.dir = z.ctypes.data, d.ctypes.data
    b.nj, b.ni = z.shape
    b.dx, b.dy = DX, DY
    for k, v in kw.items():
        setattr(b, k, v)
    return b


ROUTE_PLANES = ("inmask", "col_index", "area", "release", "storage", "out_old", "out_new", "runoff_a", "runoff_b")


def _route_block(planes, ni=5, nj=3, **kw):
    b = abi.Route()
    for k in ROUTE_PLANES:
        setattr(b, k, planes[k].ctypes.data)
    b.scale, b.ni, b.nj = 3.6, ni, nj
    for k, v in kw.items():
        setattr(b, k, v)
    return b


def test_refusals_write_nothing():
    """Every refusal returns -105 with text before anything is launched or read: the planes here are host memory that the calls must not
    touch, and they keep their poison."""
    lib = abi.load_library()
    ni, nj = 5, 3
    ncell = ni * nj
    err = lambda: lib.noahmp_hip_last_error().decode()                   # noqa: E731
    z = np.full((nj, ni), POISON, F)
    d = np.full((nj, ni), 77, np.uint8)
    m = np.full((nj, ni), 77, np.uint8)
    acc = [np.full((nj, ni), 77, U32) for _ in range(2)]
    changed = np.full(1, 77, U32)

    def ft(b):
        return lib.noahmp_hip_flow_terrain(C.byref(b) if b is not None else None, None)
    assert ft(None) == -105 and "NULL" in err() and "noahmp_hip_flow_terrain" in err()
    for field in ("height", "dir"):
        assert ft(_ft_block(z, d, **{field: None})) == -105 and "required" in err(), field
    for kw, word in ((dict(dx=0.0), "dx"), (dict(dx=-1.0), "dx"), (dict(dx=float("nan")), "dx"), (dict(dy=float("inf")), "dy"), (dict(dy=0.0), "dy"),
                     (dict(ni=-1), "ni"), (dict(nj=-1), "nj"), (dict(ni=65536, nj=32768), "ni*nj")):
        assert ft(_ft_block(z, d, **kw)) == -105 and word in err(), (kw, err())
    im = lib.noahmp_hip_flow_inmask
    assert im(None, m.ctypes.data, ni, nj, None) == -105 and "required" in err() and "noahmp_hip_flow_inmask" in err()
    assert im(d.ctypes.data, None, ni, nj, None) == -105 and "required" in err()
    assert im(d.ctypes.data, d.ctypes.data, ni, nj, None) == -105 and "different" in err()
    for a, b in ((-1, nj), (ni, -1), (65536, 32768)):
        assert im(d.ctypes.data, m.ctypes.data, a, b, None) == -105 and "ni*nj" in err()
    ac = lib.noahmp_hip_flow_accumulate
    ptr = [m.ctypes.data, acc[0].ctypes.data, acc[1].ctypes.data, changed.ctypes.data]
    for k in range(4):
        args = list(ptr)
        args[k] = None
        assert ac(*args, ni, nj, None) == -105 and "required" in err() and "noahmp_hip_flow_accumulate" in err(), k
    assert ac(ptr[0], ptr[1], ptr[1], ptr[3], ni, nj, None) == -105 and "different" in err()
    for a, b in ((-1, nj), (ni, -1), (65536, 32768)):
        assert ac(*ptr, a, b, None) == -105 and "ni*nj" in err()
    planes = {k: np.full(ncell, POISON, F) for k in ROUTE_PLANES}

    def rr(b, ncol=ncell):
        return lib.noahmp_hip_route_runoff(C.byref(b) if b is not None else None, ncol, None)
    assert rr(None) == -105 and "NULL" in err() and "noahmp_hip_route_runoff" in err()
    for field in ROUTE_PLANES[:-1]:
        assert rr(_route_block(planes, **{field: None})) == -105 and "required" in err(), field
    assert rr(_route_block(planes, out_new=planes["out_old"].ctypes.data)) == -105 and "different" in err()
    for kw in (dict(ni=-1), dict(nj=-1), dict(ni=65536, nj=32768)):
        assert rr(_route_block(planes, **kw)) == -105 and "ni*nj" in err(), kw
    for ncol in (-1, 2 ** 31):
        assert rr(_route_block(planes), ncol) == -105 and "ncol" in err()
    assert (z == POISON).all() and (d == 77).all() and (m == 77).all() and all((a == 77).all() for a in acc) and changed[0] == 77
    assert all((p == POISON).all() for p in planes.values())


HEADER_LINES = (
    "#define NOAHMP_HIP_HAS_ROUTING 1\n", "#define NOAHMP_HIP_ABI_MINOR 3\n", "typedef struct noahmp_flow_terrain {", "} noahmp_flow_terrain;",
    "typedef struct noahmp_route {", "} noahmp_route;",
    "noahmp_hip_flow_terrain(const noahmp_flow_terrain* ft, void* stream);",
    "noahmp_hip_flow_inmask(const uint8_t* dir, uint8_t* inmask, int32_t ni, int32_t nj, void* stream);",
    "noahmp_hip_flow_accumulate(const uint8_t* inmask, const uint32_t* acc_old, uint32_t* acc_new, uint32_t* changed,",
    "noahmp_hip_route_runoff(const noahmp_route* r, int64_t ncol, void* stream);",
    "k = 1..8 is E, NE, N, NW, W, SW, S, SE", "opp(k) = ((k+3) & 7) + 1",
    "inv_x = 1.0f / dx;  inv_y = 1.0f / dy;  d2 = dx*dx + dy*dy;  d = sqrtf(d2);  inv_d = 1.0f / d",
    "inv[k] = inv_x for k = 1, 5;  inv_y for k = 3, 7;  inv_d for k = 2, 4, 6, 8.",
    "drop = z0 - height[nb_k];  s = drop * inv[k];  if (s > sbest) { best = k; sbest = s; }",
    "ties go to the first k", "a NaN never wins", "a flat or a pit gives 0", "no cycle can exist", "NO PIT FILLING AND NO FLAT RESOLUTION",
    "a margin of 2 cells", "dir[nb_k] == opp(k)", "A dir value outside 0..8 counts as 0",
    "acc_new[c] = 1 + sum(acc_old[nb_k] : k = 1..8 ascending", "if (acc_new[c] != acc_old[c]) *changed = 1",
    "q = 0;  for k = 1..8 ascending, if bit k-1 of inmask[c] is set and neighbour k lies inside the window:  q = q + out_old[nb_k]",
    "x = runoff_a[d];  if runoff_b: x = x + runoff_b[d];  xs = x*scale;  v = xs*area[c]",
    "s1 = (storage[c] + v) + q;  o = s1*release[c];  storage[c] = s1 - o;  out_new[c] = o",
    "NaN and Inf operands are taken as they are and propagate downstream", "noahmp_hip_exchange_halo",
    "kinematic or diffusive wave, channel geometry, backwater, losses and lakes, a celerity above one cell per call")


def test_bindings_regenerate_identically_with_the_routing_calls():
    from tools import gen_abi
    for rel, text in (("include/noahmp_hip.h", gen_abi.c_header()), ("oracle/ref_harness_gen.f90", gen_abi.ref_harness()),
                      ("noahmp_amd/fortran/module_sf_noahmpdrv_hip.F90", gen_abi.fortran_shim()),
                      ("tests/fortran/shim_wrap_gen.f90", gen_abi.shim_wrap())):
        assert open(os.path.join(ROOT, rel)).read() == text, rel
    hdr = open(os.path.join(ROOT, "include", "noahmp_hip.h")).read()
    for word in HEADER_LINES:
        assert word in hdr, word
    assert "\n".join(gen_abi.routing_header()) in hdr
    assert "noahmp_route" not in gen_abi.ref_harness()
    f90 = open(os.path.join(ROOT, "noahmp_amd", "fortran", "module_sf_noahmpdrv_hip.F90")).read()
    for word in ("bind(C, name='noahmp_hip_flow_terrain')", "bind(C, name='noahmp_hip_flow_inmask')", "bind(C, name='noahmp_hip_flow_accumulate')",
                 "bind(C, name='noahmp_hip_route_runoff')", "type, bind(C) :: noahmp_flow_terrain", "type, bind(C) :: noahmp_route "):
        assert word in f90, word
    for sym in SYMBOLS:
        assert sym in abi.EXPORTED_SYMBOLS
    assert [n for n, _ in abi.FlowTerrain._fields_] == ["height", "dir", "ni", "nj", "dx", "dy"]
    assert [n for n, _ in abi.Route._fields_] == list(ROUTE_PLANES) + ["scale", "ni", "nj"]


SYMBOLS = ("noahmp_hip_flow_terrain", "noahmp_hip_flow_inmask", "noahmp_hip_flow_accumulate", "noahmp_hip_route_runoff")


def test_ctypes_mirrors_match_the_compiled_header(tmp_path):
    body, want = "", []
    for cname, cls in (("noahmp_flow_terrain", abi.FlowTerrain), ("noahmp_route", abi.Route)):
        names = [n for n, _ in cls._fields_]
        body += 'printf(" %%zu", sizeof(%s));' % cname + "".join('printf(" %%zu", offsetof(%s, %s));' % (cname, n) for n in names)
        want += [C.sizeof(cls)] + [getattr(cls, n).offset for n in names]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "noahmp_hip.h"\nint main(){' + body +
                   'printf(" %d %d", NOAHMP_HIP_ABI_MINOR, NOAHMP_HIP_HAS_ROUTING); return 0;}')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert out == want + [3, 1]


def test_library_exports_the_routing_calls():
    if not os.path.exists(abi.LIB_PATH):
        from noahmp_amd import build as b
        b.build()
    build_variant()
    for path in (abi.LIB_PATH, LIB_MASKED):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        for sym in SYMBOLS:
            assert " T %s\n" % sym in out, (path, sym)


@pytest.mark.skipif(tr._flang() is None, reason="no flang")
def test_generated_fortran_types_and_interfaces_compile(tmp_path):
    """The routing part of the generated module compiles, and a caller of the four interfaces type-checks."""
    from tools import gen_abi
    text = "\n".join(["module routing_abi_check", "  use iso_c_binding", "  implicit none"] + gen_abi.routing_f90_types() + ["  interface"] +
                     gen_abi.routing_f90_interfaces() +
                     ["  end interface", "contains", "  function go(ncol, planes) result(rc)", "    integer(c_int64_t), value :: ncol",
                      "    type(c_ptr), intent(in) :: planes(14)", "    type(noahmp_flow_terrain) :: ft", "    type(noahmp_route) :: r",
                      "    integer(c_int) :: rc",
                      "    ft%height = planes(1); ft%dir = planes(2); ft%ni = 64; ft%nj = 8; ft%dx = 1000.0; ft%dy = 1000.0",
                      "    rc = noahmp_hip_flow_terrain(ft, c_null_ptr)",
                      "    rc = noahmp_hip_flow_inmask(planes(2), planes(3), 64_c_int32_t, 8_c_int32_t, c_null_ptr)",
                      "    rc = noahmp_hip_flow_accumulate(planes(3), planes(4), planes(5), planes(6), 64_c_int32_t, 8_c_int32_t, c_null_ptr)",
                      "    r%inmask = planes(3); r%col_index = planes(7); r%area = planes(8); r%release = planes(9); r%storage = planes(10)",
                      "    r%out_old = planes(11); r%out_new = planes(12); r%runoff_a = planes(13); r%runoff_b = c_null_ptr",
                      "    r%scale = 3.6; r%ni = 64; r%nj = 8",
                      "    rc = noahmp_hip_route_runoff(r, ncol, c_null_ptr)",
                      "  end function go", "end module routing_abi_check", ""])
    f = tmp_path / "routing_abi_check.f90"
    f.write_text(text)
    subprocess.check_call([tr._flang(), "-c", str(f), "-o", str(tmp_path / "routing_abi_check.o"), "-J", str(tmp_path)], cwd=str(tmp_path))


def test_esri_codes():
    from noahmp_amd.routing import FlowNetwork
    codes = np.array([[1, 2, 4, 8, 16, 32, 64, 128], [0, 255, 3, 5, -1, 256, 1000, 64]], np.int32)
    want = np.array([[1, 8, 7, 6, 5, 4, 3, 2], [0, 0, 0, 0, 0, 0, 0, 3]], np.uint8)
    assert_same_bytes(FlowNetwork.from_esri(codes), want, "from_esri")


# ---------------------------------------------------------------------------------------------------------------- GPU
_dev = tr._dev
PAD = 5                                                                 # planes start at an odd offset inside their pool


@pytest.fixture(scope="module")
def engine_masked(tables):
    """The variant library: noahmp_hip_route_runoff loads only the neighbours whose bit is set."""
    from noahmp_amd.driver import Engine
    build_variant()                                                      # nothing to do where __graft_entry__.build() has run
    if not os.path.exists(LIB_MASKED):
        pytest.fail("%s missing: __graft_entry__.build() compiles it (-DNMP_ROUTE_LOAD_ALL=0)" % LIB_MASKED)
    return Engine(tables[0], lib_path=LIB_MASKED)


def _pool(n, count, dtype, poison):
    """count planes of n elements, each at offset PAD inside a poisoned row of n + 9: (pool, [views])."""
    import torch
    pool = torch.full((count, n + 9), poison, dtype=dtype, device="cuda")
    return pool, [pool[k, PAD:PAD + n] for k in range(count)]


def _guards_ok(pool, n, poison):
    h = pool.cpu().numpy()
    return (h[:, :PAD] == poison).all() and (h[:, PAD + n:] == poison).all()


@pytest.mark.gpu
@pytest.mark.parametrize("ni, nj", WINDOWS + [CUT])
def test_gpu_network_kernels_equal_the_restatement(engine, ni, nj):
    """noahmp_hip_flow_terrain, _flow_inmask and _flow_accumulate against the restatement in every byte and word: every terrain case,
    the staircase at its own size, random directions with bytes above 8, a random inmask, one pass and the passes to the fixed point.
    Destinations sit at an odd offset inside poisoned pools whose guard bytes keep the poison.  Empty windows write nothing."""
    import torch
    ncell = ni * nj
    bpool, (dird, maskd) = _pool(ncell, 2, torch.uint8, 0xEE)
    dird2, maskd2 = dird.view(nj, ni), maskd.view(nj, ni)
    cases = terrain_cases(ni, nj)
    for name, z, dx, dy in cases:
        bpool.fill_(0xEE)
        torch.cuda.synchronize()
        engine.flow_terrain(engine.flow_terrain_block(_dev(z), dird2, dx, dy))
        engine.flow_inmask(dird2, maskd2)
        engine.stream_sync()
        want = np_flow_dir(z, dx, dy)
        assert_same_bytes(dird2.cpu().numpy(), want, "%dx%d %s: dir" % (ni, nj, name))
        assert_same_bytes(maskd2.cpu().numpy(), np_inmask(want), "%dx%d %s: inmask" % (ni, nj, name))
        assert _guards_ok(bpool, ncell, 0xEE), name
    d = random_dir(ni, nj)
    dird2.copy_(_dev(d))
    torch.cuda.synchronize()
    engine.flow_inmask(dird2, maskd2)
    engine.stream_sync()
    assert_same_bytes(maskd2.cpu().numpy(), np_inmask(d), "%dx%d: inmask of random bytes" % (ni, nj))
    # accumulate
    apool, (a, b, ch) = _pool(ncell, 3, torch.int32, 77)
    a2, b2 = a.view(nj, ni), b.view(nj, ni)
    r = np.random.default_rng(ni + 31 * nj)
    start = r.integers(0, 2 ** 32, (nj, ni), dtype=np.uint64).astype(U32)
    dh, mh = hills_network(ni, nj)
    for name, mask in (("hills", mh), ("random", r.integers(0, 256, (nj, ni)).astype(np.uint8))):
        apool.fill_(77)
        a2.copy_(_dev(start.view(np.int32)))
        ch[:1].zero_()
        torch.cuda.synchronize()
        engine.flow_accumulate(_dev(mask), a2, b2, ch[:1])
        engine.stream_sync()
        want, flag = np_accumulate(mask, start)
        assert_same(b2.cpu().numpy().view(U32), want, "%dx%d %s: one pass" % (ni, nj, name))
        assert int(ch[0].item()) == flag and (ch[1:].cpu().numpy() == 77).all()
        assert _guards_ok(apool, ncell, 77)
    # a pass that changes nothing leaves the flag alone
    acc, passes = np_upstream(mh)
    a2.copy_(_dev(acc.view(np.int32)))
    ch[:1].zero_()
    torch.cuda.synchronize()
    engine.flow_accumulate(_dev(mh), a2, b2, ch[:1])
    engine.stream_sync()
    assert int(ch[0].item()) == 0
    assert_same(b2.cpu().numpy().view(U32), acc, "the fixed point")
    # empty windows
    bpool.fill_(0xEE)
    apool.fill_(77)
    torch.cuda.synchronize()
    blk = engine.flow_terrain_block(_dev(cases[0][1]), dird2, DX, DY)
    blk.nj = 0
    engine.flow_terrain(blk)
    lib = engine.lib
    assert lib.noahmp_hip_flow_inmask(dird.data_ptr(), maskd.data_ptr(), 0, nj, None) == 0
    assert lib.noahmp_hip_flow_accumulate(maskd.data_ptr(), a.data_ptr(), b.data_ptr(), ch.data_ptr(), ni, 0, None) == 0
    engine.stream_sync()
    assert (bpool.cpu().numpy() == 0xEE).all() and (apool.cpu().numpy() == 77).all()


@pytest.mark.gpu
def test_gpu_staircase(engine):
    import torch
    z, where = staircase()
    d = torch.full(z.shape, 99, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    engine.flow_terrain(engine.flow_terrain_block(_dev(z), d, DX_TIE, DY_TIE))
    engine.stream_sync()
    got = d.cpu().numpy()
    assert_same_bytes(got, np_flow_dir(z, DX_TIE, DY_TIE), "staircase")
    assert all(got[j, i] == k1 for i, j, k1, k2 in where)


def _gpu_run(eng, x, storage, out, nstep):
    """nstep calls of noahmp_hip_route_runoff on planes at odd offsets inside poisoned pools: (storage, out, guards intact)."""
    import torch
    nj, ni = x["inmask"].shape
    ncell = ni * nj
    pool, (sd, o0, o1) = _pool(ncell, 3, torch.float32, POISON)
    sd, o0, o1 = (t.view(nj, ni) for t in (sd, o0, o1))
    sd.copy_(_dev(storage))
    o0.copy_(_dev(out))
    o1.copy_(_dev(out))
    ra = _dev(x["runoff_a"])
    rb = _dev(x["runoff_b"]) if x.get("runoff_b") is not None else None
    m, col, area, rel = _dev(x["inmask"]), _dev(x["col_index"]), _dev(x["area"]), _dev(x["release"])
    torch.cuda.synchronize()
    planes, cur = [o0, o1], 0
    for _ in range(nstep):
        eng.route_runoff(eng.route_block(m, col, area, rel, sd, planes[cur], planes[1 - cur], ra, rb, x["scale"]), x["ncol"])
        cur = 1 - cur
    eng.stream_sync()
    return sd.cpu().numpy(), planes[cur].cpu().numpy(), _guards_ok(pool, ncell, POISON)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ("load_all", "masked"))
@pytest.mark.parametrize("ni, nj", WINDOWS + [CUT])
def test_gpu_route_kernel_equals_the_restatement(engine, engine_masked, form, ni, nj):
    """noahmp_hip_route_runoff of the library (loads all eight neighbours) and of the variant library (loads those of the set bits) against
    np_route in every word: 1, 2 and 25 calls, physical and NaN / Inf / denormal operands, runoff_b NULL and given, identity / permuted /
    mixed col_index, the hills' inmask and random bytes; guard words keep the poison.  An empty window writes nothing."""
    import torch
    eng = engine if form == "load_all" else engine_masked
    d, m = hills_network(ni, nj)
    r = np.random.default_rng(ni * 7 + nj)
    wild = r.integers(0, 256, (nj, ni)).astype(np.uint8)
    for which in ("physical", "nasty"):
        ops = route_operands(ni, nj, which)
        for cname, col, ncol in col_indices(ni, nj):
            for rb, mname, mask in ((True, "hills", m), (False, "random", wild)):
                x = _block(ni, nj, mask, col, ncol, ops, rb)
                for nstep in ((1, 2, 25) if (cname, which) == ("mix", "nasty") else (2,)):
                    what = "%s %dx%d %s %s rb %s mask %s, %d calls" % (form, ni, nj, which, cname, rb, mname, nstep)
                    ws, wo = np_run(x, ops["storage"], ops["out"], nstep)
                    gs, go, ok = _gpu_run(eng, x, ops["storage"], ops["out"], nstep)
                    assert_same(gs, ws, what + ": storage")
                    assert_same(go, wo, what + ": out")
                    assert ok, what + ": guard words"
    pool, (sd, o0, o1) = _pool(ni * nj, 3, torch.float32, POISON)
    x = _block(ni, nj, m, col_indices(ni, nj)[0][1], ni * nj, route_operands(ni, nj, "physical"))
    torch.cuda.synchronize()
    b = eng.route_block(_dev(x["inmask"]), _dev(x["col_index"]), _dev(x["area"]), _dev(x["release"]), sd.view(nj, ni), o0.view(nj, ni),
                        o1.view(nj, ni), _dev(x["runoff_a"]), None, 3.6)
    b.nj = 0
    eng.route_runoff(b, ni * nj)
    eng.stream_sync()
    assert (pool.cpu().numpy() == POISON).all()


@pytest.mark.gpu
def test_gpu_directions_of_a_cut_window_equal_the_whole(engine):
    """70 x 130 cut 2 x 2, single process: flow_terrain on height windows with a margin of 2 cells gives, on every tile plus its ring, the
    bytes of the undecomposed launch."""
    import torch
    ni, nj = CUT
    z = tsh.terrain(ni, nj, True)
    whole = torch.empty((nj, ni), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    engine.flow_terrain(engine.flow_terrain_block(_dev(z), whole, DX, DY))
    engine.stream_sync()
    wh = whole.cpu().numpy()
    assert_same_bytes(wh, np_flow_dir(z, DX, DY), "the whole window")
    for (tile, win, idx), (_, blk, _) in zip(tsh._cuts(ni, nj, 2), tsh._cuts(ni, nj, 1)):
        zw = np.ascontiguousarray(z[win])
        part = torch.empty(zw.shape, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        engine.flow_terrain(engine.flow_terrain_block(_dev(zw), part, DX, DY))
        engine.stream_sync()
        g = np.zeros((nj, ni), np.uint8)
        g[win] = part.cpu().numpy()
        assert_same_bytes(g[blk], wh[blk], "part %s" % (tile,))


@pytest.mark.gpu
def test_gpu_decomposed_run_equals_the_whole(engine):
    """20 calls on the four parts of 70 x 130 through FlowNetwork (set_terrain on margin-2 windows), the ring of out refreshed after every
    call by a device copy from the whole-domain plane, against the whole-domain run and the restatement: no word differs."""
    import torch
    from noahmp_amd.routing import FlowNetwork
    ni, nj = CUT
    z = tsh.terrain(ni, nj, True)
    ops = route_operands(ni, nj, "physical")
    d = np_flow_dir(z, DX, DY)
    ncell = ni * nj
    x = dict(inmask=np_inmask(d), col_index=np.arange(ncell, dtype=np.int32).reshape(nj, ni), ncol=ncell, area=ops["area"],
             release=ops["release"], runoff_a=ops["runoff_a"], runoff_b=ops["runoff_b"], scale=3.6)
    ws, wo = np_run(x, ops["storage"], ops["out"], 20)
    gs, go, _ = _gpu_run(engine, x, ops["storage"], ops["out"], 20)
    assert_same(gs, ws, "whole domain: storage")
    assert_same(go, wo, "whole domain: out")
    ra, rb = _dev(ops["runoff_a"]), _dev(ops["runoff_b"])
    gcol = np.arange(ncell, dtype=np.int32).reshape(nj, ni)
    nets = []
    for (tile, win, idx), (_, blk, bidx) in zip(tsh._cuts(ni, nj, 2), tsh._cuts(ni, nj, 1)):
        tj, ti = tile
        net = FlowNetwork(engine, ti.stop - ti.start, tj.stop - tj.start)
        net.set_terrain(_dev(z[win]), DX, DY, origin=(ti.start - win[1].start, tj.start - win[0].start))
        assert net.block_shape == bidx.shape
        net.set_area(_dev(ops["area"][blk]))
        net.set_release(_dev(ops["release"][blk]))
        net.storage.copy_(_dev(ops["storage"][blk]))
        for o in net.out:
            o.copy_(_dev(ops["out"][blk]))
        col = _dev(np.where(bidx >= 0, gcol[blk], -2).astype(np.int32))      # the columns are the whole domain's
        nets.append((net, tile, blk, col))
    G = _dev(ops["out"]).clone()
    torch.cuda.synchronize()
    for _ in range(20):
        for net, tile, blk, col in nets:
            new = 1 - net.cur
            engine.route_runoff(engine.route_block(net.inmask, col, net.area, net.release, net.storage, net.out[net.cur], net.out[new], ra, rb, 3.6),
                                ncell)
            net.cur = new
        engine.stream_sync()
        for net, tile, blk, col in nets:
            G[tile] = net.tile_view(net.out[net.cur])
        for net, tile, blk, col in nets:
            net.out[net.cur].copy_(G[blk])                               # the exchange: the ring from the owners
        torch.cuda.synchronize()
    S = np.zeros((nj, ni), F)
    for net, tile, blk, col in nets:
        S[tile] = net.tile_view(net.storage).cpu().numpy()
    assert_same(S, ws, "decomposed: storage")
    assert_same(G.cpu().numpy(), wo, "decomposed: out")


@pytest.mark.gpu
def test_gpu_refusals_launch_nothing(engine):
    """The refusals with device planes: -105, text, and every plane keeps its poison."""
    import torch
    lib = engine.lib
    ni, nj = 5, 3
    ncell = ni * nj
    fl = torch.full((8, ncell), POISON, dtype=torch.float32, device="cuda")
    by = torch.full((2, ncell), 77, dtype=torch.uint8, device="cuda")
    it = torch.full((4, ncell), 77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    z, d, m = fl[0].data_ptr(), by[0].data_ptr(), by[1].data_ptr()

    def ft(**kw):
        b = abi.FlowTerrain()
        b.height, b.dir, b.ni, b.nj, b.dx, b.dy = z, d, ni, nj, DX, DY
        for k, v in kw.items():
            setattr(b, k, v)
        return lib.noahmp_hip_flow_terrain(C.byref(b), None)
    for kw in (dict(height=None), dict(dir=None), dict(dx=0.0), dict(dy=float("nan")), dict(ni=-1), dict(ni=65536, nj=32768)):
        assert ft(**kw) == -105, kw
        assert "noahmp_hip_flow_terrain" in lib.noahmp_hip_last_error().decode()
    assert lib.noahmp_hip_flow_terrain(None, None) == -105
    assert lib.noahmp_hip_flow_inmask(d, d, ni, nj, None) == -105 and lib.noahmp_hip_flow_inmask(d, None, ni, nj, None) == -105
    assert lib.noahmp_hip_flow_inmask(d, m, 65536, 32768, None) == -105
    a0, a1, ch = it[0].data_ptr(), it[1].data_ptr(), it[2].data_ptr()
    assert lib.noahmp_hip_flow_accumulate(m, a0, a0, ch, ni, nj, None) == -105
    assert lib.noahmp_hip_flow_accumulate(m, a0, a1, None, ni, nj, None) == -105
    assert lib.noahmp_hip_flow_accumulate(m, a0, a1, ch, -1, nj, None) == -105

    def rr(ncol=ncell, **kw):
        b = abi.Route()
        b.inmask, b.col_index = m, it[3].data_ptr()
        b.area, b.release, b.storage, b.out_old, b.out_new, b.runoff_a, b.runoff_b = (fl[k].data_ptr() for k in range(1, 8))
        b.scale, b.ni, b.nj = 3.6, ni, nj
        for k, v in kw.items():
            setattr(b, k, v)
        return lib.noahmp_hip_route_runoff(C.byref(b), ncol, None)
    for kw in (dict(inmask=None), dict(storage=None), dict(runoff_a=None), dict(out_new=fl[4].data_ptr()), dict(nj=-1), dict(ni=65536, nj=32768)):
        assert rr(**kw) == -105, kw
        assert "noahmp_hip_route_runoff" in lib.noahmp_hip_last_error().decode()
    assert rr(ncol=-1) == -105 and rr(ncol=2 ** 31) == -105
    assert lib.noahmp_hip_route_runoff(None, ncell, None) == -105
    engine.stream_sync()
    torch.cuda.synchronize()
    assert (fl.cpu().numpy() == POISON).all() and (by.cpu().numpy() == 77).all() and (it.cpu().numpy() == 77).all()


@pytest.mark.gpu
def test_gpu_upstream_cells(engine):
    """FlowNetwork.upstream_cells on the 67 x 35 hills equals the restated fixed point; summed over the cells without a direction it is
    the number of cells; too few passes raise; caller-given directions with a cycle raise; set_directions refuses a byte above 8."""
    import torch
    from noahmp_amd.routing import FlowNetwork
    ni, nj = 67, 35
    z = tsh.terrain(ni, nj)
    net = FlowNetwork(engine, ni, nj)
    net.set_terrain(_dev(z), DX, DY)
    d, m = hills_network(ni, nj)
    assert_same_bytes(net.dir.cpu().numpy(), d, "dir")
    assert_same_bytes(net.inmask.cpu().numpy(), m, "inmask")
    acc, passes = np_upstream(m)
    got = net.upstream_cells().cpu().numpy().view(U32)
    assert_same(got, acc, "upstream_cells")
    assert int(got[d == 0].astype(np.int64).sum()) == ni * nj
    with pytest.raises(RuntimeError, match="cycle"):
        net.upstream_cells(max_pass=max(1, passes - 2))
    loop = np.zeros((3, 3), np.uint8)
    loop[0, 0], loop[0, 1] = 1, 5                                         # two cells that drain into each other
    net2 = FlowNetwork(engine, 3, 3)
    net2.set_directions(_dev(loop))
    with pytest.raises(RuntimeError, match="cycle"):
        net2.upstream_cells()
    with pytest.raises(ValueError):
        net2.set_directions(_dev(np.full((3, 3), 9, np.uint8)))
    esri = FlowNetwork.from_esri(torch.tensor([[1, 16, 0]], dtype=torch.int32, device="cuda"))
    assert esri.cpu().numpy().tolist() == [[1, 5, 0]]


class _RingFromWhole:
    """A stand-in for Comm in one process: exchange_halo copies the ring of the plane from the whole-domain out plane of the same call,
    ENQUEUED ONLY on torch's current stream, as the RCCL and IPC transports of the real exchange are."""

    def __init__(self, whole_planes, blk, ring):
        self.whole, self.blk, self.ring, self.calls = whole_planes, blk, ring, 0

    def exchange_halo(self, planes, geom):
        import torch
        assert len(planes) == 1 and geom == "geom"
        src = self.whole[self.calls][self.blk]
        planes[0].copy_(torch.where(self.ring, src, planes[0]))
        self.calls += 1


@pytest.mark.gpu
def test_gpu_step_with_an_exchange_equals_the_whole(engine):
    """FlowNetwork.step(comm=..., nsub=2) on the four parts of 70 x 130, five steps: the exchange is a stand-in that copies the ring from
    the whole-domain plane of the same call on torch's CURRENT stream -- here a side stream, which nothing orders against the engine's
    own, non-blocking stream but step() itself -- and only enqueues.  Every part equals the whole-domain restatement in every word of
    storage and out: the next launch, in the same step and in the next, reads a ring that has arrived."""
    import types
    import torch
    from noahmp_amd.routing import FlowNetwork
    ni, nj = CUT
    nstep, nsub, dt = 5, 2, 3600.0
    z = tsh.terrain(ni, nj, True)
    ops = route_operands(ni, nj, "physical")
    d = np_flow_dir(z, DX, DY)
    ncell = ni * nj
    x = dict(inmask=np_inmask(d), col_index=np.arange(ncell, dtype=np.int32).reshape(nj, ni), ncol=ncell, area=ops["area"],
             release=ops["release"], runoff_a=ops["runoff_a"], runoff_b=ops["runoff_b"], scale=float(F(dt) * F(1e-3)) / nsub)
    S, planes, cur, whole = ops["storage"].copy(), [ops["out"].copy(), ops["out"].copy()], 0, []
    for _ in range(nstep * nsub):
        S, planes[1 - cur] = np_route(x, planes[cur], planes[1 - cur], S)
        cur = 1 - cur
        whole.append(_dev(planes[cur]))
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    for (tile, win, idx), (_, blk, bidx) in zip(tsh._cuts(ni, nj, 2), tsh._cuts(ni, nj, 1)):
        tj, ti = tile
        net = FlowNetwork(engine, ti.stop - ti.start, tj.stop - tj.start)
        net.set_terrain(_dev(z[win]), DX, DY, origin=(ti.start - win[1].start, tj.start - win[0].start))
        net.set_area(_dev(ops["area"][blk]))
        net.set_release(_dev(ops["release"][blk]))
        net.set_input_columns(None)
        net.storage.copy_(_dev(ops["storage"][blk]))
        for o in net.out:
            o.copy_(_dev(ops["out"][blk]))
        store = types.SimpleNamespace(ni=net.ni, nj=net.nj, a=dict(runsfxy=_dev(ops["runoff_a"].reshape(nj, ni)[tile]),
                                                                   runsbxy=_dev(ops["runoff_b"].reshape(nj, ni)[tile])))
        comm = _RingFromWhole(whole, blk, _dev(bidx < 0))
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            for _ in range(nstep):
                net.step(store, dt, nsub=nsub, comm=comm, geom="geom")
        engine.stream_sync()
        torch.cuda.synchronize()
        assert comm.calls == nstep * nsub
        assert_same(net.tile_view(net.storage).cpu().numpy(), S[tile], "part %s: storage" % (tile,))
        assert_same(net.out[net.cur].cpu().numpy(), planes[cur][blk], "part %s: out, ring included" % (tile,))


@pytest.mark.gpu
def test_gpu_set_velocity_and_default_area(engine):
    """set_velocity makes release = 1 - exp(-dt*v/length) in float64, rounded once, with length = dx for E / W and cells without a
    direction, dy for N / S, the diagonal otherwise (dx != dy, every direction present, a velocity plane); the default area dx*dy is
    remade when set_directions comes again with another spacing, the caller's own area is kept."""
    from noahmp_amd.routing import FlowNetwork
    dirs = np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8]], np.uint8)
    v = np.array([[0.5, 0.25, 1.0], [2.0, 0.1, 0.75], [0.3, 1.5, 0.05]], F)
    dx, dy, dt = 1000.0, 1500.0, 900.0
    net = FlowNetwork(engine, 3, 3)
    net.set_directions(_dev(dirs), dx=dx, dy=dy)
    net.set_velocity(_dev(v), dt)
    diag = np.sqrt(dx * dx + dy * dy)
    length = np.array([[dx, dx, diag], [dy, diag, dx], [diag, dy, diag]])
    want = (1.0 - np.exp(-dt * v.astype(np.float64) / length)).astype(F)
    assert_same(net.release.cpu().numpy(), want, "release of set_velocity")
    assert len({float(t) for t in length.ravel()}) == 3 and (want > 0).all() and (want < 1).all()
    net.set_velocity(0.5, dt)
    assert_same(net.release.cpu().numpy(), (1.0 - np.exp(-dt * 0.5 / length)).astype(F), "one velocity for every cell")
    assert (net.area.cpu().numpy() == F(dx * dy)).all()
    net.set_directions(_dev(dirs), dx=500.0, dy=250.0)
    assert (net.area.cpu().numpy() == F(500.0 * 250.0)).all(), "the default area follows the spacing"
    net.set_area(7.0)
    net.set_directions(_dev(dirs), dx=dx, dy=dy)
    assert (net.area.cpu().numpy() == F(7.0)).all(), "the caller's area is kept"
    assert net.passes == 0


ENG_NI, ENG_NJ, ENG_MARGIN = tsv.VAL_NI, tsv.VAL_NJ, tsv.VAL_MARGIN
ENG_STEPS = 3


def _engine_run(engine, tables, height, sort, route, nsub=1):
    """Three engine steps of the 35 x 67 mixed tile at a rainy hour, each followed by FlowNetwork.step.  Returns the store, the network and
    per step the store's two runoff planes in TILE order."""
    import torch
    from noahmp_amd import synth
    from noahmp_amd.routing import FlowNetwork
    T, tb = tables
    s = synth.mixed_small(tb, ni=ENG_NI, nj=ENG_NJ)
    lake = np.random.default_rng(11).random((ENG_NJ, ENG_NI)) < 0.06      # water: the step skips these columns
    s.a["ivgtyp"][lake] = s.cfg.iswater
    s.a["xland"][lake] = 2.0
    synth.first_step_fixups(s)
    synth.diurnal_forcing(s, 11, t_offset=s.t_offset)
    d = s.to_device("cuda:0")
    torch.cuda.synchronize()
    net = None
    if route:
        net = FlowNetwork(engine, ENG_NI, ENG_NJ)
        net.set_terrain(_dev(height), DX, DX, origin=(ENG_MARGIN, 0))
        net.set_velocity(0.4, d.cfg.dt / nsub)
    perm = None
    if sort:
        engine.sort_store(d)
        perm = d.sort_perm.cpu().numpy()
        if route:
            net.follow(d)
    seen = []
    for it in range(1, ENG_STEPS + 1):
        st = engine.noahmplsm(d, it, 2000, 180.0)
        assert st.code == 0
        if route:
            net.step(d, d.cfg.dt, nsub=nsub)
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
    return d, net, seen


def _exits(dirp, owned):
    """The owned cells whose release nobody of this block gathers: no direction, or a direction into the ring (the neighbour rank's)."""
    kept = np.zeros(dirp.shape, bool)
    for k in range(1, 9):
        on, inside = neighbour(owned, k, fill=False)
        kept |= (dirp == k) & inside & on
    return owned & ~kept


def _restated_engine_run(net_h, seen, dt, nsub=1):
    """The restatement driven by the runoff planes the engine run produced: storage, out, and the float64 budget terms."""
    x = dict(net_h, ncol=ENG_NI * ENG_NJ, scale=float(F(dt) * F(1e-3)) / nsub)
    S = np.zeros(net_h["inmask"].shape, F)
    planes, cur = [S.copy(), S.copy()], 0
    left = total = total_abs = 0.0
    owned = net_h["col_index"] >= -1
    outlets = _exits(net_h["dir"], owned)
    tile = net_h["col_index"] >= 0
    for ra, rb in seen:
        x["runoff_a"], x["runoff_b"] = ra, rb
        for _ in range(nsub):
            S, planes[1 - cur] = np_route(x, planes[cur], planes[1 - cur], S)
            cur = 1 - cur
            left += planes[cur][outlets].astype(np.float64).sum()
            col = net_h["col_index"][tile]
            v = (ra[col].astype(np.float64) + rb[col]) * float(F(x["scale"])) * net_h["area"][tile].astype(np.float64)
            total += v.sum()
            total_abs += np.abs(v).sum()
    return S, planes[cur], left, total, total_abs


@pytest.mark.gpu
def test_gpu_engine_run_in_a_valley(engine, tables):
    """Three noahmplsm steps of a 35 x 67 mixed tile in the valley terrain (the window has a margin of 4 cells along i: the block is the
    tile plus a ring along i), each followed by FlowNetwork.step: storage and out equal the restatement driven by the store's own runoff
    planes in every word; sorted and unsorted stores give identical planes; every array of the store is bit-identical to the run without
    routing; the budget holds under the bound counted above for three calls: 10 * (1 + 2 + 3) + 3 = 63 units of the absolute input (the
    inputs differ from step to step, so every I_t is bounded by the whole); with two sub-steps per step the restatement holds as well."""
    from tools.compare import exact_check
    height = tsv._valley()
    d, net, seen = _engine_run(engine, tables, height, False, True)
    net_h = dict(inmask=net.inmask.cpu().numpy(), col_index=net.col_index.cpu().numpy(), area=net.area.cpu().numpy(),
                 release=net.release.cpu().numpy(), dir=net.dir.cpu().numpy())
    blk = (slice(None), slice(ENG_MARGIN - 1, ENG_MARGIN + ENG_NI + 1))
    dwin = np_flow_dir(height, DX, DX)
    assert_same_bytes(net_h["dir"], dwin[blk], "dir of the block")
    assert_same_bytes(net_h["inmask"], np_inmask(dwin[blk]), "inmask of the block")
    col = net_h["col_index"]
    assert (col[:, 0] == -2).all() and (col[:, -1] == -2).all() and (col[:, 1:-1] >= -1).all()
    xland = d.a["xland"].cpu().numpy().ravel()
    assert ((col[:, 1:-1].ravel() == -1) == (xland >= 1.5)).all() and (col == -1).any(), "water columns have no local input"
    assert sum(float(np.abs(p).sum()) for planes in seen for p in planes) > 0, "the steps produce runoff"
    S, out, left, total, total_abs = _restated_engine_run(net_h, seen, d.cfg.dt)
    assert_same(net.storage.cpu().numpy(), S, "storage")
    assert_same(net.out[net.cur].cpu().numpy(), out, "out")
    # discharge() is torch's out / dt, not part of the contract: the device may multiply with the rounded reciprocal (two roundings and
    # the reciprocal's: 3 units at most)
    q, q64 = net.discharge().cpu().numpy().astype(np.float64), out.astype(np.float64) / d.cfg.dt
    assert (np.abs(q - q64) <= 3 * EPS * np.abs(q64)).all() and (q64 > 0).any()
    owned = col >= -1
    exits = _exits(net_h["dir"], owned)
    assert (exits & (net_h["dir"] != 0)).any(), "some water leaves through the ring"
    have = S[owned].astype(np.float64).sum() + left + out[owned & ~exits].astype(np.float64).sum()      # held, left, and released but not yet gathered
    ratio = abs(have - total) / total_abs / EPS
    print("valley run: input %.6g m3, budget error %.2f * 2^-24 of the absolute input (bound 63)" % (total, ratio))
    assert total_abs > 0 and ratio <= 10 * (1 + 2 + 3) + 3
    ds, nets, seen_s = _engine_run(engine, tables, height, True, True)
    assert (ds.sort_perm.cpu().numpy() != np.arange(ENG_NI * ENG_NJ)).any()
    for a, b in zip(seen, seen_s):
        for p, q in zip(a, b):
            assert_same(p, q, "the runoff planes of the sorted run, in tile order")
    assert_same(nets.storage.cpu().numpy(), S, "storage of the sorted run")
    assert_same(nets.out[nets.cur].cpu().numpy(), out, "out of the sorted run")
    assert (nets.col_index.cpu().numpy() != col).any()
    without, _, _ = _engine_run(engine, tables, height, False, False)
    ok, lines = exact_check(without.to_host(), d.to_host())
    assert ok, "\n".join(lines)
    d2, net2, seen2 = _engine_run(engine, tables, height, False, True, nsub=2)
    net2_h = dict(net_h, release=net2.release.cpu().numpy())
    S2, out2, _, _, _ = _restated_engine_run(net2_h, seen2, d.cfg.dt, nsub=2)
    assert_same(net2.storage.cpu().numpy(), S2, "storage with two sub-steps")
    assert_same(net2.out[net2.cur].cpu().numpy(), out2, "out with two sub-steps")
    state = net2.state_dict()
    net2.storage.zero_()
    net2.load_state_dict(state)
    assert_same(net2.storage.cpu().numpy(), S2, "the restart state")


@pytest.mark.gpu
def test_gpu_engine_run_on_flat_terrain(engine, tables):
    """The same three steps on the flat window: no cell has a direction or an upstream neighbour, every cell is its own outlet, and
    out == release * (storage + v), storage and v those of the call."""
    height = tsv._valley(flat=True)
    d, net, seen = _engine_run(engine, tables, height, False, True)
    assert (net.dir.cpu().numpy() == 0).all() and (net.inmask.cpu().numpy() == 0).all()
    col = net.col_index.cpu().numpy()
    area, rel = net.area.cpu().numpy(), net.release.cpu().numpy()
    scale = F(F(d.cfg.dt) * F(1e-3))
    S = np.zeros(col.shape, F)
    owned, local = col >= -1, col >= 0
    for ra, rb in seen:
        x = (ra[np.where(local, col, 0)] + rb[np.where(local, col, 0)]).astype(F)
        v = np.where(local, (x * scale) * area, F(0.0)).astype(F)
        s1 = (S + v) + F(0.0)
        o = np.where(owned, s1 * rel, F(0.0)).astype(F)
        S = np.where(owned, s1 - o, S).astype(F)
    assert_same(net.out[net.cur].cpu().numpy(), o, "out == release * (storage + v)")
    assert_same(net.storage.cpu().numpy(), S, "storage")
    assert float(o.sum()) > 0
