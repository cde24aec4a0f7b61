"""Watershed delineation on the D8 network on the device (noahmp_hip_flow_basin_init / _jump / _resolve; nmp_dev_basins.hpp; Basins).

No reference routine stands behind the calls; the contract is the text in include/noahmp_hip.h.  np_basin_init / np_basin_jump /
np_basin_resolve restate it in numpy; walk() is an independent method, a sequential walker that follows dir from every cell.  Every word is
an integer and the fixed point is unique, so everything is compared word for word: no tolerance appears anywhere.  The pass counts are
derived (ceil(log2 max(L, 1)) + 1 for a longest path of L hops) and asserted."""
import ctypes as C
import functools
import json
import os
import subprocess

import numpy as np
import pytest

from noahmp_amd import abi
import test_flow_fill as tff
import test_regions as tg
import test_regrid as tr
import test_routing as trt
import test_shadow as tsh
from test_routing import DX, DY, assert_same_bytes, np_flow_dir, np_inmask

ROOT = tr.ROOT
CSRC = tr.CSRC
SRC = os.path.join(ROOT, "tests", "host_emul", "basins_check.hip")
LIB = os.path.join(ROOT, "tests", "host_emul", "libbasins_check.so")
HEADER = tff.HEADER
REFUSAL_FIXTURE = os.path.join(ROOT, "tests", "golden", "basins_refusal_text.json")
I32 = np.int32
F = np.float32
NONE, PENDING, CYCLE = -1, -2, -3
SAT = 2 ** 31 - 1
RING = tff.RING
TI, TJ = tff.TI, tff.TJ
CUT = tff.CUT
# (ni, nj): a lone cell, one row of one column, one column of one row, more than one block with odd sizes, the fill's tile, 2 x 5 tiles
SHAPES = [(1, 1), (1, 9), (9, 1), (67, 35), (TI, TJ), CUT]
STATE_POISON, WORD_POISON = 0x0707070707070707, 0x07070707
MAX_SWEEPS = tff._macro_or("NOAHMP_FLOW_BASIN_MAX_SWEEPS", 16)
SWEEPS = (2, 5, MAX_SWEEPS)


def cap_of(n):
    """ceil(log2(n)) + 1."""
    return (max(n, 1) - 1).bit_length() + 1


def passes_of(L):
    """ceil(log2 max(L, 1)) + 1: the passes to convergence plus the one that leaves the flag alone."""
    return (max(L, 1) - 1).bit_length() + 1


def assert_words(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    bad = np.flatnonzero(a.ravel() != b.ravel())
    assert bad.size == 0, "%s: %d of %d words differ, first at %d: %s != %s" % (what, bad.size, a.size, bad[0], a.ravel()[bad[0]], b.ravel()[bad[0]])


# ---------------------------------------------------------------------------------------------------------------- the restatement
def np_down(d):
    """down(c) of the header text: flat index of the downstream cell, -1 where there is none (int64 plane)."""
    nj, ni = d.shape
    k = np.where(d <= 8, d, 0).astype(np.int64)
    di = np.array((0,) + trt.DI)[k]
    dj = np.array((0,) + trt.DJ)[k]
    jj, ii = np.meshgrid(np.arange(nj), np.arange(ni), indexing="ij")
    ok = (k > 0) & (jj + dj >= 0) & (jj + dj < nj) & (ii + di >= 0) & (ii + di < ni)
    return np.where(ok, (jj + dj) * ni + ii + di, -1)


def np_basin_init(d, seed, flags):
    """(state [nj, ni, 2], label, dist) of noahmp_hip_flow_basin_init."""
    nj, ni = d.shape
    jj, ii = np.meshgrid(np.arange(nj), np.arange(ni), indexing="ij")
    c = jj * ni + ii
    side = (ii == 0) * 1 | (ii == ni - 1) * 2 | (jj == 0) * 4 | (jj == nj - 1) * 8
    ring = (side & (flags >> 4)) != 0
    sd = np.full(d.shape, -1, np.int64) if seed is None else seed.astype(np.int64)
    down = np_down(d)
    is_seed = ~ring & (sd >= 0)
    free = ~ring & ~is_seed & (down >= 0)
    state = np.stack([np.where(free, down, c), np.where(free, 1, 0)], axis=-1).astype(I32)
    label = np.where(ring | free, PENDING, np.where(is_seed, sd, NONE)).astype(I32)
    dist = np.where(ring | free, -1, 0).astype(I32)
    return state, label, dist


def np_basin_jump(state):
    """One pass: (state_new, changed)."""
    s = state.reshape(-1, 2)
    n = s.shape[0]
    p = s[:, 0].astype(np.int64)
    ok = (p >= 0) & (p < n)
    q = s[np.where(ok, p, 0)]
    hops = np.minimum(s[:, 1].astype(np.int64) + q[:, 1].astype(np.int64), SAT)
    new = np.stack([np.where(ok, q[:, 0], s[:, 0]), np.where(ok, hops, s[:, 1])], axis=-1).astype(I32)
    return new.reshape(state.shape), int((ok & (q[:, 0] != s[:, 0])).any())


def np_basin_resolve(state, label, dist):
    """(label, dist, changed) of noahmp_hip_flow_basin_resolve; roots are only read, so reading the old planes is the in-place result."""
    s = state.reshape(-1, 2)
    n = s.shape[0]
    c = np.arange(n)
    lab, dis = label.ravel().astype(np.int64), dist.ravel().astype(np.int64)
    r, h = s[:, 0].astype(np.int64), s[:, 1].astype(np.int64)
    ok = (r >= 0) & (r < n)
    rs = np.where(ok, r, 0)
    own = ok & (r == c)
    other = ok & (r != c)
    root_ok = (s[rs, 0] == rs) & (s[rs, 1] == 0)
    lr = lab[rs]
    cyc = (own & (h != 0)) | (other & (~root_ok | (lr == CYCLE)))
    take = other & root_ok & (lr != CYCLE) & (lr != PENDING)
    nl = np.where(cyc, CYCLE, np.where(take, lr, lab))
    nd = np.where(cyc, -1, np.where(take, np.minimum(h + dis[rs], SAT), dis))
    return nl.astype(I32).reshape(label.shape), nd.astype(I32).reshape(dist.shape), int((nl != lab).any())


class Restated:
    """init, every pass up to the first that changes nothing (or the cap), and one resolve, by the restatement."""

    def __init__(self, d, seed, flags):
        self.init = np_basin_init(d, seed, flags)
        self.cap = cap_of(d.size)
        self.states, self.flags = [self.init[0]], []
        self.converged = False
        while len(self.flags) < self.cap:
            new, flag = np_basin_jump(self.states[-1])
            self.states.append(new)
            self.flags.append(flag)
            if not flag:
                self.converged = True
                break
        self.passes = len(self.flags)
        self.state = self.states[-1]
        self.label, self.dist, self.resolve_flag = np_basin_resolve(self.state, self.init[1], self.init[2])
        for a in self.states + [self.label, self.dist] + list(self.init):
            a.setflags(write=False)


# ---------------------------------------------------------------------------------------------------------------- the walker
def walk(d, seed, flags):
    """An independent method: follow dir from every cell, sequentially, remembering what is known.  Returns (label, dist, hops to the
    root, or -1 for a cell on a cycle or above one).  A ring cell holds PENDING / -1: nobody has answered for it."""
    nj, ni = d.shape
    n = ni * nj
    dl = d.ravel().tolist()
    sl = None if seed is None else seed.ravel().tolist()
    label, dist, hroot = [None] * n, [None] * n, [None] * n

    def kind(c):
        j, i = divmod(c, ni)
        if (flags & RING["w"] and i == 0) or (flags & RING["e"] and i == ni - 1) or (flags & RING["s"] and j == 0) or (flags & RING["n"] and j == nj - 1):
            return "ring", None
        if sl is not None and sl[c] >= 0:
            return "seed", None
        k = dl[c]
        if 1 <= k <= 8:
            i2, j2 = i + trt.DI[k - 1], j + trt.DJ[k - 1]
            if 0 <= i2 < ni and 0 <= j2 < nj:
                return "free", j2 * ni + i2
        return "terminal", None

    for c0 in range(n):
        path, seen, x = [], set(), c0
        while True:
            if label[x] is not None:
                break
            if x in seen:                                                 # a cycle: everything on the path ends on it
                for y in path:
                    label[y], dist[y], hroot[y] = CYCLE, -1, -1
                path = []
                break
            what, nxt = kind(x)
            if what == "free":
                seen.add(x)
                path.append(x)
                x = nxt
                continue
            hroot[x] = 0
            if what == "ring":
                label[x], dist[x] = PENDING, -1
            elif what == "seed":
                label[x], dist[x] = sl[x], 0
            else:
                label[x], dist[x] = NONE, 0
            break
        for y in reversed(path):                                          # x is known; unwind
            label[y] = label[x]
            dist[y] = -1 if label[x] in (CYCLE, PENDING) else dist[x] + 1
            hroot[y] = -1 if hroot[x] < 0 else hroot[x] + 1
            x = y
    sh = (nj, ni)
    return np.array(label, I32).reshape(sh), np.array(dist, I32).reshape(sh), np.array(hroot, np.int64).reshape(sh)


def upstream_counts(d):
    """Cells that drain through every cell, itself included, by Kahn's order (an independent method; cells on a cycle get 0)."""
    down = np_down(d).ravel()
    n = down.size
    indeg = np.bincount(down[down >= 0], minlength=n)
    cnt = np.ones(n, np.int64)
    done = np.zeros(n, bool)
    stack = np.flatnonzero(indeg == 0).tolist()
    dn = down.tolist()
    indeg = indeg.tolist()
    cl = cnt.tolist()
    while stack:
        c = stack.pop()
        done[c] = True
        t = dn[c]
        if t >= 0:
            cl[t] += cl[c]
            indeg[t] -= 1
            if indeg[t] == 0:
                stack.append(t)
    return np.where(done, np.array(cl, np.int64), 0).reshape(d.shape)


# ---------------------------------------------------------------------------------------------------------------- cases
def cyclic_plane(ni, nj):
    """A hand-made plane: a 2-cycle, a 3-cycle and a 4-cycle with a tail leading into each (where the window has room), the rest draining
    west to the edge."""
    d = np.full((nj, ni), 5, np.uint8)
    if ni >= 8 and nj >= 6:
        d[1, 2], d[1, 3] = 1, 5                                           # 2-cycle (2,1) <-> (3,1); tail from the east along row 1
        d[3, 2], d[3, 3], d[4, 2] = 1, 4, 7                               # 3-cycle (2,3) -> (3,3) -> (2,4) -> (2,3); tail along row 3
        d[4, 3:] = 5                                                      # row 4 drains west into (2,4)
        d[4, 1] = 1                                                       # and from the west
        if nj >= 9:
            d[6, 4], d[6, 5], d[7, 5], d[7, 4] = 1, 3, 5, 7               # 4-cycle; rows 6 and 7 east of it lead in
    elif ni >= 4:
        d[0, 1], d[0, 2] = 1, 5                                           # one row: a 2-cycle with tails on both sides
        d[0, 0] = 1
    elif nj >= 4:
        d[:, 0] = 7
        d[1, 0], d[2, 0] = 3, 7
    return d


@functools.lru_cache(maxsize=None)
def dir_cases(ni, nj):
    """((name, dir, flags, acyclic)): directions of every raw and every filled terrain of test_flow_fill.cases, a random plane, a hand-made
    cyclic plane, and ring sides on two of them."""
    out = []
    solved = tff.solved(ni, nj)
    for name, z, eps, outlet, fl in tff.cases(ni, nj):
        out.append(("raw " + name, np_flow_dir(z, DX, DY), 0, True))
        out.append(("filled " + name, np_flow_dir(solved[name][2], DX, DY), 0, True))
    out.append(("random bytes", trt.random_dir(ni, nj), 0, False))
    out.append(("hand-made cycles", cyclic_plane(ni, nj), 0, False))
    out.append(("filled hills, ring W and N", out[1][1], RING["w"] | RING["n"], True))
    out.append(("random bytes, ring on every side", trt.random_dir(ni, nj, seed=1), 0xF0, False))
    for c in out:
        c[1].setflags(write=False)
    return tuple(out)


def pick_gauges(d, which):
    """[(i, j)]: none; the cell of the largest upstream count; or up to five: that cell, two more up the main stem and the two largest
    tributaries that join it."""
    if which == "none":
        return []
    nj, ni = d.shape
    cnt = upstream_counts(d).ravel()
    c0 = int(np.argmax(cnt))
    cells = [c0]
    if which == "nested":
        down = np_down(d).ravel()
        kids = {}
        for c in np.flatnonzero(down >= 0).tolist():
            if cnt[c] > 0:
                kids.setdefault(int(down[c]), []).append(c)
        stem = [c0]
        side = []
        while kids.get(stem[-1]):
            ks = sorted(kids[stem[-1]], key=lambda c: (-cnt[c], c))
            side.extend(ks[1:])
            stem.append(ks[0])
        cells += [stem[len(stem) // 3], stem[2 * len(stem) // 3]] + sorted(side, key=lambda c: (-cnt[c], c))[:2]
    seen, out = set(), []
    for c in cells:
        if c not in seen:
            seen.add(c)
            out.append((c % ni, c // ni))
    return out


GAUGES = ("none", "one", "nested")


@functools.lru_cache(maxsize=None)
def combo(ni, nj, ci, gi):
    """(what, dir, seed plane or None, flags, points, acyclic, Restated, walker's (label, dist, hroot)) of case ci with gauge set gi."""
    name, d, flags, acyclic = dir_cases(ni, nj)[ci]
    pts = pick_gauges(d, GAUGES[gi])
    seed = None
    if pts:
        seed = np.full(d.shape, -1, I32)
        for n, (i, j) in enumerate(pts):
            seed[j, i] = n
        seed.setflags(write=False)
    return ("%dx%d %s, gauges: %s" % (ni, nj, name, GAUGES[gi]), d, seed, flags, pts, acyclic, Restated(d, seed, flags), walk(d, seed, flags))


def combos(ni, nj):
    for ci in range(len(dir_cases(ni, nj))):
        for gi in range(len(GAUGES)):
            yield combo(ni, nj, ci, gi)


# ---------------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("ni, nj", SHAPES)
def test_restatement_equals_the_walker(ni, nj):
    """label and dist of init + passes + one resolve equal the sequential walker's in every word, in every case; the passes made are
    ceil(log2 max(L, 1)) + 1 with the walker's longest path L where no cycle exists, and at most the cap where one does; a plane with a
    cycle ends with CYCLE exactly at the walker's cells."""
    for what, d, seed, flags, pts, acyclic, rs, (wl, wd, wh) in combos(ni, nj):
        assert_words(rs.label, wl, what + ": label")
        assert_words(rs.dist, wd, what + ": dist")
        has_cycle = bool((wh < 0).any())
        assert not (acyclic and has_cycle), what
        if not has_cycle:
            assert rs.converged and rs.passes == passes_of(int(wh.max())), (what, rs.passes, int(wh.max()))
            assert not (rs.label == CYCLE).any()
        assert rs.passes <= rs.cap, what
        assert ((rs.label == CYCLE) == (wh < 0)).all(), what
        ptr, hops = rs.state[..., 0], rs.state[..., 1]
        ok = wh >= 0
        assert (hops[ok] == wh[ok]).all(), what + ": hops of the state are the walker's hops to the root"
        roots = ptr.ravel()[ptr.ravel()[ok.ravel()]]
        assert (roots == ptr.ravel()[ok.ravel()]).all(), what + ": a pointer ends at a root"
        if flags == 0:
            assert not (rs.label == PENDING).any(), what
    assert len(pick_gauges(dir_cases(*CUT)[1][1], "nested")) == 5


def test_the_serpentine_needs_14_passes_where_jacobi_needs_thousands():
    """The corridor of the 70 x 130 serpentine: the longest path is above 1000 cells -- one Jacobi pass of noahmp_hip_flow_accumulate per
    cell of it -- and the doubling needs ceil(log2 L) + 1 <= 14."""
    ni, nj = CUT
    names = [c[0] for c in dir_cases(ni, nj)]
    what, d, seed, flags, pts, acyclic, rs, (wl, wd, wh) = combo(ni, nj, names.index("filled serpentine"), 0)
    L = int(wh.max())
    assert L > 1000, L
    assert upstream(ni, nj, names.index("filled serpentine"))[1] > 1000, "passes of the Jacobi iteration"
    assert rs.passes == passes_of(L) <= 14
    assert rs.cap == 15


def build():
    """The host checker: nmp_dev_basins.hpp compiled for the CPU.  Needs nothing of the engine library."""
    deps = [SRC, HEADER] + [os.path.join(CSRC, h) for h in ("nmp_dev_basins.hpp", "nmp_dev_flow_fill.hpp", "nmp_dev_routing.hpp")]
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
    V, I = C.c_void_p, C.c_int
    lib.basin_init_cells.argtypes = [I, I, V, V, V, V, V, I]
    lib.basin_init_cells.restype = None
    lib.basin_jump_cells.argtypes = [I, I, V, V]
    lib.basin_resolve_cells.argtypes = [I, I, V, V, V, I]
    lib.basin_jump_cells.restype = lib.basin_resolve_cells.restype = I
    return lib


_p = trt._p


def host_init(d, seed, flags):
    nj, ni = d.shape
    d = np.ascontiguousarray(d, np.uint8)
    state, label, dist = np.full(d.shape + (2,), WORD_POISON, I32), np.full(d.shape, WORD_POISON, I32), np.full(d.shape, WORD_POISON, I32)
    _host().basin_init_cells(ni, nj, _p(d), _p(np.ascontiguousarray(seed, I32)) if seed is not None else None, _p(state), _p(label), _p(dist), flags)
    return state, label, dist


def host_jump(state):
    nj, ni = state.shape[:2]
    old, new = np.ascontiguousarray(state, I32), np.full(state.shape, WORD_POISON, I32)
    return new, _host().basin_jump_cells(ni, nj, _p(old), _p(new))


def host_resolve(state, label, dist, reverse):
    nj, ni = state.shape[:2]
    st, l, dd = np.ascontiguousarray(state, I32), np.array(label, I32), np.array(dist, I32)
    return l, dd, _host().basin_resolve_cells(ni, nj, _p(st), _p(l), _p(dd), reverse)


@pytest.mark.parametrize("ni, nj", SHAPES)
def test_host_compilation_equals_the_restatement(ni, nj):
    """nmp_dev_basins.hpp compiled for the host: init, EVERY pass with its flag (the first three and all the others up to the fixed
    point, or to the cap on the planes with a cycle, whose state is compared there too) and resolve, with the cells visited in ascending
    and in descending order, equal the restatement in every word."""
    for what, d, seed, flags, pts, acyclic, rs, walked in combos(ni, nj):
        for got, want, nm in zip(host_init(d, seed, flags), rs.init, ("state", "label", "dist")):
            assert_words(got, want, "%s: %s of init" % (what, nm))
        for n in range(rs.passes):
            got, flag = host_jump(rs.states[n])
            assert_words(got, rs.states[n + 1], "%s: pass %d" % (what, n + 1))
            assert flag == rs.flags[n], (what, n)
        for reverse in (0, 1):
            l, dd, flag = host_resolve(rs.state, rs.init[1], rs.init[2], reverse)
            assert_words(l, rs.label, what + ": label")
            assert_words(dd, rs.dist, what + ": dist")
            assert flag == rs.resolve_flag


def test_a_state_nobody_initialised_is_never_followed():
    """Pointers outside 0 .. ni*nj-1 are copied by a pass and left alone by resolve, restated and compiled."""
    state = np.array([[[1, 1], [1, 0], [-4, 3], [3, 9], [2 ** 31 - 1, 1], [-2 ** 31, 0]]], I32)
    want, flag = np_basin_jump(state)
    got, gflag = host_jump(state)
    assert_words(got, want, "jump")
    assert (got[0, [2, 4, 5]] == state[0, [2, 4, 5]]).all() and got[0, 3].tolist() == [3, 18] and flag == gflag == 0
    label, dist = np.full((1, 6), PENDING, I32), np.full((1, 6), -1, I32)
    label[0, 1], dist[0, 1] = 4, 0
    l, dd, f = host_resolve(state, label, dist, 0)
    wl, wdd, wf = np_basin_resolve(state, label, dist)
    assert_words(l, wl, "label")
    assert_words(dd, wdd, "dist")
    assert l[0].tolist() == [4, 4, PENDING, CYCLE, PENDING, PENDING] and dd[0].tolist() == [1, 0, -1, -1, -1, -1] and f == wf == 1


def test_hops_saturate_on_a_cycle():
    """A 3-cycle on a window large enough for 2^31 hops to appear before the cap would need 2^31 cells; the saturation is shown on the
    state directly: sat(h + hh) in a pass and in resolve."""
    big = 2 ** 31 - 1
    state = np.array([[[1, big - 1], [2, 5], [2, 0]]], I32)
    want, _ = np_basin_jump(state)
    got, _ = host_jump(state)
    assert_words(got, want, "jump")
    assert got[0, 0].tolist() == [2, big] and got[0, 1].tolist() == [2, 5]
    label, dist = np.array([[PENDING, PENDING, 0]], I32), np.array([[-1, -1, 7]], I32)
    state = np.array([[[2, big - 3], [2, 5], [2, 0]]], I32)
    l, dd, f = host_resolve(state, label, dist, 1)
    assert l[0].tolist() == [0, 0, 0] and dd[0].tolist() == [big, 12, 7]
    assert_words(dd, np_basin_resolve(state, label, dist)[1], "dist")


@functools.lru_cache(maxsize=None)
def upstream(ni, nj, ci):
    """(acc, passes) of the existing restatement of noahmp_hip_flow_accumulate on case ci, made once."""
    return trt.np_upstream(np_inmask(dir_cases(ni, nj)[ci][1]))


def subtree_counts(rs_label, dg, ngauge):
    """Cells labelled g or labelled any gauge in g's subtree of downstream_gauge."""
    own = np.array([(rs_label == g).sum() for g in range(ngauge)], np.int64)
    out = own.copy()
    for g in range(ngauge):
        t, n = dg[g], 0
        while t >= 0:
            out[t] += own[g]
            t, n = dg[t], n + 1
            assert n <= ngauge
    return own, out


def np_downstream_gauge(d, pts, label):
    down = np_down(d)
    out = np.full(len(pts), -1, I32)
    for g, (i, j) in enumerate(pts):
        t = down[j, i]
        if t >= 0 and label.ravel()[t] >= 0:
            out[g] = label.ravel()[t]
    return out


@pytest.mark.parametrize("ni, nj", SHAPES)
def test_basin_sizes_equal_the_upstream_count(ni, nj):
    """The existing restatement np_upstream (the Jacobi iteration of noahmp_hip_flow_accumulate) at every gauge's cell equals the number of
    cells labelled with that gauge or with a gauge in its subtree; with every cell without a downstream cell a gauge, on the filled
    terrains, the incremental counts add up to ni*nj."""
    for ci, (name, d, flags, acyclic) in enumerate(dir_cases(ni, nj)):
        if not acyclic or flags:
            continue
        acc, npass = upstream(ni, nj, ci)
        for gi in (1, 2):
            what, d, seed, flags, pts, acyclic, rs, walked = combo(ni, nj, ci, gi)
            dg = np_downstream_gauge(d, pts, rs.label)
            own, whole = subtree_counts(rs.label, dg, len(pts))
            assert [int(acc[j, i]) for i, j in pts] == whole.tolist(), what
            assert npass >= int(rs.state[..., 1].max()) + 1, what           # a Jacobi pass per cell of the longest path
        if name.startswith("filled"):
            down = np_down(d)
            jj, ii = np.nonzero(down < 0)
            seed = np.full(d.shape, -1, I32)
            seed[jj, ii] = np.arange(jj.size)
            rs = Restated(d, seed, 0)
            assert (rs.label >= 0).all() and np.bincount(rs.label.ravel(), minlength=jj.size).sum() == ni * nj
            assert (np.bincount(rs.label.ravel(), minlength=jj.size) == acc[jj, ii]).all(), name


# ---------------------------------------------------------------------------------------------------------------- refusals and bindings
PLANES = ("dir", "seed", "state_old", "state_new", "label", "dist", "changed")
CALLS = ("noahmp_hip_flow_basin_init", "noahmp_hip_flow_basin_jump", "noahmp_hip_flow_basin_resolve")
REQUIRED = dict(noahmp_hip_flow_basin_init=("dir", "state_old", "label", "dist"), noahmp_hip_flow_basin_jump=("state_old", "state_new", "changed"),
                noahmp_hip_flow_basin_resolve=("state_old", "label", "dist", "changed"))


def _basin_block(ptrs, ni=5, nj=3, **kw):
    b = abi.FlowBasin()
    for k in PLANES:
        setattr(b, k, ptrs[k])
    b.ni, b.nj, b.flags, b.sweeps = ni, nj, 0, 1
    for k, v in kw.items():
        setattr(b, k, v)
    return b


def refusal_probes(ptrs):
    """[(site id, call, block or None)]: one probe per refusal site and per way into it."""
    out = []
    for fn in CALLS:
        short = fn.rsplit("_", 1)[1]
        out.append((short + ".null", fn, None))
        for field in REQUIRED[fn]:
            out.append(("%s.required.%s" % (short, field), fn, _basin_block(ptrs, **{field: None})))
        out.append((short + ".misaligned.state_old", fn, _basin_block(ptrs, state_old=ptrs["state_old"] + 4)))
        for nm, kw in (("ni", dict(ni=-1)), ("nj", dict(nj=-1)), ("big", dict(ni=65536, nj=32768))):
            out.append(("%s.window.%s" % (short, nm), fn, _basin_block(ptrs, **kw)))
        for nm, fl in (("low", 1), ("outlet", 15 | 16), ("high", 256), ("all", -1)):
            out.append(("%s.flags.%s" % (short, nm), fn, _basin_block(ptrs, flags=fl)))
        for nm, sw in (("zero", 0), ("negative", -3), ("above", MAX_SWEEPS + 1)):
            out.append(("%s.sweeps.%s" % (short, nm), fn, _basin_block(ptrs, sweeps=sw)))
    out.append(("jump.same", CALLS[1], _basin_block(ptrs, state_new=ptrs["state_old"])))
    out.append(("jump.misaligned.state_new", CALLS[1], _basin_block(ptrs, state_new=ptrs["state_new"] + 4)))
    out.append(("jump.same.tiled", CALLS[1], _basin_block(ptrs, state_new=ptrs["state_old"], sweeps=MAX_SWEEPS)))
    return out


def _refusals(lib, ptrs):
    """Every refusal: -105 and the full text of the fixture."""
    want = json.load(open(REFUSAL_FIXTURE))
    probes = refusal_probes(ptrs)
    assert sorted(want) == sorted(p[0] for p in probes)
    for site, fn, block in probes:
        rc = getattr(lib, fn)(C.byref(block) if block is not None else None, None)
        assert [rc, lib.noahmp_hip_last_error().decode()] == want[site], site
        assert rc == -105 and want[site][1].startswith(fn + ": "), site


def test_refusals_write_nothing():
    """Every refusal site of the three calls gives -105 and its full text (tests/golden/basins_refusal_text.json) before anything is
    launched or read: the planes here are host memory that the calls must not touch, and they keep their poison."""
    lib = abi.load_library()
    planes = {k: np.full(32, WORD_POISON, np.int64) for k in PLANES}
    _refusals(lib, {k: v.ctypes.data for k, v in planes.items()})
    assert all((p == WORD_POISON).all() for p in planes.values())
    text = json.load(open(REFUSAL_FIXTURE))
    assert len({tuple(v) for v in text.values()}) == 3 * 6 + 1, "the distinct texts: six per call and the jump's own"


HEADER_LINES = (
    "#define NOAHMP_HIP_HAS_FLOW_BASINS 1\n", "#define NOAHMP_FLOW_BASIN_MAX_SWEEPS ", "sweeps == 1, THE PINNED FORM", "sweeps > 1, THE TILED FORM",
    "h is at least the pinned", "#define NOAHMP_HIP_ABI_MINOR 3\n", "#define NOAHMP_BASIN_NONE     (-1)", "#define NOAHMP_BASIN_PENDING  (-2)",
    "#define NOAHMP_BASIN_CYCLE    (-3)", "typedef struct noahmp_flow_basin {", "} noahmp_flow_basin;",
    "(p, h) = old[c];  (pp, hh) = old[p];  new[c] = (pp, sat(h + hh));  *changed = 1 when pp != p.",
    "FREE      state = (down(c), 1)   label = NOAHMP_BASIN_PENDING   dist = -1", "TERMINAL  state = (c, 0)         label = NOAHMP_BASIN_NONE      dist = 0",
    "ceil(log2(ni*nj)) + 1 passes", "Roots are only read and the other cells only written", "A byte", "outside 0..8 counts as 0",
    "A cycle that crosses ranks stays NOAHMP_BASIN_PENDING") + tuple("int    %s(const noahmp_flow_basin* b, void* stream);" % c for c in CALLS) + tuple(
        "#define NOAHMP_BASIN_RING_%s " % s for s in "WESN")
FIELDS = ["dir", "seed", "state_old", "state_new", "label", "dist", "changed", "ni", "nj", "flags", "sweeps"]


def test_bindings_regenerate_identically_with_the_basin_calls():
    from tools import gen_abi
    for rel, text in (("include/noahmp_hip.h", gen_abi.c_header()), ("oracle/ref_harness_gen.f90", gen_abi.ref_harness()),
                      ("noahmp_amd/fortran/module_sf_noahmpdrv_hip.F90", gen_abi.fortran_shim()),
                      ("tests/fortran/shim_wrap_gen.f90", gen_abi.shim_wrap())):
        assert open(os.path.join(ROOT, rel)).read() == text, rel
    hdr = open(HEADER).read()
    for word in HEADER_LINES:
        assert word in hdr, word
    assert "\n".join(gen_abi.flow_basin_header()) in hdr
    assert "noahmp_flow_basin" not in gen_abi.ref_harness() and "noahmp_flow_basin" not in gen_abi.shim_wrap()
    f90 = open(os.path.join(ROOT, "noahmp_amd", "fortran", "module_sf_noahmpdrv_hip.F90")).read()
    for word in tuple("bind(C, name='%s')" % c for c in CALLS) + ("type, bind(C) :: noahmp_flow_basin ", "NOAHMP_BASIN_RING_N = 128", "NOAHMP_BASIN_CYCLE = -3"):
        assert word in f90, word
    for sym in CALLS:
        assert sym in abi.EXPORTED_SYMBOLS
    assert [n for n, _ in abi.FlowBasin._fields_] == FIELDS
    assert abi.BASIN_FLAG == {"ring_" + s: v for s, v in RING.items()}
    assert (abi.BASIN_NONE, abi.BASIN_PENDING, abi.BASIN_CYCLE) == (NONE, PENDING, CYCLE) and abi.BASIN_MAX_SWEEPS == MAX_SWEEPS >= 12


def test_ctypes_mirror_matches_the_compiled_header(tmp_path):
    names = [n for n, _ in abi.FlowBasin._fields_]
    body = 'printf(" %zu", sizeof(noahmp_flow_basin));' + "".join('printf(" %%zu", offsetof(noahmp_flow_basin, %s));' % n for n in names)
    want = [C.sizeof(abi.FlowBasin)] + [getattr(abi.FlowBasin, n).offset for n in names]
    macros = ["NOAHMP_HIP_ABI_MINOR", "NOAHMP_HIP_HAS_FLOW_BASINS", "NOAHMP_BASIN_NONE", "NOAHMP_BASIN_PENDING", "NOAHMP_BASIN_CYCLE", "NOAHMP_FLOW_BASIN_MAX_SWEEPS"] + [
        "NOAHMP_BASIN_RING_%s" % s for s in "WESN"] + ["NOAHMP_BASIN_RING_W == NOAHMP_FILL_RING_W && NOAHMP_BASIN_RING_N == NOAHMP_FILL_RING_N"]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "noahmp_hip.h"\nint main(){' + body +
                   "".join('printf(" %%d", %s);' % m for m in macros) + " return 0;}")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert out == want + [3, 1, NONE, PENDING, CYCLE, MAX_SWEEPS] + [RING[s] for s in "wesn"] + [1]


def test_library_exports_the_basin_calls():
    if not os.path.exists(abi.LIB_PATH):
        from noahmp_amd import build as b
        b.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", abi.LIB_PATH]).decode()
    for sym in CALLS:
        assert " T %s\n" % sym in out, sym


@pytest.mark.skipif(tr._flang() is None, reason="no flang")
def test_generated_fortran_type_and_interfaces_compile(tmp_path):
    """The basin part of the generated module compiles, and a caller of the three interfaces type-checks."""
    from tools import gen_abi
    text = "\n".join(["module flow_basin_abi_check", "  use iso_c_binding", "  implicit none"] + gen_abi.flow_basin_f90_types() + ["  interface"] +
                     gen_abi.flow_basin_f90_interfaces() +
                     ["  end interface", "contains", "  function go(planes) result(rc)", "    type(c_ptr), intent(in) :: planes(7)",
                      "    type(noahmp_flow_basin) :: b", "    integer(c_int) :: rc",
                      "    b%dir = planes(1); b%seed = c_null_ptr; b%state_old = planes(3); b%state_new = planes(4); b%label = planes(5)",
                      "    b%dist = planes(6); b%changed = planes(7); b%ni = 64; b%nj = 8; b%sweeps = NOAHMP_FLOW_BASIN_MAX_SWEEPS",
                      "    b%flags = ior(NOAHMP_BASIN_RING_W, NOAHMP_BASIN_RING_N)",
                      "    rc = noahmp_hip_flow_basin_init(b, c_null_ptr)", "    rc = noahmp_hip_flow_basin_jump(b, c_null_ptr)",
                      "    rc = noahmp_hip_flow_basin_resolve(b, c_null_ptr)",
                      "    if (NOAHMP_BASIN_CYCLE /= -3) rc = -1",
                      "  end function go", "end module flow_basin_abi_check", ""])
    f = tmp_path / "flow_basin_abi_check.f90"
    f.write_text(text)
    subprocess.check_call([tr._flang(), "-c", str(f), "-o", str(tmp_path / "flow_basin_abi_check.o"), "-J", str(tmp_path)], cwd=str(tmp_path))


def test_nested_sums_on_the_host():
    """Basins.nested and Basins.downstream_gauge on planes given by hand (no device): a chain 2 -> 1 -> 0 with gauge 3 apart."""
    import types
    from noahmp_amd.routing import Basins
    b = Basins.__new__(Basins)
    b.ngauge = 4
    b.downstream_gauge = types.MethodType(lambda self: np.array([-1, 0, 1, -1], I32), b)
    got = b.nested(np.array([[10, 5, 2, 7], [1, 1, 1, 1]], np.int64))
    assert got.tolist() == [[17, 7, 2, 7], [3, 2, 1, 1]]


# ---------------------------------------------------------------------------------------------------------------- GPU
_dev = tr._dev


def _state64(state):
    """[nj, ni, 2] int32 -> [nj, ni] int64, the packed word."""
    return np.ascontiguousarray(state, I32).view(np.int64)[..., 0]


class _Gpu:
    """The device planes of one case at odd offsets inside poisoned pools, and the calls on them one by one."""

    def __init__(self, engine, d, seed, flags):
        import torch
        self.engine, self.torch = engine, torch
        nj, ni = d.shape
        self.shape, self.n = (nj, ni), ni * nj
        self.spool, (s0, s1) = trt._pool(self.n, 2, torch.int64, STATE_POISON)
        self.wpool, (lb, ds, sd) = trt._pool(self.n, 3, torch.int32, WORD_POISON)
        self.bpool, (dr,) = trt._pool(self.n, 1, torch.uint8, 0xEE)
        self.ipool, (ch,) = trt._pool(1, 1, torch.int32, 77)
        self.state, self.cur = [s0.view(nj, ni), s1.view(nj, ni)], 0
        self.label, self.dist, self.changed = lb.view(nj, ni), ds.view(nj, ni), ch
        self.dir = dr.view(nj, ni)
        self.dir.copy_(_dev(np.ascontiguousarray(d)))
        self.seed = None
        if seed is not None:
            self.seed = sd.view(nj, ni)
            self.seed.copy_(_dev(np.ascontiguousarray(seed)))
        self.seed_h, self.flags = seed, int(flags)
        torch.cuda.synchronize()

    def block(self, sweeps=1):
        return self.engine.flow_basin_block(self.dir, self.state[self.cur], self.state[1 - self.cur], self.label, self.dist, self.changed,
                                            flags=self.flags, seed=self.seed, sweeps=sweeps)

    def _state(self, k):
        return self.state[k].cpu().numpy().view(I32).reshape(self.shape + (2,))

    def init(self):
        self.engine.flow_basin_init(self.block())
        self.engine.stream_sync()
        return self._state(self.cur), self.label.cpu().numpy(), self.dist.cpu().numpy()

    def put(self, state, label=None, dist=None):
        self.state[self.cur].copy_(_dev(_state64(state)))
        if label is not None:
            self.label.copy_(_dev(np.ascontiguousarray(label)))
            self.dist.copy_(_dev(np.ascontiguousarray(dist)))
        self.torch.cuda.synchronize()

    def jump(self, sweeps=1):
        self.changed.zero_()
        self.torch.cuda.synchronize()
        self.engine.flow_basin_jump(self.block(sweeps))
        self.engine.stream_sync()
        self.cur = 1 - self.cur
        return self._state(self.cur), int(self.changed.item())

    def resolve(self):
        self.changed.zero_()
        self.torch.cuda.synchronize()
        self.engine.flow_basin_resolve(self.block())
        self.engine.stream_sync()
        return self.label.cpu().numpy(), self.dist.cpu().numpy(), int(self.changed.item())

    def guards_ok(self):
        ok = trt._guards_ok(self.spool, self.n, STATE_POISON) and trt._guards_ok(self.bpool, self.n, 0xEE) and trt._guards_ok(self.ipool, 1, 77)
        w = self.wpool.cpu().numpy()
        ok = ok and (w[:, :trt.PAD] == WORD_POISON).all() and (w[:, trt.PAD + self.n:] == WORD_POISON).all()
        return ok and (self.seed is not None or (w[2] == WORD_POISON).all())


@pytest.mark.gpu
@pytest.mark.parametrize("ni, nj", SHAPES)
def test_gpu_calls_equal_the_restatement(engine, ni, nj):
    """Every case and gauge set: state, label and dist after noahmp_hip_flow_basin_init, the state and the flag after each of the first 3
    passes, a pass at the fixed point (the flag is left alone, the state kept), and resolve on the restatement's final state (the capped
    one where the plane has a cycle) equal the restatement in every word; resolve again changes nothing; dir and seed are not written;
    guard words keep their poison."""
    for what, d, seed, flags, pts, acyclic, rs, walked in combos(ni, nj):
        g = _Gpu(engine, d, seed, flags)
        for got, want, nm in zip(g.init(), rs.init, ("state", "label", "dist")):
            assert_words(got, want, "%s: %s of init" % (what, nm))
        for n in range(min(3, rs.passes)):
            got, flag = g.jump()
            assert_words(got, rs.states[n + 1], "%s: pass %d" % (what, n + 1))
            assert flag == rs.flags[n], (what, n)
        if rs.converged:
            g.put(rs.state)
            got, flag = g.jump()
            assert flag == 0, what
            if not (rs.label == CYCLE).any():
                assert_words(got, rs.state, what + ": the fixed point")
        g.put(rs.state, rs.init[1], rs.init[2])
        l, dd, flag = g.resolve()
        assert_words(l, rs.label, what + ": label")
        assert_words(dd, rs.dist, what + ": dist")
        assert flag == rs.resolve_flag, what
        l, dd, flag = g.resolve()
        assert flag == 0
        assert_words(l, rs.label, what + ": label, resolved twice")
        assert_words(g._state(g.cur), rs.state, what + ": resolve keeps the state")
        assert_same_bytes(g.dir.cpu().numpy(), d, what + ": dir")
        assert g.guards_ok(), what


def lifting(succ):
    """succ^(2^b) for b = 0..30, flat."""
    out = [succ]
    for b in range(30):
        out.append(out[-1][out[-1]])
    return out


def kth_below(lift, hops):
    """The cell `hops` steps along succ from every cell."""
    c = np.arange(lift[0].size)
    for b, t in enumerate(lift):
        c = np.where((hops >> b) & 1, t[c], c)
    return c


def check_tiled_call(what, lift, old, new, flag):
    """What pins one call of the tiled form: every word is (the cell h hops below, h) unless h is saturated; h is at least the pinned
    pass's from the same state_old; the flag says whether a pointer moved."""
    ptr, hops = new[..., 0].ravel().astype(np.int64), new[..., 1].ravel().astype(np.int64)
    exact = hops < SAT
    assert (hops >= 0).all() and (kth_below(lift, hops)[exact] == ptr[exact]).all(), what + ": a word that is no (cell h hops below, h)"
    pinned, _ = np_basin_jump(old)
    assert (hops >= pinned[..., 1].ravel()).all(), what + ": fewer hops than the pinned pass"
    assert flag == int((new[..., 0] != old[..., 0]).any()), what + ": changed"


@pytest.mark.gpu
@pytest.mark.parametrize("sweeps", SWEEPS)
@pytest.mark.parametrize("ni, nj", SHAPES)
def test_gpu_tiled_form(engine, ni, nj, sweeps):
    """The tiled form of the pass, every case without gauges and with the nested set: after EVERY call the three properties that pin it
    hold against the restatement; it reaches a call that moves nothing in no more calls than the pinned form needs passes (where a
    cycle keeps the pinned form moving up to its cap, it stops there at the latest); there the state equals the pinned form's wherever no cycle exists, and resolve gives
    the pinned form's label and dist in every word."""
    for ci in range(len(dir_cases(ni, nj))):
        for gi in (0, 2):
            what, d, seed, flags, pts, acyclic, rs, (wl, wd, wh) = combo(ni, nj, ci, gi)
            what += ", sweeps %d" % sweeps
            lift = lifting(rs.init[0][..., 0].ravel().astype(np.int64))
            g = _Gpu(engine, d, seed, flags)
            old = g.init()[0]
            calls = 0
            while calls < rs.passes:
                new, flag = g.jump(sweeps)
                calls += 1
                check_tiled_call("%s, call %d" % (what, calls), lift, old, new, flag)
                old = new
                if not flag:
                    break
            # on a cycle several doublings in one call can bring a pointer back to where it was, so the tiled form may stop where the pinned
            # form runs to its cap: every cell outside a cycle has moved to its root by then, which is all resolve needs
            assert flag == 0 or not rs.converged, "%s: still moving after %d calls, the pinned form needs %d passes" % (what, calls, rs.passes)
            ok = wh >= 0
            assert_words(old[ok], rs.state[ok], what + ": the state where no cycle exists")
            l, dd, rflag = g.resolve()
            assert_words(l, rs.label, what + ": label")
            assert_words(dd, rs.dist, what + ": dist")
            assert g.guards_ok(), what


def _net(engine, d, tile=None, origin=(0, 0)):
    """A FlowNetwork over the window d of directions; tile: (ni, nj) of the tile, default the window itself.  Bytes above 8 become 0, as the
    contract reads them."""
    from noahmp_amd.routing import FlowNetwork
    nj, ni = d.shape
    ti, tj = tile or (ni, nj)
    net = FlowNetwork(engine, ti, tj)
    net.set_directions(_dev(np.where(d <= 8, d, 0).astype(np.uint8)), origin=origin)
    return net


@pytest.mark.gpu
def test_gpu_basins_run(engine):
    """Basins.run on the 70 x 130 serpentine reaches the walker's planes with passes == the restatement's <= 14 whatever the batch
    size; on the planes with cycles it raises under strict=True, naming the count, and marks exactly the walker's cells under
    strict=False; set_outlet_gauges on the filled hills labels every cell."""
    from noahmp_amd.routing import Basins
    ni, nj = CUT
    names = [c[0] for c in dir_cases(ni, nj)]
    for gi in range(len(GAUGES)):
        what, d, seed, flags, pts, acyclic, rs, (wl, wd, wh) = combo(ni, nj, names.index("filled serpentine"), gi)
        for check in (1, 4, 32):
            b = Basins(_net(engine, d))
            b.set_gauges(pts)
            assert b.ngauge == len(pts) and b.cap == rs.cap
            b.run(check=check, sweeps=1)
            assert_words(b.label.cpu().numpy(), wl, what + ": label")
            assert_words(b.hops.cpu().numpy(), wd, what + ": hops")
            assert b.passes == rs.passes <= 14 and b.rounds == 1, (b.passes, rs.passes)
            b.run(check=check)                                            # the default: the first call is the tiled form
            assert_words(b.label.cpu().numpy(), wl, what + ": label, default")
            assert_words(b.hops.cpu().numpy(), wd, what + ": hops, default")
            assert b.passes <= rs.passes
        for sweeps, tiled_calls in ((MAX_SWEEPS, 1), (MAX_SWEEPS, None), (3, 2)):
            b.run(sweeps=sweeps, tiled_calls=tiled_calls)
            assert_words(b.label.cpu().numpy(), wl, what + ": label, tiled")
            assert_words(b.hops.cpu().numpy(), wd, what + ": hops, tiled")
            assert b.passes <= rs.passes, (sweeps, tiled_calls, b.passes, rs.passes)
        assert b.passes < rs.passes, "in-tile contraction saves no pass on the corridor"
        assert_words(b.downstream_gauge(), np_downstream_gauge(d, pts, wl), what)
    for cname in ("random bytes", "hand-made cycles"):
        what, d, seed, flags, pts, acyclic, rs, (wl, wd, wh) = combo(ni, nj, names.index(cname), 2)
        d0 = np.where(d <= 8, d, 0).astype(np.uint8)
        ncyc = int((wh < 0).sum())
        assert ncyc > 0
        b = Basins(_net(engine, d0))
        b.set_gauges(pts)
        with pytest.raises(RuntimeError, match="%d cells of the tile end on a cycle of the directions and 0 are pending" % ncyc):
            b.run()
        for sweeps in (1, None):
            b.run(strict=False, sweeps=sweeps)
            assert ((b.label.cpu().numpy() == CYCLE) == (wh < 0)).all(), what
            assert_words(b.label.cpu().numpy(), wl, what + ": label")
            assert_words(b.hops.cpu().numpy(), wd, what + ": hops")
            assert b.passes <= rs.passes <= b.cap and b.unresolved() == (ncyc, 0)
            assert sweeps is None or b.passes == rs.passes
    d = dir_cases(67, 35)[1][1]
    b = Basins(_net(engine, d))
    outlets = b.set_outlet_gauges()
    b.run()
    down = np_down(d)
    assert outlets == [(int(i), int(j)) for j, i in zip(*np.nonzero(down < 0))]
    lab = b.region_map().cpu().numpy()
    acc, _ = trt.np_upstream(np_inmask(d))
    assert lab.dtype == I32 and (lab >= 0).all() and (np.bincount(lab.ravel(), minlength=len(outlets)) == acc[down < 0]).all()
    assert (b.downstream_gauge() == -1).all()


def _ownership_changes(d, part_of, wh):
    """The largest number of changes of the owning part along any flow path that reaches a root (wh >= 0: the walker's hops)."""
    down = np_down(d).ravel()
    own = part_of.ravel()
    ch = np.zeros(down.size, np.int64)
    order = np.argsort(wh.ravel(), kind="stable")
    for c in order.tolist():
        if wh.ravel()[c] > 0:
            t = down[c]
            ch[c] = ch[t] + (own[c] != own[t])
    return int(ch.max())


class _RingFromWhole:
    """A stand-in for Comm in one process: exchange_halo copies the ring of label and dist (float32 views of int32 words) from the
    whole-domain planes, ENQUEUED ONLY on torch's current stream; agree_any returns its argument."""

    def __init__(self, whole, blk, ring):
        self.whole, self.blk, self.ring, self.calls = whole, blk, ring, 0

    def exchange_halo(self, planes, geom):
        import torch
        assert len(planes) == 2 and geom == "geom" and all(p.dtype == torch.float32 for p in planes)
        for p, w in zip(planes, self.whole):
            v = p.view(torch.int32)
            v.copy_(torch.where(self.ring, w[self.blk], v))
        self.calls += 1

    def agree_any(self, flag):
        return flag


def _decomposed(engine, d, seed, want_label, want_dist, wh, what, expect_pending=0):
    """d cut 2 x 2: four Basins on their blocks, rings copied by slicing before every resolve, until no part changes."""
    import torch
    from noahmp_amd.routing import Basins
    nj, ni = d.shape
    parts, part_of = [], np.zeros(d.shape, np.int64)
    for n, (tile, blk, bidx) in enumerate(tsh._cuts(ni, nj, 1)):
        part_of[tile] = n
        own = (slice(tile[0].start - blk[0].start, tile[0].stop - blk[0].start), slice(tile[1].start - blk[1].start, tile[1].stop - blk[1].start))
        net = _net(engine, d[blk], tile=(tile[1].stop - tile[1].start, tile[0].stop - tile[0].start), origin=(own[1].start, own[0].start))
        assert net.block_shape == d[blk].shape
        b = Basins(net)
        if seed is not None:
            b.set_gauges(np.ascontiguousarray(seed[blk]))
        assert sorted(b.ring_sides()) == sorted(tff._ring_sides(tile, blk)) and len(b.ring_sides()) == 2
        with pytest.raises(ValueError, match="comm"):
            b.run()
        b.begin()
        assert b.contract()
        assert b.passes <= cap_of(d[blk].size)
        parts.append((b, tile, blk, own, _dev(bidx < 0)))
    GL = torch.full((nj, ni), PENDING, dtype=torch.int32, device="cuda")
    GD = torch.full((nj, ni), -1, dtype=torch.int32, device="cuda")
    rounds = 0
    bound = _ownership_changes(d, part_of, wh) + 2
    while True:
        for b, tile, blk, own, ring in parts:
            GL[tile], GD[tile] = b.label[own], b.hops[own]
        for b, tile, blk, own, ring in parts:                             # the exchange: the ring from the owners
            b.label.copy_(torch.where(ring, GL[blk], b.label))
            b.hops.copy_(torch.where(ring, GD[blk], b.hops))
        torch.cuda.synchronize()
        rounds += 1
        if not any([b.resolve() for b, *_ in parts]):
            break
        assert rounds < bound, "%s: more rounds than ownership changes + 2 = %d" % (what, bound)
    assert rounds <= bound
    for b, tile, blk, own, ring in parts:
        assert b.rounds == rounds
        assert_words(b.label.cpu().numpy(), want_label[blk], "%s: label of part %s after %d rounds, ring included" % (what, tile, rounds))
        assert_words(b.hops.cpu().numpy(), want_dist[blk], "%s: hops of part %s, ring included" % (what, tile))
    assert sum(b.unresolved()[1] for b, *_ in parts) == expect_pending
    return parts, rounds, bound


@pytest.mark.gpu
def test_gpu_decomposition(engine):
    """70 x 130 cut 2 x 2 in one process.  The filled hills with five gauges: every part equals the whole on its block, ring included,
    within ownership changes + 2 rounds; then Basins.run(comm=stand-in) per part on a side stream.  The filled serpentine, whose corridor
    re-enters every part many times.  A 2-cycle laid across the cut: its cells and everything above them end as PENDING in the parts
    (CYCLE in the whole), and strict=True says so."""
    import torch
    from noahmp_amd.routing import Basins
    ni, nj = CUT
    names = [c[0] for c in dir_cases(ni, nj)]
    what, d, seed, flags, pts, acyclic, rs, (wl, wd, wh) = combo(ni, nj, names.index("filled hills"), 2)
    assert len(pts) == 5
    parts, rounds, bound = _decomposed(engine, d, seed, wl, wd, wh, what)
    assert 2 <= rounds <= bound
    whole = [_dev(wl), _dev(wd)]
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    for b0, tile, blk, own, ring in parts:
        comm = _RingFromWhole(whole, blk, ring)
        b = Basins(b0.net)
        b.set_gauges(np.ascontiguousarray(seed[blk]))
        with torch.cuda.stream(side):
            b.run(comm=comm, geom="geom", sweeps=MAX_SWEEPS if tile[0].start else 1)      # two parts with the tiled form
        engine.stream_sync()
        torch.cuda.synchronize()
        assert comm.calls == b.rounds == 2
        assert_words(b.label.cpu().numpy(), wl[blk], "run(comm) of part %s: label" % (tile,))
        assert_words(b.hops.cpu().numpy(), wd[blk], "run(comm) of part %s: hops" % (tile,))
        assert_words(b.region_map().cpu().numpy(), wl[tile], "region_map of part %s" % (tile,))
    what, d, seed, flags, pts, acyclic, rs, (wl, wd, wh) = combo(ni, nj, names.index("filled serpentine"), 2)
    parts, rounds, bound = _decomposed(engine, d, seed, wl, wd, wh, what + " (paths re-enter the parts)")
    assert rounds > 10, "the corridor crosses the cut in every leg"
    what, d, seed, flags, pts, acyclic, rs, walked = combo(ni, nj, names.index("filled hills"), 1)
    d = d.copy()
    d[40, ni // 2 - 1], d[40, ni // 2] = 1, 5                             # a 2-cycle across the cut between the two western and eastern parts
    wl, wd, wh = walk(d, seed, 0)
    ncyc = int((wh < 0).sum())
    assert ncyc >= 2 and (wl[wh < 0] == CYCLE).all()
    pl, pd = np.where(wh < 0, PENDING, wl).astype(I32), wd
    wh_parts = np.where(wh < 0, 0, wh)                                    # no round is spent on them
    parts, rounds, bound = _decomposed(engine, d, seed, pl, pd, wh_parts, "a cycle across the cut", expect_pending=ncyc)
    b0, tile, blk, own, ring = parts[0]
    b = Basins(b0.net)
    b.set_gauges(np.ascontiguousarray(seed[blk]))
    npend = int((pl[tile] == PENDING).sum())
    assert npend > 0
    with pytest.raises(RuntimeError, match="0 cells of the tile end on a cycle of the directions and %d are pending" % npend):
        b.run(comm=_RingFromWhole([_dev(pl), _dev(pd)], blk, ring), geom="geom")


class _Store:
    """What Regions needs of a store: a unit field and an index block in which every cell takes part."""

    def __init__(self, ni, nj):
        import torch
        self.ni, self.nj, self.device = ni, nj, torch.device("cuda")
        self.a = dict(one=torch.ones((nj, ni), dtype=torch.float32, device="cuda"), xland=torch.ones((nj, ni), dtype=torch.float32, device="cuda"),
                      xice=torch.zeros((nj, ni), dtype=torch.float32, device="cuda"))
        torch.cuda.synchronize()

    def step_args(self, *a):
        return tg._block(self.ni, self.nj, self.a["xland"], self.a["xice"])


@pytest.mark.gpu
def test_gpu_hand_over_to_regions(engine):
    """67 x 35, the filled hills with five nested gauges: Regions accepts Basins.region_map(); the sum of a unit field per gauge is the
    number of cells labelled with it; with FlowNetwork.step at release = 1 and unit input, out at every gauge's cell converges to
    Basins.nested of those counts."""
    import types
    import torch
    from noahmp_amd.history import Regions
    from noahmp_amd.routing import Basins
    ni, nj = 67, 35
    what, d, seed, flags, pts, acyclic, rs, (wl, wd, wh) = combo(ni, nj, 1, 2)
    assert len(pts) == 5
    net = _net(engine, d)
    b = Basins(net)
    b.set_gauges(pts)
    b.run()
    rmap = b.region_map()
    assert rmap.dtype == torch.int32 and tuple(rmap.shape) == (nj, ni)
    assert_words(rmap.cpu().numpy(), wl, "region_map")
    store = _Store(ni, nj)
    rg = Regions(engine, store, rmap, b.ngauge, nslot=1)
    rg.add("cells", "one")
    rg.step()
    counts = rg.read()["cells"][0]
    own = np.array([(wl == g).sum() for g in range(len(pts))], np.float64)
    assert (counts == own).all() and own.min() >= 1, (counts, own)
    whole = b.nested(counts)
    acc, npass = trt.np_upstream(np_inmask(d))
    assert whole.tolist() == [float(acc[j, i]) for i, j in pts]
    assert (whole > counts).any(), "no gauge above another: nothing is nested"
    net.set_area(1.0)
    net.set_release(1.0)
    net.set_input_columns(None)
    one = torch.ones(ni * nj, dtype=torch.float32, device="cuda")
    st = types.SimpleNamespace(ni=ni, nj=nj, a=dict(runsfxy=one))
    torch.cuda.synchronize()
    for _ in range(npass):
        net.step(st, 1000.0, fields=("runsfxy",))                         # scale = 1.0: one unit per cell and call
    engine.stream_sync()
    out = net.out[net.cur].cpu().numpy()
    assert [float(out[j, i]) for i, j in pts] == whole.tolist()


@pytest.mark.gpu
def test_gpu_refusals_launch_nothing(engine):
    """The refusals with device planes: -105, the full text, and every plane keeps its poison; an empty window is no refusal and writes
    nothing."""
    import torch
    pl = torch.full((len(PLANES), 32), WORD_POISON, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ptrs = {k: pl[n].data_ptr() for n, k in enumerate(PLANES)}
    _refusals(engine.lib, ptrs)
    for kw in (dict(nj=0), dict(ni=0), dict(ni=0, nj=0)):
        b = _basin_block(ptrs, **kw)
        for fn in CALLS:
            assert getattr(engine.lib, fn)(C.byref(b), None) == 0
    engine.stream_sync()
    torch.cuda.synchronize()
    assert (pl.cpu().numpy() == WORD_POISON).all()


if __name__ == "__main__":                                                # PYTHONPATH=.:tests python tests/test_basins.py records the refusal texts
    lib = abi.load_library()
    planes = {k: np.full(32, WORD_POISON, np.int64) for k in PLANES}
    out = {}
    for site, fn, block in refusal_probes({k: v.ctypes.data for k, v in planes.items()}):
        rc = getattr(lib, fn)(C.byref(block) if block is not None else None, None)
        out[site] = [rc, lib.noahmp_hip_last_error().decode()]
    json.dump(out, open(REFUSAL_FIXTURE, "w"), indent=1, sort_keys=True)
    print("%s: %d sites" % (REFUSAL_FIXTURE, len(out)))
