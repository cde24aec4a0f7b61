"""Upstream sums on the D8 network on the device (noahmp_hip_flow_upstream_init / _pass; nmp_dev_accum.hpp; routing.Upstream).

No reference routine stands behind the calls; the contract is the text in include/noahmp_hip.h.  np_up_init / np_up_pass restate it in
numpy; sequential() is an independent method, an accumulation in topological order with Python integers.  Every word is an integer, all
arithmetic is mod 2^64 and the one atomic is an integer add, so everything is compared word for word: no tolerance appears anywhere.
The pass counts are derived (bit_length(L) + 1 for a longest path of L hops) and asserted."""
import ctypes as C
import functools
import json
import os
import subprocess

import numpy as np
import pytest

from noahmp_amd import abi
import test_basins as tb
import test_flow_fill as tff
import test_regrid as tr
import test_routing as trt
import test_shadow as tsh
from test_basins import assert_words, cap_of

ROOT = tr.ROOT
CSRC = tr.CSRC
SRC = os.path.join(ROOT, "tests", "host_emul", "upstream_check.hip")
LIB = os.path.join(ROOT, "tests", "host_emul", "libupstream_check.so")
HEADER = tff.HEADER
REFUSAL_FIXTURE = os.path.join(ROOT, "tests", "golden", "upstream_refusal_text.json")
I32, U32, U64 = np.int32, np.uint32, np.uint64
RING = tff.RING
# (ni, nj): a lone cell, one column, one row, more than one workgroup with odd sizes
SHAPES = [(1, 1), (1, 9), (9, 1), (67, 35), (300, 7)]
STATE_POISON, WORD_POISON = 0x0707070707070707, 0x07070707
MASK = (1 << 64) - 1


def passes_of(L):
    """bit_length(L) + 1 for a longest path of L >= 1 hops, 1 for L = 0: the pushing passes and the one that only folds."""
    return int(L).bit_length() + 1


# ---------------------------------------------------------------------------------------------------------------- the restatement
def ring_mask(shape, flags):
    nj, ni = shape
    jj, ii = np.meshgrid(np.arange(nj), np.arange(ni), indexing="ij")
    side = (ii == 0) * 1 | (ii == ni - 1) * 2 | (jj == 0) * 4 | (jj == nj - 1) * 8
    return (side & (flags >> 4)) != 0


def np_up_init(d, weight, inflow, flags):
    """(sum uint64, jump int32), flat, of noahmp_hip_flow_upstream_init; both pend planes are 0."""
    ring = ring_mask(d.shape, flags).ravel()
    down = tb.np_down(d).ravel()
    t_ring = ring[np.where(down >= 0, down, 0)]
    jump = np.where((down >= 0) & ~t_ring, down, -1).astype(I32)
    w = np.ones(d.size, U64) if weight is None else weight.ravel().astype(U64)
    q = np.zeros(d.size, U64) if inflow is None else inflow.ravel().astype(U64)
    return np.where(ring, q, w).astype(U64), jump


def np_up_pass(s, pend_in, pend_out, jump_old):
    """One pass: (sum, pend_in, pend_out, jump_new, changed)."""
    n = s.size
    with np.errstate(over="ignore"):
        s = s + pend_in
    j = jump_old.astype(np.int64)
    ok = (j >= 0) & (j < n)
    out = pend_out.copy()
    np.add.at(out, j[ok], s[ok])                                         # uint64: wraps mod 2^64
    return s, np.zeros(n, U64), out, np.where(ok, jump_old[np.where(ok, j, 0)], -1).astype(I32), int(ok.any())


class Restated:
    """init and every pass up to the first in which nobody pushes (or the cap), by the restatement.  states[k]: the five PHYSICAL planes
    (sum, pend[0], pend[1], jump[0], jump[1]) after k passes, the caller's swaps made; out[k]: which pend plane took the pushes of pass k.
    jump[1] holds the test's poison until pass 1 writes it, as on the device."""

    def __init__(self, d, weight=None, inflow=None, flags=0):
        s, jump = np_up_init(d, weight, inflow, flags)
        n = d.size
        self.cap = cap_of(n)
        P, J, cur = [np.zeros(n, U64), np.zeros(n, U64)], [jump, np.full(n, WORD_POISON, I32)], 0
        self.states, self.flags, self.out = [(s, P[0], P[1], J[0], J[1])], [], [None]
        self.converged = False
        while len(self.flags) < self.cap:
            s, P[cur], P[1 - cur], J[1 - cur], flag = np_up_pass(s, P[cur], P[1 - cur], J[cur])
            self.out.append(1 - cur)
            cur = 1 - cur
            self.states.append((s, P[0], P[1], J[0], J[1]))
            self.flags.append(flag)
            if not flag:
                self.converged = True
                break
        self.passes = len(self.flags)
        self.sum = s
        for st in self.states:
            for a in st:
                a.setflags(write=False)


NAMES = ("sum", "pend[0]", "pend[1]", "jump[0]", "jump[1]")


# ---------------------------------------------------------------------------------------------------------------- the independent method
def sequential(d, weight=None, inflow=None, flags=0):
    """Accumulation in topological order (Kahn), one cell at a time, Python integers mod 2^64: (sums uint64 [nj, ni], done bool -- False
    on a cycle, where no order exists --, the longest path L in hops).  The network is restated here on its own: a ring cell starts
    with its inflow, and an edge into a ring cell does not exist."""
    nj, ni = d.shape
    n = ni * nj
    dl = d.ravel().tolist()

    def is_ring(i, j):
        return bool((flags & RING["w"] and i == 0) or (flags & RING["e"] and i == ni - 1) or (flags & RING["s"] and j == 0) or (flags & RING["n"] and j == nj - 1))

    down, val = [-1] * n, [0] * n
    wl = None if weight is None else weight.ravel().tolist()
    ql = None if inflow is None else inflow.ravel().tolist()
    for c in range(n):
        j, i = divmod(c, ni)
        val[c] = (int(ql[c]) if ql is not None else 0) if is_ring(i, j) else (int(wl[c]) if wl is not None else 1)
        k = dl[c]
        if 1 <= k <= 8:
            i2, j2 = i + trt.DI[k - 1], j + trt.DJ[k - 1]
            if 0 <= i2 < ni and 0 <= j2 < nj and not is_ring(i2, j2):
                down[c] = j2 * ni + i2
    indeg = [0] * n
    for t in down:
        if t >= 0:
            indeg[t] += 1
    height, done = [0] * n, [False] * n
    stack = [c for c in range(n) if indeg[c] == 0]
    while stack:
        c = stack.pop()
        done[c] = True
        t = down[c]
        if t >= 0:
            val[t] = (val[t] + val[c]) & MASK
            height[t] = max(height[t], height[c] + 1)
            indeg[t] -= 1
            if indeg[t] == 0:
                stack.append(t)
    return np.array(val, U64).reshape(nj, ni), np.array(done).reshape(nj, ni), max(height)


def partial_sums(d, weight, kmax):
    """S_k for k = 0..kmax by walking: every cell adds its weight to the cells 1, 2, ... hops below it; S_k is the state after 2^k - 1
    hops.  No ring."""
    down = tb.np_down(d).ravel()
    w = np.ones(d.size, U64) if weight is None else weight.ravel().astype(U64)
    acc, at, live = w.copy(), np.arange(d.size), np.ones(d.size, bool)
    out, h = [acc.copy()], 0
    for k in range(1, kmax + 1):
        while h < 2 ** k - 1 and live.any():
            nxt = down[at]
            live = live & (nxt >= 0)
            at = np.where(live, nxt, at)
            np.add.at(acc, at[live], w[live])
            h += 1
        out.append(acc.copy())
    return out


# ---------------------------------------------------------------------------------------------------------------- cases
def weights(ni, nj, seed=0):
    return np.random.default_rng(4000 + 31 * ni + nj + seed).integers(0, 2 ** 32, (nj, ni), dtype=np.uint64).astype(U32)


def inflows(ni, nj):
    return np.random.default_rng(5000 + 31 * ni + nj).integers(0, 2 ** 40, (nj, ni), dtype=np.uint64)


def tributary_cycle():
    """Caller-made: a 2 x 2 cycle (1,1) -> (2,1) -> (2,2) -> (1,2) -> (1,1) in a 6 x 4 window; row 0 drains east into nothing, and a
    tributary (5,1) -> (4,1) -> (3,1) -> (2,1) joins the cycle; (0, 3) -> (1, 3) -> (1, 2) another."""
    d = np.zeros((4, 6), np.uint8)
    d[1, 1], d[1, 2], d[2, 2], d[2, 1] = 1, 3, 5, 7
    d[1, 5], d[1, 4], d[1, 3] = 5, 5, 5
    d[3, 0], d[3, 1] = 1, 7
    d[0, :5] = 1
    return d


def inward(ni, nj):
    """Every cell drains towards the centre cell, which has no direction: acyclic, and every ring cell but the corners' neighbours pushes
    into the tile."""
    jj, ii = np.meshgrid(np.arange(nj), np.arange(ni), indexing="ij")
    di, dj = np.sign(ni // 2 - ii), np.sign(nj // 2 - jj)
    d = np.zeros((nj, ni), np.uint8)
    for k in range(1, 9):
        d[(di == trt.DI[k - 1]) & (dj == trt.DJ[k - 1])] = k
    return d


def ring_planes(ni, nj):
    """The direction planes of the ring tests: a filled terrain (its edges drain outwards) and the plane that drains inwards."""
    return (("filled", dir_cases(ni, nj)[0][1]), ("inward", inward(ni, nj)))


@functools.lru_cache(maxsize=None)
def dir_cases(ni, nj):
    """((name, dir, acyclic)): the directions of every filled terrain of test_flow_fill's generators, and caller-given ones: random bytes
    (values above 8, cycles) and hand-made cycles."""
    out = []
    for name, d, flags, acyclic in tb.dir_cases(ni, nj):
        if flags == 0 and (name.startswith("filled ") or not acyclic):
            out.append((name, d, acyclic))
    assert sum(a for _, _, a in out) >= 2 and sum(not a for _, _, a in out) == 2
    return tuple(out)


@functools.lru_cache(maxsize=None)
def combo(ni, nj, ci, weighted):
    name, d, acyclic = dir_cases(ni, nj)[ci]
    w = weights(ni, nj) if weighted else None
    if w is not None:
        w.setflags(write=False)
    return "%dx%d %s, %s" % (ni, nj, name, "random weights" if weighted else "unit weights"), d, w, acyclic, Restated(d, w)


def combos(ni, nj):
    for ci in range(len(dir_cases(ni, nj))):
        for weighted in (False, True):
            yield combo(ni, nj, ci, weighted)


# ---------------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("ni, nj", SHAPES)
def test_restatement_equals_the_sequential_accumulation(ni, nj):
    """The final sums of init + passes equal the topological accumulation in every word wherever the cell is not on a cycle; an acyclic
    network converges in exactly bit_length(L) + 1 passes, leaves both pend planes 0 and every jump -1; after EVERY pass k,
    sum + pend_out == S_k, the sum over the cells fewer than 2^k hops up; a network with a cycle still pushes at the cap."""
    for what, d, w, acyclic, rs in combos(ni, nj):
        want, done, L = sequential(d, w)
        assert done.all() or not acyclic, what
        assert_words(rs.sum[done.ravel()], want.ravel()[done.ravel()], what + ": sums off the cycles")
        if done.all():
            assert rs.converged and rs.passes == passes_of(L), (what, rs.passes, L)
            s, p0, p1, j0, j1 = rs.states[-1]
            assert not p0.any() and not p1.any() and (rs.states[-1][3 + rs.out[-1]] == -1).all(), what
            sk = partial_sums(d, w, rs.passes)
            for k in range(rs.passes + 1):
                st = rs.states[k]
                with np.errstate(over="ignore"):
                    got = st[0] + (st[1 + rs.out[k]] if k else 0)
                assert_words(got, sk[k], "%s: sum + pend_out after pass %d" % (what, k))
            assert_words(sk[-1], want.ravel(), what + ": S_k at the last pass")
        else:
            assert not rs.converged and rs.passes == rs.cap and rs.flags[-1] == 1, what
        assert rs.passes <= rs.cap


def test_pass_counts():
    """bit_length(L) + 1: a row of n cells draining west has L = n - 1."""
    for n, want in ((1, 1), (2, 2), (3, 3), (4, 3), (5, 4), (8, 4), (9, 5), (4096, 13)):
        rs = Restated(np.full((1, n), 5, np.uint8))
        assert rs.converged and rs.passes == want == passes_of(n - 1) <= rs.cap, (n, rs.passes)
        assert_words(rs.sum, np.arange(n, 0, -1).astype(U64), "row of %d" % n)
    rs = Restated(np.zeros((3, 3), np.uint8))
    assert rs.passes == 1 and rs.flags == [0]


def test_the_cycle_with_a_tributary():
    """The 2 x 2 caller-made cycle: still pushing at the cap; the tributary cells and the cells apart from it are exact."""
    d = tributary_cycle()
    w = weights(6, 4)
    rs = Restated(d, w)
    want, done, L = sequential(d, w)
    assert not rs.converged and rs.passes == rs.cap == 6 and rs.flags == [1] * 6
    on = np.zeros(d.shape, bool)
    on[1:3, 1:3] = True
    assert (done == ~on).all()
    assert_words(rs.sum[done.ravel()], want.ravel()[done.ravel()], "cells off the cycle")
    assert int(want[1, 3]) == int(w[1, 3]) + int(w[1, 4]) + int(w[1, 5]) and int(want[3, 1]) == int(w[3, 0]) + int(w[3, 1])


def test_rings_cut_the_edges_into_them():
    """A ring cell keeps its inflow, is pushed to by nobody and still pushes into the tile; restatement against the sequential method."""
    ni, nj = 67, 35
    w, q = weights(ni, nj), inflows(ni, nj)
    for name, d in ring_planes(ni, nj):
        for flags in (RING["w"], RING["e"], RING["s"], RING["n"], 0xF0):
            rs = Restated(d, w, q, flags)
            want, done, L = sequential(d, w, q, flags)
            ring = ring_mask(d.shape, flags)
            assert done.all() and rs.converged and rs.passes == passes_of(L)
            assert_words(rs.sum, want.ravel(), "%s, flags %d" % (name, flags))
            assert_words(rs.sum[ring.ravel()], q.ravel()[ring.ravel()], "ring cells keep their inflow")
            if name == "inward":
                assert (rs.sum[~ring.ravel()] != Restated(d, w, None, flags).sum[~ring.ravel()]).any(), "no ring cell pushes into the tile"
                assert int(rs.sum[(nj // 2) * ni + ni // 2]) == (int(w[~ring].astype(U64).sum()) + int(q[ring].sum())) & MASK


def build():
    """The host checker: nmp_dev_accum.hpp compiled for the CPU.  Needs nothing of the engine library."""
    deps = [SRC, HEADER] + [os.path.join(CSRC, h) for h in ("nmp_dev_accum.hpp", "nmp_dev_basins.hpp", "nmp_dev_flow_fill.hpp", "nmp_dev_routing.hpp")]
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
    lib.upstream_init_cells.argtypes = [I, I, V, V, V, V, V, V, V, I]
    lib.upstream_init_cells.restype = None
    lib.upstream_pass_cells.argtypes = [I, I, V, V, V, V, V, I]
    lib.upstream_pass_cells.restype = I
    return lib


_p = trt._p


def host_init(d, weight, inflow, flags):
    nj, ni = d.shape
    n = d.size
    d = np.ascontiguousarray(d, np.uint8)
    s, p0, p1, j0 = [np.full(n, STATE_POISON, U64) for _ in range(3)] + [np.full(n, WORD_POISON, I32)]
    _host().upstream_init_cells(ni, nj, _p(d), _p(np.ascontiguousarray(weight, U32)) if weight is not None else None,
                                _p(np.ascontiguousarray(inflow, U64)) if inflow is not None else None, _p(s), _p(p0), _p(p1), _p(j0), flags)
    return s, p0, p1, j0, np.full(n, WORD_POISON, I32)


def host_pass(shape, state, cur, reverse):
    """One pass on copies of the five planes, pend[cur] / jump[cur] the old ones: (the five planes, changed)."""
    nj, ni = shape
    st = [np.array(a) for a in state]
    flag = _host().upstream_pass_cells(ni, nj, _p(st[0]), _p(st[1 + cur]), _p(st[2 - cur]), _p(st[3 + cur]), _p(st[4 - cur]), reverse)
    return st, flag


def check_host(what, d, rs, weight, inflow, flags):
    for got, want, nm in zip(host_init(d, weight, inflow, flags), rs.states[0], NAMES):
        assert_words(got, want, "%s: %s of init" % (what, nm))
    for k in range(rs.passes):
        cur = 1 - rs.out[k + 1]
        for reverse in (0, 1):
            got, flag = host_pass(d.shape, rs.states[k], cur, reverse)
            for g, want, nm in zip(got, rs.states[k + 1], NAMES):
                assert_words(g, want, "%s: %s after pass %d, %s order" % (what, nm, k + 1, "descending" if reverse else "ascending"))
            assert flag == rs.flags[k], (what, k)


@pytest.mark.parametrize("ni, nj", SHAPES)
def test_host_compilation_equals_the_restatement(ni, nj):
    """nmp_dev_accum.hpp compiled for the host, the atomic a plain add: init and EVERY pass with its flag, the cells visited in ascending
    and in descending order, equal the restatement in every word of every plane; with rings and inflow too."""
    for what, d, w, acyclic, rs in combos(ni, nj):
        check_host(what, d, rs, w, None, 0)
    w, q = weights(ni, nj, 1), inflows(ni, nj)
    for name, d in ring_planes(ni, nj):
        for flags in (RING["w"] | RING["n"], 0xF0):
            check_host("%dx%d %s, ring %d" % (ni, nj, name, flags), d, Restated(d, w, q, flags), w, q, flags)


def test_a_jump_nobody_initialised_is_never_followed():
    """Jumps outside 0 .. ni*nj-1 push nothing and become -1, restated and compiled; a valid jump copies its target's word as it is."""
    jump = np.array([1, 7, -4, 2 ** 31 - 1, -2 ** 31, 6, -1], I32)
    state = (np.arange(1, 8).astype(U64), np.full(7, 10, U64), np.zeros(7, U64), jump, np.full(7, WORD_POISON, I32))
    s, pin, pout, jn, flag = np_up_pass(state[0], state[1], state[2], jump)
    got, gflag = host_pass((1, 7), state, 0, 0)
    for g, want, nm in zip(got, (s, pin, pout, jump, jn), NAMES):
        assert_words(g, want, nm)
    assert jn.tolist() == [7, -1, -1, -1, -1, -1, -1] and pout.tolist() == [0, 11, 0, 0, 0, 0, 16] and flag == gflag == 1


# ---------------------------------------------------------------------------------------------------------------- refusals and bindings
PLANES = ("dir", "weight", "inflow", "sum", "pend_in", "pend_out", "jump_old", "jump_new", "changed")
CALLS = ("noahmp_hip_flow_upstream_init", "noahmp_hip_flow_upstream_pass")
REQUIRED = dict(noahmp_hip_flow_upstream_init=("dir", "sum", "pend_in", "pend_out", "jump_old"),
                noahmp_hip_flow_upstream_pass=("sum", "pend_in", "pend_out", "jump_old", "jump_new", "changed"))
FIELDS = list(PLANES) + ["ni", "nj", "flags"]


def _up_block(ptrs, ni=5, nj=3, **kw):
    b = abi.FlowUpstream()
    for k in PLANES:
        setattr(b, k, ptrs[k])
    b.ni, b.nj, b.flags = ni, nj, 0
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
            out.append(("%s.required.%s" % (short, field), fn, _up_block(ptrs, **{field: None})))
        for field in ("sum", "pend_in", "pend_out"):
            out.append(("%s.misaligned.%s" % (short, field), fn, _up_block(ptrs, **{field: ptrs[field] + 4})))
        for nm, kw in (("ni", dict(ni=-1)), ("nj", dict(nj=-1)), ("big", dict(ni=65536, nj=32768))):
            out.append(("%s.window.%s" % (short, nm), fn, _up_block(ptrs, **kw)))
        for nm, fl in (("low", 1), ("outlet", 15 | 16), ("high", 256), ("all", -1)):
            out.append(("%s.flags.%s" % (short, nm), fn, _up_block(ptrs, flags=fl)))
        out.append((short + ".same.pend", fn, _up_block(ptrs, pend_out=ptrs["pend_in"])))
        out.append((short + ".overlap.pend", fn, _up_block(ptrs, pend_out=ptrs["pend_in"] + 8 * 14)))
        out.append((short + ".sum.pend_in", fn, _up_block(ptrs, sum=ptrs["pend_in"])))
        out.append((short + ".sum.pend_out", fn, _up_block(ptrs, pend_out=ptrs["sum"])))
        out.append((short + ".sum.overlap", fn, _up_block(ptrs, sum=ptrs["pend_out"] + 8)))
    out.append(("init.misaligned.inflow", CALLS[0], _up_block(ptrs, inflow=ptrs["inflow"] + 4)))
    out.append(("pass.same.jump", CALLS[1], _up_block(ptrs, jump_new=ptrs["jump_old"])))
    out.append(("pass.overlap.jump", CALLS[1], _up_block(ptrs, jump_new=ptrs["jump_old"] + 4 * 14)))
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
    """Every refusal site of the two calls gives -105 and its full text (tests/golden/upstream_refusal_text.json) before anything is
    launched or read: the planes here are host memory that the calls must not touch, and they keep their poison.  Among them a NULL
    block, every required plane, a misaligned 8-byte plane, both jump planes the same, both pend planes the same, sum on a pend plane."""
    lib = abi.load_library()
    planes = {k: np.full(32, WORD_POISON, np.int64) for k in PLANES}
    _refusals(lib, {k: v.ctypes.data for k, v in planes.items()})
    assert all((p == WORD_POISON).all() for p in planes.values())
    text = json.load(open(REFUSAL_FIXTURE))
    assert len({tuple(v) for v in text.values()}) == 2 * 7 + 1, "the distinct texts: seven per call and the pass's jump planes"
    assert "weight" not in "".join(REQUIRED[CALLS[0]]) and text["pass.same.jump"][1] != text["pass.same.pend"][1]


HEADER_LINES = (
    "#define NOAHMP_HIP_HAS_FLOW_UPSTREAM 1\n", "#define NOAHMP_HIP_ABI_MINOR 3\n", "typedef struct noahmp_flow_upstream {", "} noahmp_flow_upstream;",
    "jump_old[c] = t when t exists and is not RING; otherwise -1", "sum[c]      = RING ? (inflow ? inflow[c] : 0) : (weight ? weight[c] : 1)",
    "pend_in[c]  = pend_out[c] = 0", "s = sum[c] + pend_in[c];  sum[c] = s;  pend_in[c] = 0;  j = jump_old[c];",
    "j in 0 .. ni*nj-1 :  atomic pend_out[j] += s;  jump_new[c] = jump_old[j];  *changed = 1   (a plain store)",
    "otherwise         :  jump_new[c] = -1", "sum + pend_out == S_k in every word", "bit_length(L) + 1 passes", "ceil(log2(ni*nj)) + 1 passes are THE CAP",
    "THE DEFERRED FOLD", "an edge INTO a ring cell is cut", "is never followed", "A legal sum is below 2^63", "(the largest k) + 2 rounds",
) + tuple("int    %s(const noahmp_flow_upstream* u, void* stream);" % c for c in CALLS) + tuple("#define NOAHMP_UPSTREAM_RING_%s " % s for s in "WESN")


def test_bindings_carry_the_upstream_calls():
    from tools import gen_abi
    for rel, text in (("include/noahmp_hip.h", gen_abi.c_header()), ("noahmp_amd/fortran/module_sf_noahmpdrv_hip.F90", gen_abi.fortran_shim())):
        assert open(os.path.join(ROOT, rel)).read() == text, rel
    hdr = open(HEADER).read()
    for word in HEADER_LINES:
        assert word in hdr, word
    assert "\n".join(gen_abi.flow_upstream_header()) in hdr
    assert "noahmp_flow_upstream" not in gen_abi.ref_harness() and "noahmp_flow_upstream" not in gen_abi.shim_wrap()
    f90 = open(os.path.join(ROOT, "noahmp_amd", "fortran", "module_sf_noahmpdrv_hip.F90")).read()
    for word in tuple("bind(C, name='%s')" % c for c in CALLS) + ("type, bind(C) :: noahmp_flow_upstream ", "NOAHMP_UPSTREAM_RING_N = 128"):
        assert word in f90, word
    for sym in CALLS:
        assert sym in abi.EXPORTED_SYMBOLS
    assert [n for n, _ in abi.FlowUpstream._fields_] == FIELDS
    assert abi.UPSTREAM_FLAG == abi.BASIN_FLAG == {"ring_" + s: v for s, v in RING.items()}
    src = open(os.path.join(CSRC, "noahmp_accum.hip")).read() + open(os.path.join(CSRC, "nmp_dev_accum.hpp")).read()
    assert "__hip_atomic_fetch_add((unsigned long long*)" in src and "__ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT" in src
    assert "__shared__" not in src and "atomicAdd" not in src


def test_ctypes_mirror_matches_the_compiled_header(tmp_path):
    names = [n for n, _ in abi.FlowUpstream._fields_]
    body = 'printf(" %zu", sizeof(noahmp_flow_upstream));' + "".join('printf(" %%zu", offsetof(noahmp_flow_upstream, %s));' % n for n in names)
    want = [C.sizeof(abi.FlowUpstream)] + [getattr(abi.FlowUpstream, n).offset for n in names]
    macros = ["NOAHMP_HIP_ABI_MINOR", "NOAHMP_HIP_HAS_FLOW_UPSTREAM"] + ["NOAHMP_UPSTREAM_RING_%s" % s for s in "WESN"] + [
        "NOAHMP_UPSTREAM_RING_W == NOAHMP_BASIN_RING_W && NOAHMP_UPSTREAM_RING_E == NOAHMP_BASIN_RING_E && NOAHMP_UPSTREAM_RING_S == NOAHMP_BASIN_RING_S"]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "noahmp_hip.h"\nint main(){' + body +
                   "".join('printf(" %%d", %s);' % m for m in macros) + " return 0;}")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert out == want + [3, 1] + [RING[s] for s in "wesn"] + [1]


def test_library_exports_the_upstream_calls():
    if not os.path.exists(abi.LIB_PATH):
        from noahmp_amd import build as b
        b.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", abi.LIB_PATH]).decode()
    for sym in CALLS:
        assert " T %s\n" % sym in out, sym


@pytest.mark.skipif(tr._flang() is None, reason="no flang")
def test_generated_fortran_type_and_interfaces_compile(tmp_path):
    """The upstream part of the generated module compiles, and a caller of the two interfaces type-checks."""
    from tools import gen_abi
    text = "\n".join(["module flow_upstream_abi_check", "  use iso_c_binding", "  implicit none"] + gen_abi.flow_upstream_f90_types() + ["  interface"] +
                     gen_abi.flow_upstream_f90_interfaces() +
                     ["  end interface", "contains", "  function go(planes) result(rc)", "    type(c_ptr), intent(in) :: planes(9)",
                      "    type(noahmp_flow_upstream) :: u", "    integer(c_int) :: rc",
                      "    u%dir = planes(1); u%weight = c_null_ptr; u%inflow = planes(3); u%sum = planes(4); u%pend_in = planes(5)",
                      "    u%pend_out = planes(6); u%jump_old = planes(7); u%jump_new = planes(8); u%changed = planes(9); u%ni = 64; u%nj = 8",
                      "    u%flags = ior(NOAHMP_UPSTREAM_RING_W, NOAHMP_UPSTREAM_RING_N)",
                      "    rc = noahmp_hip_flow_upstream_init(u, c_null_ptr)", "    rc = noahmp_hip_flow_upstream_pass(u, c_null_ptr)",
                      "    if (NOAHMP_UPSTREAM_RING_E /= 32) rc = -1",
                      "  end function go", "end module flow_upstream_abi_check", ""])
    f = tmp_path / "flow_upstream_abi_check.f90"
    f.write_text(text)
    subprocess.check_call([tr._flang(), "-c", str(f), "-o", str(tmp_path / "flow_upstream_abi_check.o"), "-J", str(tmp_path)], cwd=str(tmp_path))


def test_quantise_and_mean_of():
    """round(field / step) as uint32 words, ties to even; NaN, negative values and values above 2^32 - 1 raise; mean_of divides in
    float64 and gives NaN where the weight sum is 0."""
    import torch
    from noahmp_amd.routing import Upstream
    q = Upstream.quantise(np.array([[0.0, 0.49, 0.5, 1.5, 2.5, 1e6, (2.0 ** 32 - 1) * 0.25]]), 0.25)
    assert q.dtype == U32 and q.tolist() == [[0, 2, 2, 6, 10, 4000000, 2 ** 32 - 1]]
    t = Upstream.quantise(torch.tensor([3.0e9, 7.0]), 1.0)
    assert t.dtype == torch.int32 and t.numpy().view(U32).tolist() == [3000000000, 7]
    for bad, word in ((np.array([1.0, np.nan]), "NaN"), (np.array([-0.6, 1.0]), "negative"), (np.array([2.0 ** 32]), "above"), (np.array([np.inf]), "above")):
        with pytest.raises(ValueError, match=word):
            Upstream.quantise(bad, 1.0)
    assert Upstream.quantise(np.array([-0.4]), 1.0).tolist() == [0]
    m = Upstream.mean_of(torch.tensor([6, 0, 2 ** 53 + 2], dtype=torch.int64), torch.tensor([4, 0, 2], dtype=torch.int64))
    assert m.dtype == torch.float64 and m[0].item() == 1.5 and np.isnan(m[1].item()) and m[2].item() == 2.0 ** 52 + 1


# ---------------------------------------------------------------------------------------------------------------- GPU
_dev = tr._dev


class _Gpu:
    """The device planes of one case at odd offsets inside poisoned pools, and the calls on them one by one."""

    def __init__(self, engine, d, weight=None, inflow=None, flags=0):
        import torch
        self.engine, self.torch = engine, torch
        nj, ni = d.shape
        self.shape, self.n = (nj, ni), ni * nj
        self.spool, (s, p0, p1, q) = trt._pool(self.n, 4, torch.int64, STATE_POISON)
        self.wpool, (j0, j1, w) = trt._pool(self.n, 3, torch.int32, WORD_POISON)
        self.bpool, (dr,) = trt._pool(self.n, 1, torch.uint8, 0xEE)
        self.ipool, (ch,) = trt._pool(1, 1, torch.int32, 77)
        v = lambda t: t.view(nj, ni)                                      # noqa: E731
        self.sum, self.pend, self.jump, self.changed, self.cur = v(s), [v(p0), v(p1)], [v(j0), v(j1)], ch, 0
        self.dir = v(dr)
        self.dir.copy_(_dev(np.ascontiguousarray(d)))
        self.weight = self.inflow = None
        if weight is not None:
            self.weight = v(w)
            self.weight.copy_(_dev(np.ascontiguousarray(weight, U32).view(I32)))
        if inflow is not None:
            self.inflow = v(q)
            self.inflow.copy_(_dev(np.ascontiguousarray(inflow, U64).view(np.int64)))
        self.flags = int(flags)
        torch.cuda.synchronize()

    def block(self):
        c = self.cur
        return self.engine.flow_upstream_block(self.dir, self.sum, self.pend[c], self.pend[1 - c], self.jump[c], self.jump[1 - c], self.changed,
                                               flags=self.flags, weight=self.weight, inflow=self.inflow)

    def planes(self):
        u = lambda t: t.cpu().numpy().ravel().view(U64)                   # noqa: E731
        return u(self.sum), u(self.pend[0]), u(self.pend[1]), self.jump[0].cpu().numpy().ravel(), self.jump[1].cpu().numpy().ravel()

    def init(self):
        self.engine.flow_upstream_init(self.block())
        self.engine.stream_sync()
        return self.planes()

    def step(self):
        self.changed.zero_()
        self.torch.cuda.synchronize()
        self.engine.flow_upstream_pass(self.block())
        self.engine.stream_sync()
        self.cur = 1 - self.cur
        return self.planes(), int(self.changed.item())

    def guards_ok(self):
        ok = trt._guards_ok(self.spool, self.n, STATE_POISON) and trt._guards_ok(self.wpool, self.n, WORD_POISON)
        ok = ok and trt._guards_ok(self.bpool, self.n, 0xEE) and trt._guards_ok(self.ipool, 1, 77)
        if self.inflow is None:
            ok = ok and bool((self.spool[3] == STATE_POISON).all().item())
        if self.weight is None:
            ok = ok and bool((self.wpool[2] == WORD_POISON).all().item())
        return ok


def check_gpu(engine, what, d, rs, weight=None, inflow=None, flags=0):
    """Every plane after init and after EVERY pass, and every flag, against the restatement; dir is not written; guards keep the poison."""
    g = _Gpu(engine, d, weight, inflow, flags)
    for got, want, nm in zip(g.init(), rs.states[0], NAMES):
        assert_words(got, want, "%s: %s of init" % (what, nm))
    for k in range(rs.passes):
        got, flag = g.step()
        for a, want, nm in zip(got, rs.states[k + 1], NAMES):
            assert_words(a, want, "%s: %s after pass %d" % (what, nm, k + 1))
        assert flag == rs.flags[k], (what, k)
    trt.assert_same_bytes(g.dir.cpu().numpy(), d, what + ": dir")
    assert g.guards_ok(), what
    return g


@pytest.mark.gpu
@pytest.mark.parametrize("ni, nj", SHAPES)
def test_gpu_calls_equal_the_restatement(engine, ni, nj):
    """Filled terrain and caller-given directions (random bytes, hand-made cycles: those run to the cap), unit and random weights: the
    planes are poisoned before init, and every plane is compared after init and after every pass."""
    for what, d, w, acyclic, rs in combos(ni, nj):
        check_gpu(engine, what, d, rs, w)


@pytest.mark.gpu
def test_gpu_weights_that_carry_into_the_high_word(engine):
    """All weights 0xFFFFFFFF on 67 x 35: the sums pass 2^32, and equal the sequential accumulation."""
    ni, nj = 67, 35
    d = dir_cases(ni, nj)[0][1]
    w = np.full((nj, ni), 0xFFFFFFFF, U32)
    rs = Restated(d, w)
    g = check_gpu(engine, "all weights 2^32 - 1", d, rs, w)
    want, done, L = sequential(d, w)
    assert_words(g.planes()[0], want.ravel(), "sums")
    assert int(want.max()) > 2 ** 33 and rs.passes == passes_of(L)


@pytest.mark.gpu
def test_gpu_rings_with_inflow(engine):
    """A ring on each side and on all four, with a random inflow, against the restatement in every plane after every pass."""
    ni, nj = 67, 35
    w, q = weights(ni, nj), inflows(ni, nj)
    for name, d in ring_planes(ni, nj):
        for flags in (RING["w"], RING["e"], RING["s"], RING["n"], 0xF0):
            check_gpu(engine, "%s, ring %d" % (name, flags), d, Restated(d, w, q, flags), w, q, flags)
        check_gpu(engine, name + ", ring everywhere, no inflow plane", d, Restated(d, None, None, 0xF0), None, None, 0xF0)


def _upstream(engine, d, weight=None):
    from noahmp_amd.routing import Upstream
    u = Upstream(tb._net(engine, d))
    u.set_weight(weight)
    return u


@pytest.mark.gpu
def test_gpu_long_row_and_funnel(engine):
    """One row of 4096 cells draining west: L = 4095, 13 passes, whatever the batch size.  A 64 x 64 funnel -- every row drains west,
    column 0 drains south -- where one cell takes thousands of adds per pass: the sequential sums, and two runs give identical words."""
    d = np.full((1, 4096), 5, np.uint8)
    for check in (1, 4, 32):
        u = _upstream(engine, d)
        s = u.run(check=check)
        assert u.passes == 13 == passes_of(4095) and u.converged and u.rounds == 1 and u.cap == 13
        assert_words(s.cpu().numpy().view(U64), np.arange(4096, 0, -1).astype(U64).reshape(1, 4096), "the row")
    d = np.full((64, 64), 5, np.uint8)
    d[:, 0] = 7
    d[0, 0] = 0
    w = weights(64, 64)
    want, done, L = sequential(d, w)
    assert L == 126 and int(want[0, 0]) == int(w.astype(U64).sum())
    check_gpu(engine, "funnel", d, Restated(d, w), w)
    runs = []
    for _ in range(2):
        u = _upstream(engine, d, w)
        runs.append(u.run().cpu().numpy().view(U64).copy())
        assert u.passes == passes_of(L) == 8
    assert_words(runs[0], want, "funnel")
    assert_words(runs[1], runs[0], "funnel, second run")


@pytest.mark.gpu
def test_gpu_unit_weights_equal_upstream_cells(engine):
    """Upstream.cells() equals FlowNetwork.upstream_cells() on the same network in every word, in a logarithmic number of passes; the
    channel mask is the threshold on it."""
    ni, nj = 67, 35
    for ci in range(2):
        name, d, acyclic = dir_cases(ni, nj)[ci]
        assert acyclic
        net = tb._net(engine, d)
        acc = net.upstream_cells().cpu().numpy().view(U32)
        from noahmp_amd.routing import Upstream
        u = Upstream(net)
        s = u.cells().cpu().numpy()
        assert s.dtype == np.int64 and u.sum is not None
        assert_words(s, acc.astype(np.int64), name)
        assert u.passes == passes_of(sequential(d)[2]) < net.passes
        thr = int(np.median(acc)) + 1
        assert_words(u.channel_mask(thr).cpu().numpy(), acc >= thr, name + ": channel mask")


@pytest.mark.gpu
def test_gpu_cycle_with_a_tributary(engine):
    """The 2 x 2 caller-made cycle: changed is still set at the cap, every word equals the restatement, the tributary cells equal the
    sequential sums; strict=True raises, strict=False leaves converged False."""
    d, w = tributary_cycle(), weights(6, 4)
    rs = Restated(d, w)
    assert rs.passes == rs.cap and rs.flags[-1] == 1
    g = check_gpu(engine, "cycle", d, rs, w)
    want, done, L = sequential(d, w)
    assert_words(g.planes()[0][done.ravel()], want.ravel()[done.ravel()], "cells off the cycle")
    u = _upstream(engine, d, w)
    with pytest.raises(RuntimeError, match="still push after the cap of 6 passes"):
        u.run()
    s = u.run(strict=False)
    assert not u.converged and u.passes == u.cap == 6
    assert_words(s.cpu().numpy().view(U64).ravel(), rs.sum, "run(strict=False)")


class _RingFromWhole:
    """A stand-in for Comm in one process: exchange_halo copies the ring of the two word planes (float32 views of int32 words) from the
    whole-domain sums, ENQUEUED ONLY on torch's current stream; agree_any returns its argument."""

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


def _words(t):
    """int64 plane -> (low, high) int32 planes."""
    import torch
    v = t.contiguous().view(torch.int32).view(t.shape + (2,))
    return v[..., 0].contiguous(), v[..., 1].contiguous()


@pytest.mark.gpu
def test_gpu_decomposition(engine):
    """A 50 x 36 filled terrain with random weights cut 2 x 2: four Upstream objects on one GPU, the test doing the exchange by slicing,
    in lockstep.  Every part equals the undecomposed run on its tile within (the largest number of ownership changes along a flow
    path) + 2 rounds; then Upstream.run(comm=stand-in) per part on a side stream equals it on the whole block, ring included."""
    import torch
    from noahmp_amd.routing import Upstream
    ni, nj = 50, 36
    name, d, acyclic = dir_cases(ni, nj)[0]
    w = weights(ni, nj)
    whole = _upstream(engine, d, w).run().clone()
    want, done, L = sequential(d, w)
    assert_words(whole.cpu().numpy().view(U64), want, "the undecomposed run")
    wl, wd, wh = tb.walk(d, None, 0)
    parts, part_of = [], np.zeros(d.shape, np.int64)
    for n, (tile, blk, bidx) in enumerate(tsh._cuts(ni, nj, 1)):
        part_of[tile] = n
        own = (slice(tile[0].start - blk[0].start, tile[0].stop - blk[0].start), slice(tile[1].start - blk[1].start, tile[1].stop - blk[1].start))
        net = tb._net(engine, d[blk], tile=(tile[1].stop - tile[1].start, tile[0].stop - tile[0].start), origin=(own[1].start, own[0].start))
        u = Upstream(net)
        u.set_weight(np.ascontiguousarray(w[blk]))
        assert sorted(u.ring_sides()) == sorted(tff._ring_sides(tile, blk)) and len(u.ring_sides()) == 2
        with pytest.raises(ValueError, match="comm"):
            u.run()
        u.begin()                                                         # round 0: inflow is 0
        assert u.accumulate() and u.passes <= u.cap
        parts.append((u, tile, blk, own, _dev(bidx < 0)))
    bound = tb._ownership_changes(d, part_of, wh) + 2
    assert bound >= 3, "no path crosses a cut"
    G = torch.zeros((nj, ni), dtype=torch.int64, device="cuda")
    rounds = 1
    while True:
        for u, tile, blk, own, ring in parts:
            G[tile] = u.sum[own]
        moved = []
        for u, tile, blk, own, ring in parts:                             # the exchange: the ring from the owners, low and high words
            for p, g in zip(u.halo_planes(), _words(G[blk])):
                v = p.view(torch.int32)
                v.copy_(torch.where(ring, g, v))
            torch.cuda.synchronize()
            moved.append(u.absorb_ring())
            if moved[-1]:
                u.begin()
                assert u.accumulate()
        rounds += 1
        if not any(moved):
            break
        assert rounds < bound, "%s: more rounds than ownership changes + 2 = %d" % (name, bound)
    assert 3 <= rounds <= bound, (rounds, bound)
    for u, tile, blk, own, ring in parts:
        assert_words(u.sum[own].cpu().numpy(), whole[tile].cpu().numpy(), "part %s after %d rounds" % (tile, rounds))
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    for u0, tile, blk, own, ring in parts:
        comm = _RingFromWhole(_words(whole), blk, ring)
        u = Upstream(u0.net)
        u.set_weight(np.ascontiguousarray(w[blk]))
        with torch.cuda.stream(side):
            u.run(comm=comm, geom="geom")
        engine.stream_sync()
        torch.cuda.synchronize()
        assert comm.calls == u.rounds - 1 and 2 <= u.rounds <= 3 and u.converged
        assert_words(u.sum.cpu().numpy(), whole[blk].cpu().numpy(), "run(comm) of part %s, ring included" % (tile,))
        with pytest.raises(RuntimeError, match="after 1 rounds"):
            u.run(comm=comm, geom="geom", max_rounds=1)


@pytest.mark.gpu
def test_gpu_refusals_launch_nothing(engine):
    """The refusals with device planes -- a misaligned plane and each aliasing among them: -105, the full text, and every plane keeps its
    poison; an empty window is no refusal and writes nothing."""
    import torch
    pl = torch.full((len(PLANES), 32), WORD_POISON, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ptrs = {k: pl[n].data_ptr() for n, k in enumerate(PLANES)}
    _refusals(engine.lib, ptrs)
    for kw in (dict(nj=0), dict(ni=0), dict(ni=0, nj=0)):
        b = _up_block(ptrs, **kw)
        for fn in CALLS:
            assert getattr(engine.lib, fn)(C.byref(b), None) == 0
    engine.stream_sync()
    torch.cuda.synchronize()
    assert (pl.cpu().numpy() == WORD_POISON).all()


if __name__ == "__main__":                                                # PYTHONPATH=.:tests python tests/test_upstream.py records the refusal texts
    lib = abi.load_library()
    planes = {k: np.full(32, WORD_POISON, np.int64) for k in PLANES}
    out = {}
    for site, fn, block in refusal_probes({k: v.ctypes.data for k, v in planes.items()}):
        rc = getattr(lib, fn)(C.byref(block) if block is not None else None, None)
        out[site] = [rc, lib.noahmp_hip_last_error().decode()]
    json.dump(out, open(REFUSAL_FIXTURE, "w"), indent=1, sort_keys=True)
    print("%s: %d sites" % (REFUSAL_FIXTURE, len(out)))
