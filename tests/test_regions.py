"""Region series: per-step weighted sums, minima and maxima of fields of the step block over labelled regions (noahmp_hip_region_plan /
_plan_follow / _step, noahmp_amd/csrc/noahmp_regions.hip, noahmp_amd/history.py::Regions).

The contract: region r has the members L_r = cells with region == r in ascending TILE index; a SUM entry's
term is the float64 (double)w * (double)x of a cell that takes part, else +0.0; the terms are summed by S -- chunks of 256 consecutive
terms, each folded as a binary tree (h = 128 .. 1: v[i] += v[i+h]), then S of the partials.  MIN / MAX: float32 minimum / maximum with
the comparisons of hist_apply (a NaN sample never wins; identity +-HUGE).  The result is a function of the tile-order values alone.

Every comparison is exact: values equal as float64 numbers or both NaN (the sign of a zero is not part of the contract).  CPU: the
restatement against the exact sum; nmp_dev_regions.hpp compiled for the host (tests/host_emul/regions_check.hip, built on demand)
against numpy; the generated bindings; the Fortran driver's build.  GPU: the kernels against the restatement."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from noahmp_amd import abi, synth
from noahmp_amd.abi import REG_OP

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "noahmp_amd", "csrc")
SRC = os.path.join(HERE, "host_emul", "regions_check.hip")
LIB = os.path.join(HERE, "host_emul", "libregions_check.so")
F, D = np.float32, np.float64
HUGE = np.finfo(np.float32).max
OPS = ("sum", "min", "max")


# ---------------------------------------------------------------------------------------------------------------- the restatement
def fold(v):                       # v: float64, len <= 256
    v = np.concatenate([v, np.zeros(256 - len(v))])
    h = 128
    while h:
        v = v[:h] + v[h:2 * h]
        h //= 2
    return v[0]


def S(t):
    """The issue's numpy restatement, word for word."""
    if len(t) == 0:
        return 0.0
    while True:
        t = np.array([fold(t[i:i + 256]) for i in range(0, len(t), 256)])
        if len(t) == 1:
            return t[0]


def S_fast(t, pad=0.0, comb=np.add):
    """The same tree on whole levels at once (the tests' working form; test_fast_restatement_is_the_restatement holds the two together).
    pad / comb: the identity and the node of MIN / MAX, whose result does not depend on the tree."""
    t = np.asarray(t, dtype=D)
    if t.size == 0:
        return D(pad)
    with np.errstate(all="ignore"):
        while True:
            nch = -(-t.size // 256)
            v = np.full(nch * 256, pad, D)
            v[:t.size] = t
            v = v.reshape(nch, 256)
            h = 128
            while h:
                v = comb(v[:, :h], v[:, h:2 * h])
                h //= 2
            t = v[:, 0]
            if t.size == 1:
                return t[0]


def np_takes_part(xland, xice, thres):
    with np.errstate(all="ignore"):
        return ~((xland - F(1.5)) >= 0) & ~(xice >= F(thres))


def np_terms(op, part, w, x):
    """float64 terms of the members of one region, in member order (nmp_dev_regions.hpp::reg_term)."""
    part, w, x = np.asarray(part, bool), np.asarray(w, F), np.asarray(x, F)
    with np.errstate(all="ignore"):
        if op == "sum":
            return np.where(part, w.astype(D) * x.astype(D), 0.0)
        if op == "min":
            return np.where(part & (x < HUGE), x, HUGE).astype(D)       # hist_apply(MIN, +HUGE, x): a NaN never replaces
        return np.where(part & (x > -HUGE), x, -HUGE).astype(D)


def np_reduce(op, t):
    if op == "sum":
        return S_fast(t)
    if t.size == 0:
        return D(HUGE if op == "min" else -HUGE)
    return t.min() if op == "min" else t.max()                         # the terms are never NaN


def np_series(region, nregion, weight, part, fields):
    """[len(fields)][nregion] float64: fields = [(tile-order float32 plane or None = 1.0, op)], region / weight / part in tile order."""
    reg = np.asarray(region).ravel()
    w = np.ones(reg.size, F) if weight is None else np.asarray(weight, F).ravel()
    part = np.asarray(part).ravel()
    order = np.argsort(reg, kind="stable")                             # members of each region in ascending tile index
    lo, hi = np.searchsorted(reg[order], np.arange(nregion)), np.searchsorted(reg[order], np.arange(nregion), side="right")
    out = np.zeros((len(fields), nregion), D)
    for f, (x, op) in enumerate(fields):
        xs = np.ones(reg.size, F) if x is None else np.asarray(x, F).ravel()
        for r in range(nregion):
            m = order[lo[r]:hi[r]]
            out[f, r] = np_reduce(op, np_terms(op, part[m], w[m], xs[m]))
    return out


def np_acc(op, acc, s):
    with np.errstate(all="ignore"):
        return acc + s if op == "sum" else (np.where(s < acc, s, acc) if op == "min" else np.where(s > acc, s, acc))


def assert_same(a, b, what):
    a, b = np.asarray(a, D), np.asarray(b, D)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    with np.errstate(all="ignore"):
        bad = ~((a == b) | (np.isnan(a) & np.isnan(b)))
    assert not bad.any(), "%s: %d of %d values differ, first at %s: %r vs %r" % (
        what, bad.sum(), bad.size, np.argwhere(bad)[0], a[tuple(np.argwhere(bad)[0])], b[tuple(np.argwhere(bad)[0])])


def nasty(r, n):
    """Random float32 values that contain NaN, +-Inf, -0.0, zeros and denormals."""
    x = (r.standard_normal(n) * 10.0 ** r.integers(-3, 4, n)).astype(F)
    special = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-40, -3e-42, HUGE, -HUGE], dtype=F)
    at = r.random(n) < 0.25
    x[at] = special[r.integers(0, len(special), int(at.sum()))]
    return x


def mixed(r, n):
    """Finite values spread over seven decades, both signs: a sum in another order differs in its last bits."""
    return (r.standard_normal(n) * 10.0 ** r.uniform(-3, 4, n)).astype(F)


# ---------------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("n", [1, 255, 256, 257, 65536, 65537])
def test_restatement_against_the_exact_sum(n):
    """S against math.fsum of the exact float64 terms.  Every term passes through at most 8 additions per level, so
    |S - exact| <= (8 * levels + 1) * 2^-53 * sum |t| (the + 1: fsum's own rounding).  This pins the restatement, not the kernel."""
    r = np.random.default_rng(n)
    t = mixed(r, n).astype(D) * mixed(r, n).astype(D)                   # products of two float32 values: exact in float64
    levels = 1 if n <= 256 else (2 if n <= 65536 else 3)
    got, exact = S(t), math.fsum(t.tolist())
    assert abs(got - exact) <= (8 * levels + 1) * 2.0 ** -53 * math.fsum(np.abs(t).tolist()), (n, got, exact)
    assert got == S_fast(t)


def test_fast_restatement_is_the_restatement():
    r = np.random.default_rng(3)
    assert S([]) == 0.0 and S_fast([]) == 0.0
    for n in (1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 65535, 65536, 65537, 70001):
        t = mixed(r, n).astype(D)
        assert S(t) == S_fast(t), n
    t = mixed(r, 5000).astype(D)                                        # the order is part of the result: the same terms shuffled sum differently
    assert any(S_fast(t) != S_fast(r.permutation(t)) for _ in range(4))


def build():
    deps = [SRC, os.path.join(CSRC, "nmp_dev_regions.hpp"), os.path.join(CSRC, "nmp_dev_history.hpp"), os.path.join(ROOT, "include", "noahmp_hip.h")]
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
    lib.regions_term.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_long]
    lib.regions_takes_part.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_long]
    lib.regions_combine.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_long]
    lib.regions_identity.argtypes = [C.c_int]
    lib.regions_identity.restype = C.c_double
    lib.regions_reduce.argtypes = [C.c_int, C.c_void_p, C.c_long]
    lib.regions_reduce.restype = C.c_double
    return lib


def test_host_compilation_equals_numpy_on_special_values():
    """nmp_dev_regions.hpp compiled for the host: the term, takes_part and the min / max compares on NaN / +-Inf / -0.0 / denormal samples
    and weights; MIN / MAX do not depend on the order of the terms."""
    lib = _host()
    r = np.random.default_rng(17)
    n = 20000
    xland = r.choice(np.array([1.0, 2.0, 1.5, 1.4999999, np.nan], dtype=F), n)
    xice = r.choice(np.array([0.0, 0.5, 0.49999997, 1.0, np.nan], dtype=F), n)
    part = np_takes_part(xland, xice, 0.5)
    out = np.zeros(n, np.uint8)
    lib.regions_takes_part(xland.ctypes.data, xice.ctypes.data, 0.5, out.ctypes.data, n)
    assert np.array_equal(out.astype(bool), part) and 0 < part.sum() < n
    w, x = nasty(r, n), nasty(r, n)
    assert np.isnan(x).any() and np.isinf(w).any() and (np.signbit(x) & (x == 0)).any() and ((w != 0) & (np.abs(w) < 1e-38)).any()
    for op in OPS:
        t = np.zeros(n, D)
        lib.regions_term(REG_OP[op], xland.ctypes.data, xice.ctypes.data, 0.5, w.ctypes.data, x.ctypes.data, t.ctypes.data, n)
        want = np_terms(op, part, w, x)
        assert_same(t, want, "term " + op)
        if op == "sum":
            assert not np.signbit(t[~part]).any()                       # a cell that takes no part: +0.0
            continue
        assert not np.isnan(t).any()
        ident = lib.regions_identity(REG_OP[op])
        assert ident == (HUGE if op == "min" else -HUGE) and lib.regions_identity(REG_OP["sum"]) == 0.0
        a, b, c = t[: n // 2].copy(), t[n // 2:].copy(), np.zeros(n // 2, D)
        lib.regions_combine(REG_OP[op], a.ctypes.data, b.ctypes.data, c.ctypes.data, n // 2)
        assert_same(c, np.minimum(a, b) if op == "min" else np.maximum(a, b), "combine " + op)
        sh = r.permutation(t)
        assert lib.regions_reduce(REG_OP[op], t.ctypes.data, n) == lib.regions_reduce(REG_OP[op], sh.ctypes.data, n) == np_reduce(op, t)
    a, b, c = nasty(r, n).astype(D) * 3.0, nasty(r, n).astype(D), np.zeros(n, D)
    lib.regions_combine(REG_OP["sum"], a.ctypes.data, b.ctypes.data, c.ctypes.data, n)
    with np.errstate(all="ignore"):
        assert_same(c, a + b, "combine sum")


def test_bindings_regenerate_identically():
    """include/noahmp_hip.h, the Fortran interfaces and oracle/ref_harness_gen.f90 are what tools/gen_abi.py makes of abi_spec.py, with the
    region series in them and the ABI version untouched."""
    from tools import gen_abi
    for rel, text in (("include/noahmp_hip.h", gen_abi.c_header()), ("oracle/ref_harness_gen.f90", gen_abi.ref_harness()),
                      ("noahmp_amd/fortran/module_sf_noahmpdrv_hip.F90", gen_abi.fortran_shim()),
                      ("tests/fortran/shim_wrap_gen.f90", gen_abi.shim_wrap())):
        assert open(os.path.join(ROOT, rel)).read() == text, rel
    hdr = open(os.path.join(ROOT, "include", "noahmp_hip.h")).read()
    for word in ("noahmp_region_entry", "noahmp_hip_region_plan_size(", "noahmp_hip_region_plan(", "noahmp_hip_region_plan_follow(",
                 "noahmp_hip_region_step(", "NOAHMP_REG_SUM", "NOAHMP_REG_MIN", "NOAHMP_REG_MAX", "#define NOAHMP_HIP_ABI_VERSION 1"):
        assert word in hdr, word
    f90 = open(os.path.join(ROOT, "noahmp_amd", "fortran", "module_sf_noahmpdrv_hip.F90")).read()
    for name in ("noahmp_hip_region_plan_size", "noahmp_hip_region_plan", "noahmp_hip_region_plan_follow", "noahmp_hip_region_step"):
        assert "bind(C, name='%s')" % name in f90, name
        assert name in abi.EXPORTED_SYMBOLS
    assert "type, bind(C) :: noahmp_region_entry" in f90
    assert (REG_OP["sum"], REG_OP["min"], REG_OP["max"]) == (0, 1, 2)


def test_ctypes_mirror_matches_the_compiled_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "noahmp_hip.h"\nint main(){'
                   'printf("%zu %zu %zu %zu %zu %d %d", sizeof(noahmp_region_entry), offsetof(noahmp_region_entry, src),'
                   'offsetof(noahmp_region_entry, nlev), offsetof(noahmp_region_entry, lev), offsetof(noahmp_region_entry, op),'
                   'NOAHMP_REG_MAX_ENTRIES, NOAHMP_REG_CHUNK); return 0;}')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    E = abi.RegionEntry
    assert out == [C.sizeof(E), E.src.offset, E.nlev.offset, E.lev.offset, E.op.offset, 32, 256]


def _needs_flang():
    from tests.fortran import build_regions
    return pytest.mark.skipif(not build_regions.available(), reason="flang or oracle/_ref modules missing")


@_needs_flang()
def test_fortran_regions_driver_compiles_and_links():
    from tests.fortran import build_regions
    if not os.path.exists(abi.LIB_PATH):
        from noahmp_amd import build as b
        b.build()
    lib = build_regions.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib]).decode()
    assert "regions_driver_run" in out
    und = subprocess.check_output(["nm", "-D", "--undefined-only", lib]).decode()
    assert "noahmp_hip_region_plan" in und and "noahmp_hip_region_step" in und and "noahmp_hip_step_async" in und


# ---------------------------------------------------------------------------------------------------------------- GPU: raw C-ABI calls
def _block(ni, nj, xland, xice, thres=0.5):
    a = abi.StepArgs()
    a.ims = a.its = a.ids = 1
    a.jms = a.jts = a.jds = 1
    a.ime = a.ite = a.ide = ni
    a.jme = a.jte = a.jde = nj
    a.xland, a.xice, a.xice_thres = xland.data_ptr(), xice.data_ptr(), thres
    return a


def _classes(r, ncol, skipped=0.2):
    """XLAND / XICE with about `skipped` of the cells not advanced (open water or sea ice)."""
    xland = r.choice(np.array([1.0, 2.0], dtype=F), ncol, p=[1 - skipped / 2, skipped / 2])
    xice = r.choice(np.array([0.0, 1.0], dtype=F), ncol, p=[1 - skipped / 2, skipped / 2])
    return xland, xice


def _deal(counts, ncol):
    """A region map in which the regions are interleaved cell by cell (dealt round-robin, negative ids among them), not compact."""
    left = dict(counts)
    left[-1] = ncol - sum(counts.values())
    assert left[-1] >= 0
    ids = []
    while len(ids) < ncol:
        for k in sorted(left):
            if left[k] > 0:
                ids.append(k)
                left[k] -= 1
    return np.array(ids, np.int32)


class _Case:
    """Planes of one tile on the device in the column order `perm` (None: tile order), a plan, and calls of noahmp_hip_region_step."""

    def __init__(self, engine, ni, nj, region, nregion, weight, xland, xice, fields, perm=None):
        import torch
        self.torch, self.engine, self.lib = torch, engine, engine.lib
        self.ni, self.nj, self.nregion, self.fields = ni, nj, nregion, fields
        self.region_h, self.weight_h = region, weight
        self.xland_h, self.xice_h = xland, xice
        self.region = torch.from_numpy(region.reshape(nj, ni)).cuda()
        self.weight = None if weight is None else torch.from_numpy(weight.reshape(nj, ni)).cuda()
        words = C.c_int64(0)
        assert self.lib.noahmp_hip_region_plan_size(ni, nj, nregion, C.byref(words)) == 0
        self.plan = torch.zeros((words.value + 1) // 2, dtype=torch.int64, device="cuda")
        self.words = words.value
        self.scratch = None
        self.place(perm, first=True)

    def _to_order(self, x, perm, nlev=1):
        """tile-order host array -> device tensor in column order perm (position p holds tile column perm[p])"""
        torch = self.torch
        if nlev == 1:
            flat = x.ravel()
            return torch.from_numpy(np.ascontiguousarray((flat if perm is None else flat[perm]).reshape(self.nj, self.ni))).cuda()
        cols = x.reshape(self.nj, nlev, self.ni).transpose(0, 2, 1).reshape(-1, nlev)              # [tile column][level]
        cols = cols if perm is None else cols[perm]
        return torch.from_numpy(np.ascontiguousarray(cols.reshape(self.nj, self.ni, nlev).transpose(0, 2, 1))).cuda()

    def place(self, perm, first=False):
        """(Re)build the planes in column order `perm`; first: noahmp_hip_region_plan, else noahmp_hip_region_plan_follow."""
        torch = self.torch
        self.xland, self.xice = self._to_order(self.xland_h, perm), self._to_order(self.xice_h, perm)
        self.dev = [None if x is None else self._to_order(x, perm, nl) for x, op, nl, lev in self.fields]
        inv = None
        if perm is not None:
            inv_h = np.empty(perm.size, np.int32)
            inv_h[perm] = np.arange(perm.size, dtype=np.int32)
            inv = torch.from_numpy(inv_h).cuda()
        self.inv = inv
        torch.cuda.synchronize()
        if first:
            rc = self.lib.noahmp_hip_region_plan(self.region.data_ptr(), self.weight.data_ptr() if self.weight is not None else None, self.ni,
                                                 self.nj, self.nregion, inv.data_ptr() if inv is not None else None, self.plan.data_ptr(),
                                                 self.words, None)
        else:
            rc = self.lib.noahmp_hip_region_plan_follow(self.plan.data_ptr(), inv.data_ptr() if inv is not None else None, None)
        assert rc == 0, self.lib.noahmp_hip_last_error().decode()
        self.entries = self.engine.region_entries([(t, op, lev) for t, (x, op, nl, lev) in zip(self.dev, self.fields)])

    def step(self, series, slot, acc=None):
        torch = self.torch
        n = len(self.fields)
        b = C.c_int64(0)
        assert self.lib.noahmp_hip_region_scratch_size(self.plan.data_ptr(), n, C.byref(b)) == 0
        if self.scratch is None or self.scratch.numel() * 8 < b.value:
            self.scratch = torch.zeros((b.value + 7) // 8, dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
        rc = self.lib.noahmp_hip_region_step(self.plan.data_ptr(), n, self.entries, C.byref(_block(self.ni, self.nj, self.xland, self.xice)),
                                             series.data_ptr(), int(series.shape[0]), slot, acc.data_ptr() if acc is not None else None,
                                             self.scratch.data_ptr(), None)
        assert rc == 0, self.lib.noahmp_hip_last_error().decode()
        self.engine.stream_sync()

    def want(self):
        part = np_takes_part(self.xland_h, self.xice_h, 0.5)
        planes = []
        for x, op, nl, lev in self.fields:
            planes.append((None if x is None else (x if nl == 1 else x.reshape(self.nj, nl, self.ni)[:, lev, :]), op))
        return np_series(self.region_h, self.nregion, self.weight_h, part, planes)


def _series(nslot, n, nregion, fill=-7.0):
    import torch
    t = torch.full((nslot, n, nregion), fill, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    return t


@pytest.mark.gpu
def test_region_sizes_at_the_trees_edges(engine):
    """One map with 0, 1, 63, 255, 256, 257 and 513 members per region, one region without a participating cell, negative cells, the
    regions interleaved cell by cell, rows of 259 cells; about 20 % of the cells skipped by XLAND / XICE."""
    ni, nj = 259, 8
    ncol = ni * nj
    sizes = {0: 0, 1: 1, 2: 63, 3: 255, 4: 256, 5: 257, 6: 513, 7: 40}
    region = _deal(sizes, ncol)
    assert (region < 0).sum() == ncol - sum(sizes.values()) and all((region == k).sum() == v for k, v in sizes.items())
    r = np.random.default_rng(21)
    xland, xice = _classes(r, ncol)
    xland[region == 7] = 2.0                                            # region 7: members, none of which takes part
    xland[region == 1], xice[region == 1] = 1.0, 0.0                    # the single member of region 1 does
    part = np_takes_part(xland, xice, 0.5)
    assert 0.1 < (~part).mean() < 0.3 and not part[region == 7].any() and all(part[region == k].any() for k in range(1, 7))
    weight = r.uniform(0.5, 2.0, ncol).astype(F)
    fields = [(mixed(r, ncol), "sum", 1, 0), (None, "sum", 1, 0), (mixed(r, ncol), "min", 1, 0), (mixed(r, ncol), "max", 1, 0)]
    c = _Case(engine, ni, nj, region, 8, weight, xland, xice, fields)
    series = _series(1, 4, 8)
    c.step(series, 0)
    got, want = series.cpu().numpy()[0], c.want()
    assert_same(got, want, "series")
    assert got[0, 0] == 0.0 and got[2, 0] == HUGE and got[3, 0] == -HUGE            # the empty region
    assert got[0, 7] == 0.0 and got[1, 7] == 0.0 and got[2, 7] == HUGE              # members, none taking part
    assert np.count_nonzero(got[0]) == 6 and (got[1, 1:7] > 0).all()


@pytest.mark.gpu
def test_three_levels(engine):
    """One region of 65 537 members (257 chunks: a third level) plus small ones on a 300 x 256 tile."""
    ni, nj = 300, 256
    ncol = ni * nj
    sizes = {0: 700, 1: 65537, 2: 257, 3: 1, 4: 5000}
    region = _deal(sizes, ncol)
    r = np.random.default_rng(22)
    xland, xice = _classes(r, ncol)
    weight = r.uniform(0.5, 2.0, ncol).astype(F)
    fields = [(mixed(r, ncol), "sum", 1, 0), (mixed(r, ncol), "max", 1, 0)]
    c = _Case(engine, ni, nj, region, 5, weight, xland, xice, fields)
    series = _series(1, 2, 5)
    c.step(series, 0)
    assert_same(series.cpu().numpy()[0], c.want(), "series")


@pytest.mark.gpu
@pytest.mark.parametrize("n, weighted", [(1, False), (5, True), (32, False), (32, True)])
def test_entries_ops_levels_ring_and_accumulators(engine, n, weighted):
    """n entries with the ops in turn, one of them a level of a 4-level array, one the constant 1 (src = NULL), nasty() values; two calls
    into ring slots 3 % 2 and 4 % 2 with the interval accumulators carried across them."""
    ni, nj, nregion = 67, 9, 6
    ncol = ni * nj
    r = np.random.default_rng(30 + n + weighted)
    region = r.integers(-1, nregion, ncol).astype(np.int32)
    xland, xice = _classes(r, ncol)
    weight = nasty(r, ncol) if weighted else None
    fields = []
    for f in range(n):
        op = OPS[f % 3]
        if f == 1:
            fields.append((nasty(r, ncol * 4), op, 4, 2))               # level 2 of a (nj, 4, ni) array
        elif f == 3:
            fields.append((None, op, 1, 0))
        else:
            fields.append((nasty(r, ncol), op, 1, 0))
    c = _Case(engine, ni, nj, region, nregion, weight, xland, xice, fields)
    import torch
    series = _series(2, n, nregion)
    ident = np.array([{"sum": 0.0, "min": HUGE, "max": -HUGE}[op] for x, op, nl, lev in fields])
    acc = torch.from_numpy(np.repeat(ident[:, None], nregion, axis=1).copy()).cuda()
    torch.cuda.synchronize()
    c.step(series, 3, acc)
    first = series.cpu().numpy().copy()
    assert (first[0] == -7.0).all()                                     # slot 3 % 2 = 1 was written, slot 0 was not
    want1 = c.want()
    assert_same(first[1], want1, "slot 1")
    # other values for the second call: the same planes, rewritten in place
    fields2 = [(None if x is None else nasty(r, x.size), op, nl, lev) for x, op, nl, lev in fields]
    for t, (x, op, nl, lev) in zip(c.dev, fields2):
        if t is not None:
            t.copy_(torch.from_numpy(x.reshape(tuple(t.shape))))
    torch.cuda.synchronize()
    c.fields = fields2
    c.step(series, 4, acc)
    second = series.cpu().numpy()
    want2 = c.want()
    assert_same(second[0], want2, "slot 0")
    assert_same(second[1], want1, "slot 1 is left alone")
    want_acc = np.stack([np_acc(op, np_acc(op, np.full(nregion, ident[f]), want1[f]), want2[f]) for f, (x, op, nl, lev) in enumerate(fields)])
    assert_same(acc.cpu().numpy(), want_acc, "acc")
    if n >= 5:
        assert np.isnan(want1).any() and np.isfinite(want1).any()


@pytest.mark.gpu
@pytest.mark.parametrize("layered", [False, True])
def test_layout_invariance(engine, layered):
    """The same planes in tile order, under a random permutation (positions from inv_perm) and, after noahmp_hip_region_plan_follow, under
    a second one give the series of the tile-order call, value for value.  The input is such that another order of the additions would show."""
    ni, nj, nregion = 131, 23, 4
    ncol = ni * nj
    r = np.random.default_rng(41 + layered)
    region = _deal({0: 1500, 1: 700, 2: 300, 3: 257}, ncol)
    xland, xice = _classes(r, ncol)
    weight = r.uniform(0.5, 2.0, ncol).astype(F)
    fields = [(mixed(r, ncol), "sum", 1, 0), (None, "sum", 1, 0), (mixed(r, ncol), "min", 1, 0), (mixed(r, ncol), "max", 1, 0),
              (mixed(r, ncol), "sum", 1, 0)]
    if layered:
        fields[2] = (mixed(r, ncol * 4), "sum", 4, 1)
    # the restatement over a shuffled member list differs for this input
    m = np.flatnonzero(region == 0)
    t = np_terms("sum", np_takes_part(xland, xice, 0.5)[m], weight[m], fields[0][0][m])
    assert any(S_fast(t) != S_fast(r.permutation(t)) for _ in range(4))
    base = _Case(engine, ni, nj, region, nregion, weight, xland, xice, fields)
    s0 = _series(1, len(fields), nregion)
    base.step(s0, 0)
    ref = s0.cpu().numpy()[0]
    assert_same(ref, base.want(), "tile order")
    lib = engine.lib
    perm1, perm2 = r.permutation(ncol).astype(np.int32), r.permutation(ncol).astype(np.int32)
    c = _Case(engine, ni, nj, region, nregion, weight, xland, xice, fields, perm=perm1)
    for which, perm in (("first permutation", None), ("after plan_follow", perm2)):
        if perm is not None:
            c.place(perm)
        s = _series(1, len(fields), nregion)
        c.step(s, 0)
        assert_same(s.cpu().numpy()[0], ref, which)
    c.place(None)                                                       # ... and back to tile order: follow with inv_perm = NULL
    s = _series(1, len(fields), nregion)
    c.step(s, 0)
    assert_same(s.cpu().numpy()[0], ref, "back in tile order")
    # the scratch a plan asks for does not change when the plan follows a sort
    b0, b1 = C.c_int64(0), C.c_int64(0)
    assert lib.noahmp_hip_region_scratch_size(base.plan.data_ptr(), len(fields), C.byref(b0)) == 0
    base.place(perm1)
    assert lib.noahmp_hip_region_scratch_size(base.plan.data_ptr(), len(fields), C.byref(b1)) == 0
    assert b0.value == b1.value
    s = _series(1, len(fields), nregion)
    base.step(s, 0)
    assert_same(s.cpu().numpy()[0], ref, "tile-order plan after plan_follow")


@pytest.mark.gpu
def test_refusals_launch_nothing(engine):
    import torch
    lib = engine.lib
    ni, nj, nregion = 64, 2, 3
    ncol = ni * nj
    region = (np.arange(ncol) % nregion).astype(np.int32)
    x = np.full(ncol, 2.0, F)
    c = _Case(engine, ni, nj, region, nregion, None, np.ones(ncol, F), np.zeros(ncol, F), [(x, "sum", 1, 0)])
    series = _series(2, 1, nregion, fill=9.0)
    acc = torch.full((1, nregion), 5.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    c.step(series, 0)                                                   # sizes the scratch
    series.fill_(9.0)
    torch.cuda.synchronize()
    blk = _block(ni, nj, c.xland, c.xice)

    def call(n=1, entries=None, ring=series, block=blk, plan=c.plan):
        e = entries if entries is not None else c.entries
        rc = lib.noahmp_hip_region_step(plan.data_ptr(), n, e, C.byref(block), ring.data_ptr() if ring is not None else None, 2, 0,
                                        acc.data_ptr(), c.scratch.data_ptr(), None)
        return rc, lib.noahmp_hip_last_error().decode()

    # an id >= nregion: refused at plan time, and the workspace is no plan afterwards
    bad = region.copy()
    bad[77] = nregion
    bad_d = torch.from_numpy(bad.reshape(nj, ni)).cuda()
    plan2 = torch.zeros_like(c.plan)
    torch.cuda.synchronize()
    rc = lib.noahmp_hip_region_plan(bad_d.data_ptr(), None, ni, nj, nregion, None, plan2.data_ptr(), c.words, None)
    assert rc == -105 and "nregion" in lib.noahmp_hip_last_error().decode()
    rc, msg = call(plan=plan2)
    assert rc == -105 and "plan" in msg
    rc = lib.noahmp_hip_region_plan(c.region.data_ptr(), None, ni, nj, nregion, None, plan2.data_ptr(), c.words - 1, None)
    assert rc == -105 and "words" in lib.noahmp_hip_last_error().decode()
    e33 = engine.region_entries([(c.dev[0], "sum", None)] * 33)
    rc, msg = call(n=33, entries=e33)
    assert rc == -107 and "entries" in msg
    rc, msg = call(entries=engine.region_entries([(c.dev[0], 3, None)]))
    assert rc == -105 and "op" in msg
    rc, msg = call(ring=None)
    assert rc == -105 and "ring" in msg
    halo = _block(ni, nj, c.xland, c.xice)
    halo.its = 2
    rc, msg = call(block=halo)
    assert rc == -105 and "tile" in msg
    other = _block(ni // 2, nj * 2, c.xland, c.xice)
    rc, msg = call(block=other)
    assert rc == -105 and "tile" in msg
    engine.stream_sync()
    assert (series == 9.0).all() and (acc == 5.0).all()
    rc, msg = call()                                                    # ... and the same objects in a valid call
    engine.stream_sync()
    assert rc == 0, msg
    cnt = np.bincount(region, minlength=nregion)
    assert_same(series.cpu().numpy()[0, 0], 2.0 * cnt, "valid call")
    assert_same(acc.cpu().numpy()[0], 5.0 + 2.0 * cnt, "acc")
    assert (series[1] == 9.0).all()


# ---------------------------------------------------------------------------------------------------------------- GPU: end to end
NSTEP, NI, NJ = 24, 64, 4
FKEYS = ("coszin", "swdown", "glw", "t3d", "rainbl")
WATCH = ("runsfxy", "hfx", "t2mvxy", "smois")
NREGION = 5
# (name, field, op, level): what the scenario keeps per region and step
KEEP = [("runoff", "runsfxy", "sum", None), ("hfx", "hfx", "sum", None), ("sm_top", "smois", "sum", 0), ("t2mv_max", "t2mvxy", "max", None)]


def _start(tables):
    """The 64 x 4, 24-step scenario of the history tests: mixed land with 8 open-water and 8 sea-ice cells."""
    s = synth.mixed_small(tables[1], ni=NI, nj=NJ)
    r = np.random.default_rng(11)
    cells = r.choice(NI * NJ, 16, replace=False)
    for c in cells[:8]:
        s["xland"][c // NI, c % NI] = 2.0
    for c in cells[:4]:
        s["ivgtyp"][c // NI, c % NI] = s.cfg.iswater
    for c in cells[8:]:
        s["xice"][c // NI, c % NI] = 1.0
    synth.first_step_fixups(s)
    return s, np.sort(cells)


def _regions_of(skipped):
    """Four basins in vertical stripes with a few cells in none, and a fifth that consists of the skipped cells only; cell areas."""
    r = np.random.default_rng(14)
    reg = ((np.arange(NI * NJ) % NI) * 4 // NI).astype(np.int32)
    reg[r.choice(NI * NJ, 20, replace=False)] = -1
    reg[skipped] = 4
    area = r.uniform(0.8e6, 1.2e6, NI * NJ).astype(F)
    return reg.reshape(NJ, NI), area.reshape(NJ, NI)


def _forcing(s, it):
    synth.diurnal_forcing(s, (it - 1) % 24, t_offset=s.t_offset)
    return {k: s.a[k].copy() for k in FKEYS}


@pytest.fixture(scope="module")
def oracle_series(port, tables):
    """The C restatement of the reference advanced 24 steps; the restatement of the region series applied to its per-step arrays."""
    s, skipped = _start(tables)
    reg, area = _regions_of(skipped)
    o = s.copy()
    part = np_takes_part(s["xland"], s["xice"], s.cfg.xice_thres)
    assert set(np.flatnonzero(~part.ravel())) == set(skipped)
    out = {name: [] for name, f, op, lev in KEEP}
    wsum = []
    for it in range(1, NSTEP + 1):
        o.a.update(_forcing(s, it))
        st = port.noahmplsm(o, it, 2000, 180.0)
        assert st.code == 0
        planes = [(None, "sum")] + [((o.a[f] if lev is None else o.a[f][:, lev, :]).copy(), op) for name, f, op, lev in KEEP]
        sr = np_series(reg, NREGION, area, part, planes)
        wsum.append(sr[0])
        for k, (name, f, op, lev) in enumerate(KEEP):
            out[name].append(sr[k + 1])
    return {k: np.stack(v) for k, v in out.items()}, np.stack(wsum)


def _engine_run(engine, tables, sorted_layout):
    """The engine advanced through the same chain with a Regions sample after every step, read back after steps 8, 16 and 24 through a
    ring of 8 slots; sorted_layout: the store is sorted before the first step and re-sorted (other keys) before step 13."""
    import torch
    from noahmp_amd.history import Regions
    s, skipped = _start(tables)
    reg, area = _regions_of(skipped)
    d = s.to_device("cuda:0")
    perm = engine.sort_store(d, tsk_bin=0) if sorted_layout else None
    first_perm = perm.clone() if sorted_layout else None
    work = {k: d.a[k] for k in FKEYS}
    src0 = {k: torch.from_numpy(s.a[k].copy()).cuda() for k in FKEYS}
    sc = engine.scatter([work[k] for k in FKEYS], [src0[k] for k in FKEYS], perm, NI, NJ) if sorted_layout else None
    rg = Regions(engine, d, reg, NREGION, weight=area, nslot=8)
    for name, f, op, lev in KEEP:
        rg.add(name, f, op=op, level=lev)
    got, means = {name: [] for name, f, op, lev in KEEP}, {}
    for it in range(1, NSTEP + 1):
        f = _forcing(s, it)
        if sorted_layout:
            if it == NSTEP // 2 + 1:
                perm = engine.sort_store(d)
                work = {k: d.a[k] for k in FKEYS}
                sc.set_dests([work[k] for k in FKEYS])
                sc.set_perm(perm)
                rg.follow(d)
            dev = [torch.from_numpy(f[k]).cuda() for k in FKEYS]
            torch.cuda.synchronize()
            sc.set_sources(dev)
            sc()
        else:
            for k in FKEYS:
                d.a[k].copy_(torch.from_numpy(f[k]))
            torch.cuda.synchronize()
        st = engine.noahmplsm(d, it, 2000, 180.0)
        assert st.code == 0
        rg.step()
        if it % 8 == 0:
            rec = rg.read()
            for k, v in rec.items():
                got[k].append(v)
            for k, v in rg.means().items():
                means.setdefault(k, []).append(v)
    engine.stream_sync()
    return dict(series={k: np.concatenate(v) for k, v in got.items()}, means={k: np.concatenate(v) for k, v in means.items()},
                acc=rg.acc.cpu().numpy(), resorted=sorted_layout and not torch.equal(perm, first_perm))


@pytest.mark.gpu
def test_engine_series_equal_the_oracle_in_tile_order_and_sorted(engine, tables, oracle_series):
    """Regions series of runsfxy, hfx, smois level 0 (area-weighted sums) and t2mvxy (max) over 5 regions, the last one on skipped cells
    only: the restatement applied to the oracle's per-step arrays, in tile order and in the sorted layout with a re-sort before step 13
    that Regions.follow tracks; the two runs equal each other."""
    want, wsum = oracle_series
    tile = _engine_run(engine, tables, False)
    srt = _engine_run(engine, tables, True)
    assert srt["resorted"]
    for name, f, op, lev in KEEP:
        assert want[name].shape == (NSTEP, NREGION)
        assert_same(tile["series"][name], want[name], name + " (tile order)")
        assert_same(srt["series"][name], want[name], name + " (sorted layout)")
        assert_same(srt["series"][name], tile["series"][name], name + " (tile order vs sorted)")
    assert (want["hfx"][:, 4] == 0.0).all() and (want["t2mv_max"][:, 4] == -HUGE).all() and (wsum[:, 4] == 0.0).all()
    assert np.count_nonzero(want["hfx"][:, :4]) == 4 * NSTEP and np.count_nonzero(want["runoff"]) > 0
    with np.errstate(all="ignore"):
        for name in ("runoff", "hfx", "sm_top"):
            assert_same(tile["means"][name], want[name] / wsum, name + " mean")
            assert_same(srt["means"][name], want[name] / wsum, name + " mean (sorted)")
    assert (tile["means"]["sm_top"][:, :4] > 0.02).all() and (tile["means"]["sm_top"][:, :4] < 1.0).all()
    # the interval accumulators: sums of the step sums, maxima of the maxima (entry 0 is the summed weights)
    a = np.zeros(NREGION)
    for it in range(NSTEP):
        a = a + wsum[it]
    acc_want = [a]
    for name, f, op, lev in KEEP:
        a = np.full(NREGION, 0.0 if op == "sum" else -HUGE)
        for it in range(NSTEP):
            a = np_acc(op, a, want[name][it])
        acc_want.append(a)
    assert_same(tile["acc"], np.stack(acc_want), "acc")
    assert_same(srt["acc"], np.stack(acc_want), "acc (sorted)")


@pytest.mark.gpu
@_needs_flang()
def test_fortran_regions_driver_equals_the_python_path(engine, tables):
    """tests/fortran/regions_driver.f90 -- the device-resident loop with a basin series of RUNSFXY through the generated interfaces --
    gives the series of the same chain driven from Python (Regions)."""
    import torch
    from tests.fortran import build_regions
    from noahmp_amd.history import Regions
    lib = C.CDLL(build_regions.build())
    lib.regions_driver_run.argtypes = [C.POINTER(abi.StepArgs), C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p,
                                       C.c_int, C.c_void_p]
    engine.lib.noahmp_hip_set_tables(C.byref(tables[0]))
    r = np.random.default_rng(9)
    s = synth.mixed_small(tables[1], ni=96, nj=6, seed=19)
    synth.diurnal_forcing(s, 12, t_offset=s.t_offset)
    s["xlatin"] = r.uniform(-60.0, 70.0, size=(s.nj, s.ni)).astype(F)
    s["xland"][0, :5] = 2.0
    lon = r.uniform(-180.0, 180.0, size=(s.nj, s.ni)).astype(F)
    rain = np.where(r.random((s.nj, s.ni)) < 0.3, 4e-4, 0.0).astype(F)
    nsteps, iday0, nregion = 30, 200, 7
    reg = r.integers(-1, nregion, (s.nj, s.ni)).astype(np.int32)
    area = r.uniform(0.8e6, 1.2e6, (s.nj, s.ni)).astype(F)
    # Python
    d = s.to_device("cuda:0")
    dlon, drain = torch.from_numpy(lon).cuda(), torch.from_numpy(rain).cuda()
    rg = Regions(engine, d, reg, nregion, weight=area, nslot=nsteps)
    rg.add("runoff", "runsfxy")
    torch.cuda.synchronize()
    args = d.step_args(1, 2000, 0.0)
    for n in range(nsteps):
        jul = engine.forcing_prep(d, dlon, drain, iday0 + n // 24, n % 24, first_step=(n == 0), wait=False)
        args.itimestep, args.julian = n + 1, jul
        engine.noahmplsm_async(args)
        rg.step()
    st, _ = engine.sync()
    assert st.code == 0
    py = rg.read()["runoff"]
    wsum = rg._last[Regions.WEIGHT]
    # Fortran
    f = s.copy()
    series = np.zeros((nsteps, 2, nregion), D)
    a = f.step_args(1, 2000, 0.0)
    rc = lib.regions_driver_run(C.byref(a), lon.ctypes.data, rain.ctypes.data, nsteps, iday0, s.cfg.zlvl, reg.ctypes.data, area.ctypes.data,
                                nregion, series.ctypes.data)
    assert rc == 0, engine.lib.noahmp_hip_last_error().decode()
    assert_same(series[:, 0, :], py, "runoff series")
    assert_same(series[:, 1, :], wsum, "summed weights")
    assert np.count_nonzero(py) > 20 and (wsum > 0).all()
