"""Budget-preserving regrid of fluxes (noahmp_regrid_conserve.hip, nmp_dev_regrid_conserve.hpp): the bilinear field, optionally shaped
by a pattern, rescaled so that the area-weighted mean over the model cells of each source cell is the source cell's value.

No reference routine stands behind the calls: the contract is the text in include/noahmp_hip.h.  np_conserve below restates that text in
numpy on top of test_regrid's np_plan / np_regrid -- float32 values, float64 terms, the summation tree S written out here -- and every
output is compared with it bit for bit (NaN equals NaN): the per-cell functions compiled for the host, the kernels at every chunk and
level boundary, any column order, decomposed windows, and an engine chain fed through ForcingRegrid.record(modes={"pcp": "conserve"})."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from noahmp_amd import abi
from test_regrid import (BIL, CSRC, F, D, ROOT, SOURCES, assert_same, mask, nasty, np_plan, np_regrid, plan_case, source, targets, _flang)

SRC = os.path.join(ROOT, "tests", "host_emul", "regrid_conserve_check.hip")
LIB = os.path.join(ROOT, "tests", "host_emul", "libregrid_conserve_check.so")
BOUND = 2.0 ** -22
NAMES = ("noahmp_hip_regrid_conserve_plan_size", "noahmp_hip_regrid_conserve_plan", "noahmp_hip_regrid_conserve_scratch_size",
         "noahmp_hip_forcing_regrid_conserve")


# ---------------------------------------------------------------------------------------------------------------- the restatement
def np_S(terms):
    """S of the header: chunks of 256 consecutive terms, the last padded with +0.0, folded h = 128 .. 1, again on the partials."""
    t = np.asarray(terms, D).ravel()
    if t.size == 0:
        return D(0.0)
    with np.errstate(all="ignore"):
        while True:
            nch = -(-t.size // 256)
            v = np.zeros(nch * 256, D)
            v[:t.size] = t
            v = v.reshape(nch, 256)
            h = 128
            while h > 0:
                v[:, :h] = v[:, :h] + v[:, h:2 * h]
                h //= 2
            t = v[:, 0].copy()
            if t.size == 1:
                return t[0]


def np_groups(plan, g):
    """The owner of every window cell, -1 for the cells that are no members."""
    n, nx, per = plan.shape[1], int(g.nx), bool(g.periodic_x)
    nxny = nx * int(g.ny)
    w = plan[2:].view(F)
    grp = np.full(n, -1, np.int64)
    for c in range(n):
        b, nr = int(plan[0, c]), int(plan[1, c])
        if b < 0 or b >= nxny or nr < 0 or nr >= nxny:
            continue
        c1 = b + 1 - nx if (per and b % nx == nx - 1) else b + 1
        idx = [b, c1, b + nx, c1 + nx]
        if any(w[k, c] != 0 and idx[k] >= nxny for k in range(1, 4)):
            continue
        grp[c] = nr
    return grp


def np_conserve(plan, g, src, area=None, pattern=None, fill=-999.0, grp=None):
    """The header text for one entry over a window.  Returns (out [n] in window order, N {group: float64}, r {group: (kind, value)})."""
    n = plan.shape[1]
    grp = np_groups(plan, g) if grp is None else grp
    src = np.asarray(src, F)
    a = np.ones(n, F) if area is None else np.asarray(area, F).ravel()
    out = np.full(n, F(fill), F)
    with np.errstate(all="ignore"):
        gb = np_regrid(plan, g, src, BIL, fill=0.0)                     # the bits of noahmp_hip_forcing_regrid
        q = gb if pattern is None else gb * np.asarray(pattern, F).ravel()
        v = np.where(q > 0, q, F(0.0)).astype(F)
        N, R = {}, {}
        for s in np.unique(grp[grp >= 0]):
            m = np.flatnonzero(grp == s)                                # ascending window index
            Ns = np_S(a[m].astype(D) * v[m].astype(D))
            Ds = np_S(a[m].astype(D))
            p = src[s]
            N[int(s)] = Ns
            if not p > 0:
                out[m] = F(0.0)
                R[int(s)] = (0, F(0.0))
            elif Ns > 0:
                r = F((D(p) * Ds) / Ns)
                out[m] = v[m] * r
                R[int(s)] = (1, r)
            else:
                out[m] = p
                R[int(s)] = (2, p)
    return out, N, R


def group_sum_plane(N, nxny, poison=-7.0):
    x = np.full(nxny, poison, D)
    for s, v in N.items():
        x[s] = v
    return x


def assert_same64(a, b, what):
    a, b = np.ascontiguousarray(a, D), np.ascontiguousarray(b, D)
    bad = ~((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b)))
    if bad.any():
        i = int(np.flatnonzero(bad.ravel())[0])
        raise AssertionError("%s: %d of %d float64 values differ, first at %d: %r vs %r" % (what, bad.sum(), bad.size, i, a.ravel()[i], b.ravel()[i]))


def conservation(out, grp, src, area, what):
    """For every group with p > 0: |sum(area*out) - p*sum(area)| / (p*sum(area)) < 2^-22 in float64 on the stored float32 outputs."""
    a = np.ones(out.size, D) if area is None else np.asarray(area, D).ravel()
    seen = 0
    for s in np.unique(grp[grp >= 0]):
        p = D(src[s])
        if not p > 0:
            continue
        m = grp == s
        lhs, rhs = np.sum(a[m] * out[m].astype(D)), p * np.sum(a[m])
        dev = abs(lhs - rhs) / rhs
        assert dev < BOUND, "%s: group %d deviates by %.3g (2^%.1f)" % (what, s, dev, np.log2(max(dev, 1e-300)))
        seen += 1
    return seen


# ---------------------------------------------------------------------------------------------------------------- host compilation
def build():
    deps = [SRC, os.path.join(CSRC, "nmp_dev_regrid_conserve.hpp"), os.path.join(CSRC, "nmp_dev_regrid.hpp"),
            os.path.join(CSRC, "nmp_dev_regions.hpp"), os.path.join(ROOT, "include", "noahmp_hip.h")]
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
    lib.conserve_groups.argtypes = [C.c_void_p, C.c_long, C.POINTER(abi.RegridSource), C.c_void_p]
    lib.conserve_groups.restype = None
    lib.conserve_run.argtypes = [C.c_void_p, C.c_long, C.POINTER(abi.RegridSource), C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_void_p]
    lib.conserve_run.restype = C.c_long
    return lib


def _ptr(a):
    return a.ctypes.data if a is not None else None


def operands(name, ncell, seed, kind):
    """src, area, pattern of a case.  kind "nasty": NaN, Inf, zeros, negatives, denormals in src, zeros in the pattern;
    "flux": a precipitation-like field in float32's normal range with zeros, negatives and NaN in it (the conservation bound's premise:
    r and the products are neither denormal nor overflow)."""
    g = SOURCES[name]
    r = np.random.default_rng(seed)
    nxny = g.nx * g.ny
    if kind == "nasty":
        src = nasty(r, nxny)
        src[r.random(nxny) < 0.4] = F(r.uniform(0.1, 3.0))
    else:
        src = r.uniform(1e-5, 5e-3, nxny).astype(F)
        at = r.random(nxny)
        src[at < 0.15] = 0.0
        src[(at >= 0.15) & (at < 0.25)] = F(-1e-4)
        src[(at >= 0.25) & (at < 0.30)] = np.nan
    area = r.uniform(0.5e6, 1.5e6, ncell).astype(F)
    pattern = r.uniform(0.25, 4.0, ncell).astype(F)
    pattern[r.random(ncell) < 0.1] = 0.0
    return src, area, pattern


@functools.lru_cache(maxsize=None)
def value_case(name, kind, seed_kind):
    """One window (67 x 5 targets of test_regrid) with its restated results for the four combinations of area and pattern."""
    _, _, v, plan, _ = plan_case(name, 67, 5, kind, 2)
    g = SOURCES[name]
    n = plan.shape[1]
    src, area, pattern = operands(name, n, 7 + len(name), seed_kind)
    grp = np_groups(plan, g)
    if v is not None and seed_kind == "nasty":
        src = src.copy()
        src[v == 0] = np.nan                                            # NaN behind the mask: a dropped corner is never read
    pattern = pattern.copy()
    wet = [s for s in np.unique(grp[grp >= 0]) if src[s] > 0]
    if wet:
        pattern[grp == wet[0]] = 0.0                                    # the pattern is zero on a whole wet footprint: out = p
    res = {}
    for ua in (False, True):
        for up in (False, True):
            res[ua, up] = np_conserve(plan, g, src, area if ua else None, pattern if up else None, -999.0, grp)
    return plan, grp, src, area, pattern, res


@pytest.mark.parametrize("name", list(SOURCES))
@pytest.mark.parametrize("kind", ["none", "random"])
def test_host_compilation_equals_numpy(name, kind):
    """nmp_dev_regrid_conserve.hpp compiled for the host against the restatement: outputs and the N_s plane, with and without a mask,
    area and pattern; NaN / Inf / zero / negative / denormal sources, zeros in the pattern; the out = p branch is taken."""
    lib = _host()
    g = SOURCES[name]
    plan, grp, src, area, pattern, res = value_case(name, kind, "nasty")
    n, nxny = plan.shape[1], g.nx * g.ny
    hg = np.zeros(n, np.int32)
    lib.conserve_groups(plan.ctypes.data, n, C.byref(g), hg.ctypes.data)
    assert np.array_equal(hg, grp)
    assert (grp < 0).any() and (grp >= 0).sum() > 100
    kinds = set()
    for (ua, up), (want, N, R) in res.items():
        got = np.full(n, 7.0, F)
        ns, ds = np.full(nxny, -7.0, D), np.full(nxny, -7.0, D)
        bad = lib.conserve_run(plan.ctypes.data, n, C.byref(g), src.ctypes.data, _ptr(area if ua else None), _ptr(pattern if up else None), -999.0,
                               got.ctypes.data, ns.ctypes.data, ds.ctypes.data, None)
        assert bad == 0
        assert_same(got, want, "%s mask %s area %d pattern %d" % (name, kind, ua, up))
        assert_same64(ns, group_sum_plane(N, nxny), "%s mask %s area %d pattern %d: N_s" % (name, kind, ua, up))
        kinds |= {k for k, _ in R.values()}
        if up:
            assert any(k == 2 for k, _ in R.values()), "the out = p branch is not taken"
    assert kinds == {0, 1, 2}


def test_host_compilation_reads_no_dropped_corner_and_refuses_bad_area():
    lib = _host()
    g = SOURCES["plain"]
    plan, grp, src, area, pattern, res = value_case("plain", "random", "nasty")
    n, nxny = plan.shape[1], g.nx * g.ny
    reads = np.zeros(nxny, np.int32)
    got, ns, ds = np.zeros(n, F), np.zeros(nxny, D), np.zeros(nxny, D)
    lib.conserve_run(plan.ctypes.data, n, C.byref(g), src.ctypes.data, None, None, -999.0, got.ctypes.data, ns.ctypes.data, ds.ctypes.data,
                     reads.ctypes.data)
    v = mask("plain", "random")
    assert (reads[v == 0] == 0).all() and reads.sum() > 0
    for bad_value in (0.0, -1.0, np.nan, np.inf):
        a = area.copy()
        a[np.flatnonzero(grp >= 0)[3]] = bad_value
        assert lib.conserve_run(plan.ctypes.data, n, C.byref(g), src.ctypes.data, a.ctypes.data, None, -999.0, got.ctypes.data, ns.ctypes.data,
                                ds.ctypes.data, None) == 1
    a = area.copy()
    a[np.flatnonzero(grp < 0)] = np.nan                                 # a non-member's area is not looked at
    assert lib.conserve_run(plan.ctypes.data, n, C.byref(g), src.ctypes.data, a.ctypes.data, None, -999.0, got.ctypes.data, ns.ctypes.data,
                            ds.ctypes.data, None) == 0


@pytest.mark.parametrize("name", list(SOURCES))
@pytest.mark.parametrize("kind", ["none", "random"])
def test_conservation_bound_holds_for_every_wet_group(name, kind):
    """sum(area*out) = p*sum(area) within 2^-22 for every group with p > 0, none left out, through the host compilation: zeros, negatives
    and NaN among the sources, zeros in the pattern, the out = p branch among the groups."""
    lib = _host()
    g = SOURCES[name]
    plan, grp, src, area, pattern, res = value_case(name, kind, "flux")
    n, nxny = plan.shape[1], g.nx * g.ny
    for (ua, up), (want, N, R) in res.items():
        got = np.full(n, 7.0, F)
        ns, ds = np.zeros(nxny, D), np.zeros(nxny, D)
        lib.conserve_run(plan.ctypes.data, n, C.byref(g), src.ctypes.data, _ptr(area if ua else None), _ptr(pattern if up else None), -999.0,
                         got.ctypes.data, ns.ctypes.data, ds.ctypes.data, None)
        assert_same(got, want, "%s %s" % (name, kind))
        seen = conservation(got, grp, src, area if ua else None, "%s mask %s area %d pattern %d" % (name, kind, ua, up))
        assert seen == sum(1 for s in R if src[s] > 0) and seen >= 3


def test_restatement_identity_on_cell_centres():
    """Model cells on the source's cell centres: every group has one member and r is exactly 1, so out = p where p > 0 (NaN where p is
    +Inf), else +0.0."""
    r = np.random.default_rng(3)
    for name, g in SOURCES.items():
        jj, ii = np.meshgrid(np.arange(g.ny), np.arange(g.nx), indexing="ij")
        plan, unf = np_plan((g.lat0 + jj * g.dlat).astype(F), (g.lon0 + ii * g.dlon).astype(F), g)
        assert unf == 0
        src = nasty(r, g.nx * g.ny)
        area = r.uniform(0.5, 2.0, src.size).astype(F)
        with np.errstate(all="ignore"):
            want = np.where(src > 0, src, F(0.0)).astype(F)
        want[src == np.inf] = np.nan                                    # no guard: (inf * D) / inf is the arithmetic's own NaN
        for a in (None, area):
            out, N, R = np_conserve(plan, g, src, a)
            assert_same(out, want, "identity " + name)
            assert all(v == 1.0 for s, (k, v) in R.items() if k == 1 and src[s] < np.inf)


def test_restatement_ratio_is_at_most_four_and_a_flat_field_is_unchanged():
    """Without mask and pattern the near corner's weight is at least 1/4, so r <= 4 on a non-negative field; a flat field on targets whose
    weights are exact in float32 (fractions that are multiples of 1/16) comes back unchanged, bit for bit."""
    r = np.random.default_rng(4)
    for name in SOURCES:
        g = SOURCES[name]
        xlat, xlon = targets(name, 67, 5)
        plan, _ = np_plan(xlat, xlon, g)
        src = r.uniform(0.0, 1.0, g.nx * g.ny).astype(F) ** 8            # mostly small, a few large: steep gradients
        src[r.random(src.size) < 0.2] = 0.0
        out, N, R = np_conserve(plan, g, src, r.uniform(0.5, 2.0, plan.shape[1]).astype(F))
        rs = [float(v) for k, v in R.values() if k == 1]
        assert rs and max(rs) <= 4.0
    g = SOURCES["plain"]
    jj, ii = np.meshgrid(np.arange(24), np.arange(40), indexing="ij")
    xlat, xlon = (g.lat0 + (jj + 0.5) / 8.0 * g.dlat).astype(F), (g.lon0 + (ii + 0.5) / 8.0 * g.dlon).astype(F)
    plan, unf = np_plan(xlat, xlon, g)
    assert unf == 0
    out, N, R = np_conserve(plan, g, np.full(g.nx * g.ny, 2.5, F))
    assert_same(out, np.full(out.size, 2.5, F), "flat field")


def test_bindings_regenerate_identically_with_the_conserve_block():
    from tools import gen_abi
    for rel, text in (("include/noahmp_hip.h", gen_abi.c_header()), ("noahmp_amd/fortran/module_sf_noahmpdrv_hip.F90", gen_abi.fortran_shim())):
        assert open(os.path.join(ROOT, rel)).read() == text, rel
    hdr = open(os.path.join(ROOT, "include", "noahmp_hip.h")).read()
    for word in ("#define NOAHMP_HIP_HAS_FORCING_REGRID_CONSERVE 1\n", "noahmp_regrid_conserve_entry", "#define NOAHMP_HIP_ABI_VERSION 1\n",
                 "#define NOAHMP_HIP_ABI_MINOR 3\n", "NOAHMP_REGRID_EDGE_I_FIRST") + tuple(n + "(" for n in NAMES):
        assert word in hdr, word
    f90 = open(os.path.join(ROOT, "noahmp_amd", "fortran", "module_sf_noahmpdrv_hip.F90")).read()
    for name in NAMES:
        assert "bind(C, name='%s')" % name in f90, name
        assert name in abi.EXPORTED_SYMBOLS
    assert "type, bind(C) :: noahmp_regrid_conserve_entry" in f90
    assert "conserve" not in gen_abi.ref_harness()


def test_ctypes_mirror_matches_the_compiled_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "noahmp_hip.h"\nint main(){'
                   'printf("%zu %zu %zu %zu %d %d", sizeof(noahmp_regrid_conserve_entry), offsetof(noahmp_regrid_conserve_entry, dst),'
                   'offsetof(noahmp_regrid_conserve_entry, pattern), offsetof(noahmp_regrid_conserve_entry, fill),'
                   'NOAHMP_REGRID_CONSERVE_MAX_ENTRIES, NOAHMP_REGRID_EDGE_I_FIRST | NOAHMP_REGRID_EDGE_I_LAST | NOAHMP_REGRID_EDGE_J_FIRST |'
                   'NOAHMP_REGRID_EDGE_J_LAST); return 0;}')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    E = abi.RegridConserveEntry
    assert out == [C.sizeof(E), E.dst.offset, E.pattern.offset, E.fill.offset, abi.REGRID_CONSERVE_MAX, sum(abi.REGRID_EDGE.values())]
    assert out[4:] == [8, 15]


def test_library_exports_the_conserve_calls():
    if not os.path.exists(abi.LIB_PATH):
        from noahmp_amd import build as b
        b.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", abi.LIB_PATH]).decode()
    for name in NAMES:
        assert " T " + name in out, name


@pytest.mark.skipif(_flang() is None, reason="no flang")
def test_generated_fortran_types_and_interfaces_compile(tmp_path):
    from tools import gen_abi
    text = "\n".join(["module regrid_conserve_abi_check", "  use iso_c_binding", "  implicit none"] + gen_abi.regrid_f90_types() +
                     gen_abi.regrid_conserve_f90_types() + ["  interface"] + gen_abi.regrid_conserve_f90_interfaces() +
                     ["  end interface", "contains", "  function go(cplan, plan, planes, scratch) result(rc)",
                      "    type(c_ptr), value :: cplan, plan, scratch", "    type(c_ptr), intent(in) :: planes(3)",
                      "    type(noahmp_regrid_source) :: g", "    type(noahmp_regrid_conserve_entry) :: e(1)",
                      "    integer(c_int64_t) :: words, bytes", "    integer(c_int32_t) :: clipped", "    integer(c_int) :: rc",
                      "    g%nx = 464; g%ny = 224; g%lon0 = -124.9375d0; g%lat0 = 25.0625d0",
                      "    g%dlon = 0.125d0; g%dlat = 0.125d0; g%periodic_x = 0",
                      "    rc = noahmp_hip_regrid_conserve_plan_size(64, 8, g, words)",
                      "    rc = noahmp_hip_regrid_conserve_plan(plan, 64, 8, g, planes(3), c_null_ptr, &",
                      "                                         ior(NOAHMP_REGRID_EDGE_I_FIRST, NOAHMP_REGRID_EDGE_J_LAST), cplan, words, clipped, c_null_ptr)",
                      "    rc = noahmp_hip_regrid_conserve_scratch_size(cplan, 1, bytes)",
                      "    e(1)%src = planes(1); e(1)%dst = planes(2); e(1)%pattern = c_null_ptr; e(1)%fill = -1.e33",
                      "    rc = noahmp_hip_forcing_regrid_conserve(cplan, plan, g, c_null_ptr, 512_c_int64_t, 1, e, c_null_ptr, scratch, c_null_ptr)",
                      "  end function go", "end module regrid_conserve_abi_check", ""])
    f = tmp_path / "regrid_conserve_abi_check.f90"
    f.write_text(text)
    subprocess.check_call([_flang(), "-c", str(f), "-o", str(tmp_path / "regrid_conserve_abi_check.o"), "-J", str(tmp_path)], cwd=str(tmp_path))


# ---------------------------------------------------------------------------------------------------------------- GPU
def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()             # a copy: the cached cases are read-only


def gpu_run(engine, plan, ni, nj, g, entries, area=None, dst_index=None, ndst=None, edges=0b1111, poison=7.0, want_sum=True):
    """entries: [(src, pattern or None, fill)] numpy.  Returns (outs [n][ndst] numpy, N plane float64 (poison -7), clipped)."""
    import torch
    n = ni * nj
    ndst = n if ndst is None else ndst
    plan_d = _dev(np.ascontiguousarray(plan).reshape(-1))
    di = _dev(np.asarray(dst_index, np.int32)) if dst_index is not None else None
    cp = engine.regrid_conserve_plan(plan_d, ni, nj, g, area=_dev(area) if area is not None else None, dst_index=di, domain_edges=edges)
    dst = torch.full((len(entries), ndst), poison, dtype=torch.float32, device="cuda")
    ns = torch.full((g.nx * g.ny,), -7.0, dtype=torch.float64, device="cuda") if want_sum else None
    keep = [(_dev(s), dst[f], _dev(p) if p is not None else None, fl) for f, (s, p, fl) in enumerate(entries)]
    torch.cuda.synchronize()
    engine.forcing_regrid_conserve(cp, keep, dst_index=di, group_sum=ns)
    engine.stream_sync()
    return dst.cpu().numpy(), ns.cpu().numpy() if want_sum else None, cp.clipped


def hand_plan(r, g, owners):
    """A hand-made regrid plan in which window cell c is owned by owners[c] (-1: an outside cell): a random base whose four corners lie in
    the source, random weights that partition one."""
    n, nx, ny = len(owners), int(g.nx), int(g.ny)
    plan = np.zeros((6, n), np.int32)
    w = plan[2:].view(F)
    bi, bj = r.integers(0, nx - 1, n), r.integers(0, ny - 1, n)
    plan[0] = bj * nx + bi
    plan[1] = owners
    tx, ty = r.random(n).astype(F), r.random(n).astype(F)
    ux, uy = F(1) - tx, F(1) - ty
    w[0], w[1], w[2], w[3] = ux * uy, tx * uy, ux * ty, tx * ty
    out = np.asarray(owners) < 0
    plan[0, out] = -1
    w[:, out] = 0
    return plan


@functools.lru_cache(maxsize=None)
def boundary_case():
    """Groups of 1, 255, 256, 257 and 513 members, an empty source cell between them and five outside cells, interleaved in one window of
    1287 cells (no multiple of four), with the restated results of eight entries."""
    g = SOURCES["plain"]
    r = np.random.default_rng(21)
    sizes = {3: 1, 8: 255, 9: 256, 17: 257, 30: 513, -1: 5}
    owners = r.permutation(np.concatenate([np.full(k, s) for s, k in sizes.items()]))
    plan = hand_plan(r, g, owners)
    n = owners.size
    area = r.uniform(0.5e6, 1.5e6, n).astype(F)
    entries = []
    for f in range(8):
        src = r.uniform(1e-5, 5e-3, g.nx * g.ny).astype(F) if f % 2 == 0 else nasty(r, g.nx * g.ny)
        if f == 2:
            src[[8, 17]] = (0.0, np.nan)
        pat = None if f % 3 == 0 else r.uniform(0.25, 4.0, n).astype(F)
        if f == 4:
            pat[owners == 9] = 0.0
        entries.append((src, pat, -100.0 - f))
    grp = np_groups(plan, g)
    assert np.array_equal(grp, owners)
    want = [np_conserve(plan, g, s, area, p, fl, grp) for s, p, fl in entries]
    return g, plan, owners, area, entries, want


@pytest.mark.gpu
@pytest.mark.parametrize("nent", [1, 8])
def test_gpu_chunk_boundaries_equal_numpy(engine, nent):
    """Groups of 1, 255, 256, 257, 513 members, an empty source cell and outside cells in one window of 1287 cells, n = 1 and 8 entries:
    outputs and the N_s plane bit for bit; the flux entries keep the budget of every wet group."""
    g, plan, owners, area, entries, want = boundary_case()
    n = owners.size
    outs, ns, clipped = gpu_run(engine, plan, n, 1, g, entries[:nent], area=area)
    for f in range(nent):
        assert_same(outs[f], want[f][0], "entry %d of %d" % (f, nent))
    assert_same64(ns, group_sum_plane(want[0][1], g.nx * g.ny), "N_s")
    assert conservation(outs[0], owners, entries[0][0], area, "boundaries") == 5
    assert clipped == 0


@functools.lru_cache(maxsize=None)
def big_case():
    g = SOURCES["plain"]
    r = np.random.default_rng(22)
    ni, nj = 257, 256
    owners = np.full(ni * nj, 12)
    plan = hand_plan(r, g, owners)
    plan[0] = 12                                                        # inside one source cell: one base
    src = r.uniform(1e-5, 5e-3, g.nx * g.ny).astype(F)
    area = r.uniform(0.5e6, 1.5e6, ni * nj).astype(F)
    return g, ni, nj, plan, owners, src, area, np_conserve(plan, g, src, area, None, -1.0, owners)


@pytest.mark.gpu
def test_gpu_third_level_equals_numpy(engine):
    """A 257 x 256 window inside one source cell: one group of 65 792 members, 257 chunks, so the third level runs."""
    g, ni, nj, plan, owners, src, area, (want, N, R) = big_case()
    outs, ns, clipped = gpu_run(engine, plan, ni, nj, g, [(src, None, -1.0)], area=area, edges=0)
    assert_same(outs[0], want, "one group of %d members" % owners.size)
    assert_same64(ns, group_sum_plane(N, g.nx * g.ny), "N_s")
    assert conservation(outs[0], owners, src, area, "third level") == 1
    assert clipped == 1                                                 # the group reaches every side, none is a domain edge


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SOURCES))
def test_gpu_masked_window_equals_numpy_and_reads_no_dropped_corner(engine, name):
    """The 67 x 5 window of test_regrid with a random mask: outside cells, unfilled cells, empty source cells; NaN behind the mask must not
    reach any output (a corner of weight zero is never read); with and without area and pattern, in one call of four entries."""
    g = SOURCES[name]
    for kind, seed_kind in (("random", "nasty"), ("none", "flux")):
        plan, grp, src, area, pattern, res = value_case(name, kind, seed_kind)
        for ua in (False, True):
            outs, ns, _ = gpu_run(engine, plan, 67, 5, g, [(src, pattern if up else None, -999.0) for up in (False, True)] * 2,
                                  area=area if ua else None)
            for f, up in enumerate((False, True, False, True)):
                assert_same(outs[f], res[ua, up][0], "%s mask %s area %d pattern %d" % (name, kind, ua, up))
            assert_same64(ns, group_sum_plane(res[ua, False][1], g.nx * g.ny), "%s mask %s area %d: N_s" % (name, kind, ua))


@pytest.mark.gpu
def test_gpu_column_order_and_margin_cells(engine):
    """A random permutation as dst_index gives the permuted result of the identity run, outputs and N_s bit for bit; cells with a negative
    dst_index are summed but leave a poisoned destination untouched."""
    g, plan, owners, area, entries, want = boundary_case()
    n = owners.size
    r = np.random.default_rng(23)
    ident, ns0, _ = gpu_run(engine, plan, n, 1, g, entries[:3], area=area)
    perm = r.permutation(n).astype(np.int32)
    outs, ns, _ = gpu_run(engine, plan, n, 1, g, entries[:3], area=area, dst_index=perm)
    for f in range(3):
        back = np.empty(n, F)
        back[:] = outs[f][perm]
        assert_same(back, ident[f], "permuted, entry %d" % f)
    assert_same64(ns, ns0, "N_s, permuted")
    keepers = r.random(n) < 0.5                                         # the written cells, packed; the others are margin
    di = np.full(n, -1, np.int32)
    di[keepers] = r.permutation(int(keepers.sum())).astype(np.int32)
    nd = int(keepers.sum()) + 9
    outs, ns, _ = gpu_run(engine, plan, n, 1, g, entries[:3], area=area, dst_index=di, ndst=nd)
    for f in range(3):
        assert_same(outs[f][di[keepers]], ident[f][keepers], "margin, entry %d" % f)
        untouched = np.ones(nd, bool)
        untouched[di[keepers]] = False
        assert (outs[f][untouched] == 7.0).all()
    assert_same64(ns, ns0, "N_s, margin")


# ---- decomposition: a 96 x 64 model grid over a source whose cells hold 12 x 12 model cells, cut 2 x 2
DEC_NI, DEC_NJ = 96, 64
DEC_SRC = source(10, 8, -100.0, 40.0, 0.12, 0.12)
_dj, _di = np.meshgrid(np.arange(DEC_NJ), np.arange(DEC_NI), indexing="ij")
DEC_LAT = (40.0 + 0.063 + 0.01 * _dj).astype(F)
DEC_LON = (-100.0 + 0.031 + 0.01 * _di).astype(F)           # both cuts of the 2 x 2 decomposition run through source cells


@functools.lru_cache(maxsize=None)
def dec_case():
    r = np.random.default_rng(24)
    g = DEC_SRC
    plan, unf = np_plan(DEC_LAT, DEC_LON, g)
    assert unf == 0
    src = r.uniform(1e-5, 5e-3, g.nx * g.ny).astype(F)
    src[r.random(src.size) < 0.2] = 0.0
    area = r.uniform(0.9e6, 1.1e6, (DEC_NJ, DEC_NI)).astype(F)
    pattern = r.uniform(0.5, 2.0, (DEC_NJ, DEC_NI)).astype(F)
    grp = np_groups(plan, g)
    return plan, grp, src, area, pattern, np_conserve(plan, g, src, area, pattern, -1.0, grp)


def _window_run(engine, j0, j1, i0, i1, margin, edges_all=False):
    """Tile [j0:j1, i0:i1] of the whole grid with `margin` cells around it, clipped to the domain.  Returns (tile result, clipped)."""
    plan, grp, src, area, pattern, _ = dec_case()
    g = DEC_SRC
    wj0, wj1, wi0, wi1 = max(j0 - margin, 0), min(j1 + margin, DEC_NJ), max(i0 - margin, 0), min(i1 + margin, DEC_NI)
    nj, ni = wj1 - wj0, wi1 - wi0
    wplan, unf = engine.regrid_plan(_dev(DEC_LAT[wj0:wj1, wi0:wi1]), _dev(DEC_LON[wj0:wj1, wi0:wi1]), g)
    di = np.full((nj, ni), -1, np.int32)
    tni = i1 - i0
    di[j0 - wj0:j1 - wj0, i0 - wi0:i1 - wi0] = np.arange((j1 - j0) * tni, dtype=np.int32).reshape(j1 - j0, tni)
    edges = 15 if edges_all else ((1 if wi0 == 0 else 0) | (2 if wi1 == DEC_NI else 0) | (4 if wj0 == 0 else 0) | (8 if wj1 == DEC_NJ else 0))
    outs, _, clipped = gpu_run(engine, wplan.cpu().numpy()[:6 * ni * nj].reshape(6, -1), ni, nj, g,
                               [(src, pattern[wj0:wj1, wi0:wi1], -1.0)], area=area[wj0:wj1, wi0:wi1], dst_index=di,
                               ndst=(j1 - j0) * tni, edges=edges, want_sum=False)
    return outs[0].reshape(j1 - j0, tni), clipped


@pytest.mark.gpu
def test_gpu_decomposition_reproduces_the_whole_grid(engine):
    """The whole 96 x 64 grid equals the restatement; each of the 2 x 2 tiles with a margin of 12 cells reports clipped == 0 and reproduces
    the whole grid's bits on its cells; without a margin it reports clipped > 0; with every side flagged as a domain edge 0."""
    plan, grp, src, area, pattern, (want, N, R) = dec_case()
    outs, ns, clipped = gpu_run(engine, plan, DEC_NI, DEC_NJ, DEC_SRC, [(src, pattern, -1.0)], area=area)
    assert clipped == 0
    assert_same(outs[0], want, "whole grid")
    assert_same64(ns, group_sum_plane(N, DEC_SRC.nx * DEC_SRC.ny), "whole grid N_s")
    assert conservation(outs[0], grp, src, area, "whole grid") >= 30
    whole = outs[0].reshape(DEC_NJ, DEC_NI)
    for j0 in (0, 32):
        for i0 in (0, 48):
            tile, clipped = _window_run(engine, j0, j0 + 32, i0, i0 + 48, 12)
            assert clipped == 0
            assert_same(tile, whole[j0:j0 + 32, i0:i0 + 48], "tile at (%d, %d)" % (j0, i0))
            _, clipped = _window_run(engine, j0, j0 + 32, i0, i0 + 48, 0)
            assert clipped > 0
            _, clipped = _window_run(engine, j0, j0 + 32, i0, i0 + 48, 0, edges_all=True)
            assert clipped == 0


@pytest.mark.gpu
def test_gpu_forcing_regrid_window_reproduces_the_whole_grid(engine):
    """ForcingRegrid.set_conserve(window=...) on the last tile of the 2 x 2 cut, with a margin of 12 cells: clipped == 0 and record() gives
    the whole grid's bits on the tile, beside a bilinear plane made by the ordinary launch; without a window clipped > 0."""
    import torch
    from noahmp_amd.regrid import ForcingRegrid
    plan, grp, src, area, pattern, (want, N, R) = dec_case()
    g = DEC_SRC
    j0, i0, m = 32, 48, 12
    rg = ForcingRegrid(engine, _dev(DEC_LAT[j0:, i0:]), _dev(DEC_LON[j0:, i0:]), g)
    rg.set_conserve(area=_dev(area[j0 - m:, i0 - m:]), window=(_dev(DEC_LAT[j0 - m:, i0 - m:]), _dev(DEC_LON[j0 - m:, i0 - m:]), m, m),
                    domain_edges=abi.REGRID_EDGE["i_last"] | abi.REGRID_EDGE["j_last"])
    assert rg.clipped == 0
    rg.set_pattern("pcp", _dev(pattern[j0 - m:, i0 - m:]))
    coarse = {"pcp": _dev(src.reshape(g.ny, g.nx)), "t": _dev(src.reshape(g.ny, g.nx))}
    torch.cuda.synchronize()
    rec = rg.record(coarse, modes={"pcp": "conserve"})
    engine.stream_sync()
    assert_same(rec["pcp"].cpu().numpy(), want.reshape(DEC_NJ, DEC_NI)[j0:, i0:], "the tile through its window")
    assert_same(rec["t"].cpu().numpy(), np_regrid(plan, g, src, BIL, fill=np.nan).reshape(DEC_NJ, DEC_NI)[j0:, i0:], "the bilinear plane beside it")
    rg.set_conserve(area=_dev(area[j0:, i0:]), domain_edges=abi.REGRID_EDGE["i_last"] | abi.REGRID_EDGE["j_last"])
    assert rg.clipped > 0


@pytest.mark.gpu
def test_gpu_refusals_launch_nothing(engine):
    """Every refusal the header lists: -107 / -105 with text, the destinations and the scratch keep their poison."""
    import torch
    g, plan, owners, area, entries, want = boundary_case()
    lib = engine.lib
    n = owners.size
    plan_d = _dev(plan.reshape(-1))
    cp = engine.regrid_conserve_plan(plan_d, n, 1, g, area=_dev(area))
    src = _dev(entries[0][0])
    dst = torch.full((9, n), 7.0, dtype=torch.float32, device="cuda")
    nbytes = engine.regrid_conserve_scratch_bytes(cp, 8)
    scratch = torch.full((nbytes // 8 + 1,), -3.0, dtype=torch.float64, device="cuda")
    e = engine.regrid_conserve_entries([(src, dst[f], None, -1.0) for f in range(8)])
    e9 = (abi.RegridConserveEntry * 9)()
    for f in range(9):
        e9[f].src, e9[f].dst = src.data_ptr(), dst[f].data_ptr()
    torch.cuda.synchronize()

    def call(nent, ent, c=cp.cplan.data_ptr(), p=plan_d.data_ptr(), grid=g, sc=scratch.data_ptr(), ndst=n):
        rc = lib.noahmp_hip_forcing_regrid_conserve(c, p, C.byref(grid) if grid is not None else None, None, ndst, nent, ent, None, sc, None)
        engine.stream_sync()
        return rc, lib.noahmp_hip_last_error().decode()
    assert call(9, e9)[0] == -107 and call(0, e)[0] == -107 and call(-1, e)[0] == -107
    for bad in ("src", "dst"):
        keep = getattr(e[5], bad)
        setattr(e[5], bad, None)
        rc, msg = call(8, e)
        assert rc == -105 and "entry 5" in msg, (bad, rc, msg)
        setattr(e[5], bad, keep)
    assert call(8, e, p=None)[0] == -105 and call(8, None)[0] == -105 and call(8, e, sc=None)[0] == -105 and call(8, e, ndst=-1)[0] == -105
    assert call(8, e, grid=None)[0] == -105
    rc, msg = call(8, e, grid=source(1, 5, 0.0, 0.0, 1.0, 1.0))
    assert rc == -105 and "nx" in msg
    assert call(8, e, grid=source(5, 7, 0.0, 0.0, 1.0, 1.0))[0] == -105                  # not the plan's source grid
    assert call(8, e, c=None)[0] == -105
    moved = cp.cplan.clone()                                                              # a copy of a plan is no plan
    torch.cuda.synchronize()
    rc, msg = call(8, e, c=moved.data_ptr())
    assert rc == -105 and "plan" in msg
    b = C.c_int64(-5)
    assert lib.noahmp_hip_regrid_conserve_scratch_size(moved.data_ptr(), 1, C.byref(b)) == -105 and b.value == -5
    assert lib.noahmp_hip_regrid_conserve_scratch_size(cp.cplan.data_ptr(), 9, C.byref(b)) == -107
    assert (dst.cpu().numpy() == 7.0).all() and (scratch.cpu().numpy() == -3.0).all()
    # the plan call: an area that is not finite and > 0 on a member, a workspace that cannot be
    for bad_value in (0.0, -1.0, np.nan, np.inf):
        a = area.copy()
        a[np.flatnonzero(owners >= 0)[11]] = bad_value
        with pytest.raises(RuntimeError, match="area"):
            engine.regrid_conserve_plan(plan_d, n, 1, g, area=_dev(a))
    a = area.copy()
    a[owners < 0] = np.nan                                                                # a non-member's area is not looked at
    engine.regrid_conserve_plan(plan_d, n, 1, g, area=_dev(a))
    ws = torch.zeros(cp.cplan.numel(), dtype=torch.int32, device="cuda")
    cl = C.c_int32(-5)
    torch.cuda.synchronize()
    for words, edges, rp in ((ws.numel() - 2, 15, plan_d.data_ptr()), (ws.numel(), 16, plan_d.data_ptr()), (ws.numel(), 15, None)):
        rc = lib.noahmp_hip_regrid_conserve_plan(rp, n, 1, C.byref(g), None, None, edges, ws.data_ptr(), words, C.byref(cl), None)
        assert rc == -105 and cl.value == -5 and (ws.cpu().numpy() == 0).all(), (words, edges)
    rc, msg = call(8, e)                                                                  # and the plan still works
    assert rc == 0
    assert_same(dst[7].cpu().numpy(), np_conserve(plan, g, entries[0][0], area, None, -1.0, owners)[0], "after the refusals")


# ---- the chain: coarse records -> ForcingRegrid.record(modes={"pcp": "conserve"}) -> forcing_interpolate_prep -> noahmplsm
@pytest.mark.gpu
def test_gpu_chain_and_budget(engine, tables):
    """Two steps of the regrid chain test's synthetic tile with precipitation through the conserve call (area and a pattern), in tile
    order and after sort_store + follow: RAINBL and every output equal the chain fed with the restated fine records, bit for bit.  Then
    the Regions sum of the regridded precipitation over regions = source cells with weight = area equals p * D_s within 2^-22."""
    import torch
    import test_regrid as tr
    from noahmp_amd.regrid import ForcingRegrid
    from noahmp_amd.history import Regions
    from tools.compare import exact_check
    g = tr.CHAIN_SRC
    r = np.random.default_rng(19)
    names = list(tr.COARSE)
    coarse = [{k: r.uniform(lo, hi, g.nx * g.ny).astype(F).reshape(g.ny, g.nx) for k, (lo, hi) in tr.COARSE.items()} for _ in range(3)]
    for c in coarse:
        c["pcp"].ravel()[r.random(g.nx * g.ny) < 0.3] = 0.0
    area = r.uniform(0.9e6, 1.1e6, (8, 64)).astype(F)
    pattern = r.uniform(0.5, 2.0, (8, 64)).astype(F)
    plan, unf = np_plan(tr.CHAIN_LAT, tr.CHAIN_LON, g)
    assert unf == 0
    grp = np_groups(plan, g)
    fine_pcp = [np_conserve(plan, g, coarse[k]["pcp"].ravel(), area, pattern, np.nan, grp)[0].reshape(8, 64) for k in range(3)]

    def restated(k):
        out = {nm: _dev(np_regrid(plan, g, coarse[k][nm].ravel(), BIL, None, 0.0, np.nan).reshape(8, 64)) for nm in names if nm != "pcp"}
        out["pcp"] = _dev(fine_pcp[k])
        return out
    ref_d = tr._chain(engine, tables, restated)
    ref = ref_d.to_host()
    cd = [{k: _dev(v) for k, v in c.items()} for c in coarse]

    def feed_of(rg):
        class Feed:
            def __call__(self, k):
                return rg.record(cd[k], modes={"pcp": "conserve"})
            follow = staticmethod(rg.follow)
        return Feed()
    rg = ForcingRegrid(engine, _dev(tr.CHAIN_LAT), _dev(tr.CHAIN_LON), g)
    rg.set_conserve(area=_dev(area))
    rg.set_pattern("pcp", _dev(pattern))
    assert rg.clipped == 0 and rg.unfilled == 0
    torch.cuda.synchronize()
    rec = rg.record(cd[2], modes={"pcp": "conserve"})
    engine.stream_sync()
    assert_same(rec["pcp"].cpu().numpy(), fine_pcp[2], "record 2, pcp")
    assert_same(rec["t"].cpu().numpy(), restated(2)["t"].cpu().numpy(), "record 2, t")
    got_d = tr._chain(engine, tables, feed_of(rg))
    got = got_d.to_host()
    ok, lines = exact_check(ref, got)
    assert ok, "\n".join(lines)
    assert_same(np.asarray(got.a["rainbl"]), np.asarray(ref.a["rainbl"]), "RAINBL")

    rg2 = ForcingRegrid(engine, _dev(tr.CHAIN_LAT), _dev(tr.CHAIN_LON), g)
    rg2.set_conserve(area=_dev(area))
    rg2.set_pattern("pcp", _dev(pattern))
    ds = tr._chain(engine, tables, feed_of(rg2), sort=True)
    perm = ds.sort_perm.cpu().numpy()
    hs = ds.to_host()
    for k in ("rainbl", "tsk", "hfx", "tgxy", "smois", "t2mvxy", "runsfxy"):
        x, y = np.asarray(ref.a[k]), np.asarray(hs.a[k])
        if x.ndim == 3:
            x, y = np.moveaxis(x, 1, 0).reshape(x.shape[1], -1), np.moveaxis(y, 1, 0).reshape(y.shape[1], -1)
            assert_same(y, x[:, perm], "sorted chain " + k)
        else:
            assert_same(y.ravel(), x.ravel()[perm], "sorted chain " + k)

    # the budget, summed by the region series: every cell takes part
    d = got_d
    rec = rg.record(cd[1], modes={"pcp": "conserve"})
    engine.stream_sync()
    d.a["rainbl"].copy_(rec["pcp"])
    d.a["xland"].fill_(1.0)
    d.a["xice"].fill_(0.0)
    torch.cuda.synchronize()
    nxny = g.nx * g.ny
    regs = Regions(engine, d, grp.astype(np.int32).reshape(8, 64), nxny, weight=area, nslot=2)
    regs.add("pcp", "rainbl")
    regs.step()
    sums = regs.read()["pcp"][0]
    p = coarse[1]["pcp"].ravel().astype(D)
    checked = 0
    for s in np.unique(grp[grp >= 0]):
        if p[s] > 0:
            want = p[s] * np.sum(area.ravel()[grp == s].astype(D))
            assert abs(sums[s] - want) / want < BOUND, (s, sums[s], want)
            checked += 1
    assert checked >= 5
