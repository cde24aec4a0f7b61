"""The full text of every refusal of the forcing and terrain entry points (noahmp_{shortwave,shadow,skyview,wind,routing,regrid,
regrid_conserve,history,regions}.hip), which the tests of each feature check by substring only: (return code, noahmp_hip_last_error())
of one probe per refusal site equals tests/golden/refusal_text.json.

The fixture is data: `python tests/test_refusal_text.py [out.json]` records it (on a machine with a device both halves, else the host
half; the other half of an existing file is kept).

A site is one place in the source that sets the error text.  Most sites refuse before the engine is initialised and before anything is
read: their probes run without a device on poisoned host arrays, which keep their poison.  The sites behind a successful plan lookup
(noahmp_regions.hip, noahmp_regrid_conserve.hip) need a plan that the device has built: they are marked gpu and work on poisoned device
planes.  Two of those, "regions.plan.bad_id" and "conserve.plan.bad_area", are refusals of the plan call AFTER its kernels have looked at
the map: they are the only probes that launch anything.

No input reaches: (none -- every site of the nine units is probed.)"""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))      # for __main__; the suite has it already

from noahmp_amd import abi                                                # noqa: E402
import test_history as th                                                 # noqa: E402
import test_regions as tg                                                 # noqa: E402
import test_regrid as tr                                                  # noqa: E402
import test_regrid_conserve as tc                                         # noqa: E402
import test_routing as tro                                                # noqa: E402
import test_shadow as tsh                                                 # noqa: E402
import test_shortwave as ts                                               # noqa: E402
import test_skyview as tsv                                                # noqa: E402
import test_wind as tw                                                    # noqa: E402

F = np.float32
POISON = 7.0
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refusal_text.json")
NI, NJ = 5, 3
NCELL = NI * NJ
NAN, INF = float("nan"), float("inf")
BIG = dict(ni=65536, nj=32768)                                            # ni*nj = 2^31


class _Plane:
    """A poisoned host plane with the data_ptr() of a tensor, for the block builders that expect one."""

    def __init__(self, n=NCELL, shape=None):
        self.a = np.full(shape or n, POISON, F)
        self.ptr = self.a.ctypes.data

    def data_ptr(self):
        return self.ptr

    def ok(self):
        return bool((self.a == POISON).all())


def _ref(x):
    return C.byref(x) if x is not None else None


def host_probes(lib):
    """[(id, thunk -> rc)] of the sites that refuse before the engine is initialised, and the planes that must keep their poison."""
    pool = {}

    def P(name, **kw):
        if name not in pool:
            pool[name] = _Plane(**kw)
        return pool[name].ptr
    z, z2 = _Plane(shape=(NJ, NI)), _Plane(shape=(NJ, NI))
    pool["z"], pool["z2"] = z, z2
    out = [_Plane(), _Plane(), _Plane()]
    pool.update(out0=out[0], out1=out[1], out2=out[2])
    now = (abi.SunTime * 1)()
    now[0].iday, now[0].ihour = 171, 18
    t65 = (abi.SunTime * 65)()
    probes = []

    def add(name, fn):
        probes.append((name, fn))

    # ---- noahmp_shortwave.hip
    def swb(**kw):
        b = abi.Shortwave()
        b.sw_a, b.sw_b, b.mean_a, b.xlat, b.lon, b.swdown = (P(k) for k in ("sw_a", "sw_b", "mean_a", "lat", "lon", "swdown"))
        b.normal_e, b.normal_n, b.normal_u = P("ne"), P("nn"), P("nu")
        b.idts, b.idts2 = ts.IDTS, ts.IDTS2
        b.mode, b.max_ratio, b.mu_min, b.max_terrain_ratio, b.solar_constant = ts.ZENITH, 10.0, 0.05, 5.0, 1361.0
        for k, v in kw.items():
            setattr(b, k, v)
        return b

    def sw(b, nc=NCELL, when=now):
        return lambda: lib.noahmp_hip_forcing_shortwave(_ref(b), nc, when, None)
    add("shortwave.block_null", sw(None))
    add("shortwave.now_null", sw(swb(), when=None))
    add("shortwave.mode", sw(swb(mode=2)))
    add("shortwave.columns", sw(swb(), nc=2 ** 31))
    add("shortwave.required", sw(swb(swdown=None)))
    add("shortwave.mean_a", sw(swb(mean_a=None)))
    add("shortwave.normals", sw(swb(normal_n=None)))
    add("shortwave.dates", sw(swb(mode=ts.LINEAR, idts=10801, idts2=10800)))

    def mean(nsample=3, times=t65, lat="lat", nc=NCELL):
        return lambda: lib.noahmp_hip_forcing_cosz_mean(P(lat) if lat else None, P("lon"), nc, nsample, times, P("mean"), None)
    add("cosz_mean.nsample", mean(nsample=65))
    add("cosz_mean.times_null", mean(times=None))
    add("cosz_mean.columns", mean(nc=-1))
    add("cosz_mean.required", mean(lat=None))
    add("shortwave_lit.lit_null", lambda: lib.noahmp_hip_forcing_shortwave_lit(_ref(swb()), None, NCELL, now, None))
    add("shortwave_lit.columns", lambda: lib.noahmp_hip_forcing_shortwave_lit(_ref(swb()), P("lit"), -1, now, None))

    def sky(y, b=None):
        b = b or swb()
        return lambda: lib.noahmp_hip_forcing_radiation_sky(_ref(b), _ref(y), NCELL, now, None)
    add("radiation_sky.sky_null", sky(None))
    add("radiation_sky.svf_null", sky(tsv._sky_block(svf=0)))
    add("radiation_sky.glw_needs_tsurf", sky(tsv._sky_block(svf=P("svf"), glw=P("glw"))))
    add("radiation_sky.mode", sky(tsv._sky_block(svf=P("svf")), swb(mode=-1)))

    # ---- noahmp_shadow.hip
    def shb(**kw):
        b = abi.Shadow()
        b.height, b.xlat, b.lon, b.lit = z.ptr, P("lat"), P("lon"), P("lit")
        b.cosalpha = b.sinalpha = b.dst_index = None
        b.ni, b.nj, b.nstep, b.dx, b.dy, b.mu_min, b.height_max = NI, NJ, tsh.NSTEP_TEST, tsh.DX, tsh.DX, tsh.MU_MIN, 4000.0
        for k, v in kw.items():
            setattr(b, k, v)
        return b

    def sh(b, ndst=NCELL, when=now):
        return lambda: lib.noahmp_hip_forcing_shadow(_ref(b), ndst, when, None)
    add("shadow.block_null", sh(None))
    add("shadow.now_null", sh(shb(), when=None))
    add("shadow.required", sh(shb(lit=None)))
    add("shadow.rotation", sh(shb(cosalpha=P("rot"))))
    add("shadow.window", sh(shb(**BIG)))
    add("shadow.nstep", sh(shb(nstep=abi.SHADOW_MAX_STEPS + 1)))
    add("shadow.spacing", sh(shb(dy=INF)))
    add("shadow.ndst", sh(shb(), ndst=-1))

    # ---- noahmp_skyview.hip
    def svb(**kw):
        b = abi.Skyview()
        b.height, b.svf, b.dir_x, b.dir_y = z.ptr, P("svf"), P("dir_x"), P("dir_y")
        b.dst_index = None
        b.ni, b.nj, b.nstep, b.ndir, b.dx, b.dy = NI, NJ, tsv.NSTEP_TEST, 8, tsv.DX, tsv.DY
        for k, v in kw.items():
            setattr(b, k, v)
        return b

    def sv(b, ndst=NCELL):
        return lambda: lib.noahmp_hip_skyview(_ref(b), ndst, None)
    add("skyview.block_null", sv(None))
    add("skyview.required", sv(svb(dir_y=None)))
    add("skyview.window", sv(svb(ni=-1)))
    add("skyview.nstep", sv(svb(nstep=0)))
    add("skyview.ndir", sv(svb(ndir=65)))
    add("skyview.spacing", sv(svb(dx=NAN)))
    add("skyview.ndst", sv(svb(), ndst=2 ** 31))

    # ---- noahmp_wind.hip
    wout = [p.a for p in out]

    def wt(b, ndst=NCELL):
        return lambda: lib.noahmp_hip_wind_terrain(_ref(b), ndst, None)
    add("wind_terrain.block_null", wt(None))
    add("wind_terrain.required", wt(tw._terrain_block(z.a, wout, curv=None)))
    add("wind_terrain.rotation", wt(tw._terrain_block(z.a, wout, sinalpha=P("rot"))))
    add("wind_terrain.window", wt(tw._terrain_block(z.a, wout, nj=-1)))
    add("wind_terrain.ncurv", wt(tw._terrain_block(z.a, wout, ncurv=65)))
    add("wind_terrain.spacing", wt(tw._terrain_block(z.a, wout, dx=0.0)))
    add("wind_terrain.ndst", wt(tw._terrain_block(z.a, wout), ndst=-1))
    for k in ("u", "v", "sx", "sy", "curv"):
        P(k)
    wplanes = {k: pool[k].a for k in ("u", "v", "sx", "sy", "curv")}

    def fw(b, nc=NCELL):
        return lambda: lib.noahmp_hip_forcing_wind(_ref(b), nc, None)
    add("forcing_wind.block_null", fw(None))
    add("forcing_wind.required", fw(tw._wind_block(wplanes, sy=None)))
    add("forcing_wind.slope_max", fw(tw._wind_block(wplanes, slope_max=0.0)))
    add("forcing_wind.curv_max", fw(tw._wind_block(wplanes, curv_max=INF)))
    add("forcing_wind.ncell", fw(tw._wind_block(wplanes), nc=2 ** 31))

    # ---- noahmp_routing.hip
    def ft(b):
        return lambda: lib.noahmp_hip_flow_terrain(_ref(b), None)
    add("flow_terrain.block_null", ft(None))
    add("flow_terrain.required", ft(tro._ft_block(z.a, z2.a, dir=None)))
    add("flow_terrain.window", ft(tro._ft_block(z.a, z2.a, **BIG)))
    add("flow_terrain.spacing", ft(tro._ft_block(z.a, z2.a, dy=-1.0)))
    add("flow_inmask.required", lambda: lib.noahmp_hip_flow_inmask(None, z2.ptr, NI, NJ, None))
    add("flow_inmask.same_plane", lambda: lib.noahmp_hip_flow_inmask(z.ptr, z.ptr, NI, NJ, None))
    add("flow_inmask.window", lambda: lib.noahmp_hip_flow_inmask(z.ptr, z2.ptr, -1, NJ, None))
    acc = [z.ptr, P("acc0"), P("acc1"), P("changed")]
    add("flow_accumulate.required", lambda: lib.noahmp_hip_flow_accumulate(acc[0], acc[1], acc[2], None, NI, NJ, None))
    add("flow_accumulate.same_plane", lambda: lib.noahmp_hip_flow_accumulate(acc[0], acc[1], acc[1], acc[3], NI, NJ, None))
    add("flow_accumulate.window", lambda: lib.noahmp_hip_flow_accumulate(*acc, NI, -1, None))
    for k in tro.ROUTE_PLANES:
        P("route_" + k)
    rplanes = {k: pool["route_" + k].a for k in tro.ROUTE_PLANES}

    def rr(b, ncol=NCELL):
        return lambda: lib.noahmp_hip_route_runoff(_ref(b), ncol, None)
    add("route_runoff.block_null", rr(None))
    add("route_runoff.required", rr(tro._route_block(rplanes, runoff_a=None)))
    add("route_runoff.same_plane", rr(tro._route_block(rplanes, out_new=pool["route_out_old"].ptr)))
    add("route_runoff.window", rr(tro._route_block(rplanes, **BIG)))
    add("route_runoff.ncol", rr(tro._route_block(rplanes), ncol=-1))

    # ---- noahmp_regrid.hip
    g = tr.SOURCES["plain"]
    w64 = C.c_int64(-5)

    def entries(n=2, **kw):
        e = (abi.RegridEntry * max(n, 1))()
        for f in range(n):
            e[f].src, e[f].dst, e[f].mode = P("coarse"), P("fine%d" % f), f % 2
        for k, v in kw.items():
            setattr(e[1], k, v)
        return e

    def rg(plan="plan", nc=NCELL, grid=g, n=2, e=entries()):
        return lambda: lib.noahmp_hip_forcing_regrid(P(plan) if plan else None, nc, _ref(grid), n, e, None)
    add("regrid.entries_n", rg(n=33))
    add("regrid.source_null", rg(grid=None))
    add("regrid.source_size", rg(grid=tr.source(1, 5, 0.0, 0.0, 1.0, 1.0)))
    add("regrid.columns", rg(nc=-1))
    add("regrid.plan_null", rg(plan=None))
    add("regrid.entries_null", rg(e=None))
    add("regrid.entry_mode", rg(e=entries(mode=2)))
    add("regrid.entry_plane", rg(e=entries(dst=None)))

    def metb(**kw):
        m = abi.RegridMet()
        for k in ("src_t", "src_p", "src_q", "src_lw", "dst_t", "dst_p", "dst_q", "dst_lw", "dz"):
            setattr(m, k, P("met_" + k))
        m.lapse, m.fill = -0.0065, -999.0
        for k, v in kw.items():
            setattr(m, k, v)
        return m

    def rm(m, n=0):
        return lambda: lib.noahmp_hip_forcing_regrid_met(P("plan"), NCELL, _ref(g), _ref(m), n, None, None)
    add("regrid_met.met_null", rm(None))
    add("regrid_met.met_required", rm(metb(dz=None)))
    add("regrid_met.met_lw", rm(metb(dst_lw=None)))
    add("regrid_met.entries_null", rm(metb(), n=1))
    add("regrid_plan_size.refused", lambda: lib.noahmp_hip_regrid_plan_size(NI, NJ, None))

    def pl(grid=g, radius=2, ni=NI, nj=NJ, plan="plan", words=6 * NCELL + 1):
        return lambda: lib.noahmp_hip_regrid_plan_latlon(P("lat"), P("lon"), ni, nj, _ref(grid), None, radius, P(plan) if plan else None, words,
                                                         None, None)
    add("regrid_plan.source_null", pl(grid=None))
    add("regrid_plan.spacing", pl(grid=tr.source(7, 5, -100.0, 30.0, 0.0, 0.25)))
    add("regrid_plan.radius", pl(radius=17))
    add("regrid_plan.cells", pl(ni=-1))
    add("regrid_plan.required", pl(plan=None))
    add("regrid_plan.words", pl(words=6 * NCELL))

    # ---- noahmp_regrid_conserve.hip
    def cps(ni=NI, nj=NJ, grid=g, words=w64):
        return lambda: lib.noahmp_hip_regrid_conserve_plan_size(ni, nj, _ref(grid), _ref(words))
    add("conserve_plan_size.words_null", cps(words=None))
    add("conserve_plan_size.source_null", cps(grid=None))
    add("conserve_plan_size.source_size", cps(grid=tr.source(4097, 4096, 0.0, 0.0, 1.0, 1.0)))
    add("conserve_plan_size.window", cps(ni=4097, nj=4096))
    P("cplan", n=4096)

    def cpl(rp="plan", cplan=None, edges=15, words=1 << 40):
        cplan = pool["cplan"].ptr if cplan is None else cplan
        return lambda: lib.noahmp_hip_regrid_conserve_plan(P(rp) if rp else None, NI, NJ, _ref(g), None, None, edges, cplan, words, None, None)
    add("conserve_plan.required", cpl(rp=None))
    add("conserve_plan.aligned", cpl(cplan=pool["cplan"].ptr + 4))
    add("conserve_plan.edges", cpl(edges=16))
    add("conserve_plan.words", cpl(words=3))
    add("conserve_scratch_size.no_plan", lambda: lib.noahmp_hip_regrid_conserve_scratch_size(pool["cplan"].ptr, 1, _ref(w64)))

    def centries(n=2, **kw):
        e = (abi.RegridConserveEntry * max(n, 1))()
        for f in range(n):
            e[f].src, e[f].dst = P("coarse"), P("fine%d" % f)
        for k, v in kw.items():
            setattr(e[1], k, v)
        return e

    def cv(n=2, grid=g, rp="plan", e=centries(), ndst=NCELL):
        return lambda: lib.noahmp_hip_forcing_regrid_conserve(pool["cplan"].ptr, P(rp) if rp else None, _ref(grid), None, ndst, n, e, None,
                                                              P("scratch"), None)
    add("conserve.entries_n", cv(n=0))
    add("conserve.source_size", cv(grid=tr.source(5, 1, 0.0, 0.0, 1.0, 1.0)))
    add("conserve.regrid_plan_null", cv(rp=None))
    add("conserve.entries_null", cv(e=None))
    add("conserve.entry_plane", cv(e=centries(src=None)))
    add("conserve.ndst", cv(ndst=-1))
    add("conserve.no_plan", cv())

    # ---- noahmp_history.hip
    xl, xi = _Plane(), _Plane()
    pool["xland"], pool["xice"] = xl, xi
    blk = th._block(NI, NJ, xl, xi)

    def hentries(n=2, **kw):
        e = (abi.HistoryEntry * max(n, 1))()
        for f in range(n):
            e[f].src, e[f].acc, e[f].nlev, e[f].op, e[f].scale = P("hsrc%d" % f), P("hacc%d" % f), 1, f, 1.0
        for k, v in kw.items():
            setattr(e[1], k, v)
        return e

    def hs(n=2, e=hentries(), p=None, a=blk):
        return lambda: lib.noahmp_hip_history_step(n, e, _ref(p), _ref(a), P("count"), None)
    add("history_step.entries_n", hs(n=33))
    add("history_step.entries_null", hs(e=None))
    add("history_step.entry_op", hs(e=hentries(op=5)))
    add("history_step.entry_acc", hs(e=hentries(acc=None)))
    add("history_step.entry_levels", hs(e=hentries(nlev=0)))
    add("history_step.entry_src", hs(e=hentries(src=None)))
    add("history_step.block_null", hs(a=None))
    halo = th._block(NI, NJ, xl, xi)
    halo.its = 2
    add("history_step.block_tile", hs(a=halo))
    inside_out = th._block(NI, NJ, xl, xi)
    inside_out.ims = inside_out.its = 5
    inside_out.ime = inside_out.ite = 3
    add("history_step.columns", hs(a=inside_out))
    fields = (C.c_void_p * 2)(P("hsrc0"), None)

    def probes_(**kw):
        p = abi.HistoryProbes()
        p.npoint, p.column, p.nfield, p.field, p.ring, p.nslot, p.slot = 4, P("column"), 2, fields, P("ring"), 2, 0
        for k, v in kw.items():
            setattr(p, k, v)
        return p
    add("history_step.probe_points", hs(p=probes_(npoint=4097)))
    add("history_step.probe_fields", hs(p=probes_(nfield=33)))
    add("history_step.probe_required", hs(p=probes_(ring=None)))
    add("history_step.probe_slots", hs(p=probes_(nslot=0)))
    add("history_step.probe_field_null", hs(p=probes_()))
    dst = (C.c_void_p * 2)(P("hdst0"), P("hdst1"))
    mean_flags = (C.c_uint32 * 2)(0, 1)

    def hf(n=2, e=hentries(), flags=mean_flags, count="count", ni=NI, nj=NJ):
        return lambda: lib.noahmp_hip_history_finish(n, e, dst, flags, P(count) if count else None, None, None, 16, -1.0, ni, nj, None)
    add("history_finish.entries_n", hf(n=-1))
    add("history_finish.flags_null", hf(flags=None))
    add("history_finish.columns", hf(**BIG))
    add("history_finish.mean_count", hf(count=None))

    # ---- noahmp_regions.hip
    def rps(ni=NI, nj=NJ, nregion=3, words=w64):
        return lambda: lib.noahmp_hip_region_plan_size(ni, nj, nregion, _ref(words))
    add("region_plan_size.words_null", rps(words=None))
    add("region_plan_size.cells", rps(ni=4097, nj=4096))
    add("region_plan_size.regions", rps(nregion=-1))

    def rpl(region="region", plan=None, words=1 << 40, nregion=3):
        plan = pool["cplan"].ptr if plan is None else plan
        return lambda: lib.noahmp_hip_region_plan(P(region) if region else None, None, NI, NJ, nregion, None, plan, words, None)
    add("region_plan.size", rpl(nregion=(1 << 24) + 1))
    add("region_plan.required", rpl(region=None))
    add("region_plan.aligned", rpl(plan=pool["cplan"].ptr + 4))
    add("region_plan.words", rpl(words=3))
    add("region_plan_follow.no_plan", lambda: lib.noahmp_hip_region_plan_follow(pool["cplan"].ptr, None, None))
    add("region_scratch_size.no_plan", lambda: lib.noahmp_hip_region_scratch_size(None, 1, _ref(w64)))

    def rentries(n=2, **kw):
        e = (abi.RegionEntry * max(n, 1))()
        for f in range(n):
            e[f].src, e[f].nlev, e[f].lev, e[f].op = P("hsrc%d" % f), 1, 0, f
        for k, v in kw.items():
            setattr(e[1], k, v)
        return e

    def rs(n=2, e=rentries()):
        return lambda: lib.noahmp_hip_region_step(pool["cplan"].ptr, n, e, _ref(blk), P("series"), 2, 0, None, P("scratch"), None)
    add("region_step.entries_n", rs(n=33))
    add("region_step.entries_null", rs(e=None))
    add("region_step.entry_op", rs(e=rentries(op=3)))
    add("region_step.entry_level", rs(e=rentries(nlev=2, lev=2)))
    add("region_step.no_plan", rs())
    return probes, pool, w64


def device_probes(engine):
    """[(id, thunk -> rc)] of the sites behind a plan that the device has built, and a check that the planes kept their poison."""
    import torch
    lib = engine.lib
    probes = []

    def add(name, fn):
        probes.append((name, fn))
    # ---- noahmp_regions.hip
    ni, nj, nregion = 64, 2, 3
    ncol = ni * nj
    region = (np.arange(ncol) % nregion).astype(np.int32)
    x = np.full(ncol, 2.0, F)
    c = tg._Case(engine, ni, nj, region, nregion, None, np.ones(ncol, F), np.zeros(ncol, F), [(x, "sum", 1, 0)])
    series = tg._series(2, 1, nregion, fill=9.0)
    c.step(series, 0)                                                   # sizes the scratch
    series.fill_(9.0)
    bad = region.copy()
    bad[77] = nregion
    bad_d = torch.from_numpy(bad.reshape(nj, ni)).cuda()
    plan2 = torch.zeros_like(c.plan)
    torch.cuda.synchronize()
    blk = tg._block(ni, nj, c.xland, c.xice)
    b64 = C.c_int64(-5)

    def rs(block=blk, ring=series, scratch=c.scratch):
        return lambda: lib.noahmp_hip_region_step(c.plan.data_ptr(), 1, c.entries, _ref(block), ring.data_ptr() if ring is not None else None,
                                                  2, 0, None, scratch.data_ptr() if scratch is not None else None, None)
    add("region_plan.bad_id", lambda: lib.noahmp_hip_region_plan(bad_d.data_ptr(), None, ni, nj, nregion, None, plan2.data_ptr(), c.words, None))
    add("region_scratch_size.refused", lambda: lib.noahmp_hip_region_scratch_size(c.plan.data_ptr(), 33, _ref(b64)))
    add("region_step.block_null", rs(block=None))
    halo = tg._block(ni, nj, c.xland, c.xice)
    halo.its = 2
    add("region_step.block_tile", rs(block=halo))
    add("region_step.block_size", rs(block=tg._block(ni // 2, nj * 2, c.xland, c.xice)))
    add("region_step.series", rs(ring=None))
    add("region_step.scratch", rs(scratch=None))
    # ---- noahmp_regrid_conserve.hip
    g, plan, owners, area, entries, want = tc.boundary_case()
    n = owners.size
    plan_d = tc._dev(plan.reshape(-1))
    cp = engine.regrid_conserve_plan(plan_d, n, 1, g, area=tc._dev(area))
    src = tc._dev(entries[0][0])
    dst = torch.full((2, n), POISON, dtype=torch.float32, device="cuda")
    scratch = torch.full((engine.regrid_conserve_scratch_bytes(cp, 2) // 8 + 1,), -3.0, dtype=torch.float64, device="cuda")
    e = engine.regrid_conserve_entries([(src, dst[f], None, -1.0) for f in range(2)])
    a = area.copy()
    a[np.flatnonzero(owners >= 0)[11]] = 0.0
    bad_area = tc._dev(a)
    ws = torch.zeros(cp.cplan.numel(), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def cv(grid=g, sc=scratch):
        return lambda: lib.noahmp_hip_forcing_regrid_conserve(cp.cplan.data_ptr(), plan_d.data_ptr(), _ref(grid), None, n, 2, e, None,
                                                              sc.data_ptr() if sc is not None else None, None)
    add("conserve_plan.bad_area", lambda: lib.noahmp_hip_regrid_conserve_plan(plan_d.data_ptr(), n, 1, _ref(g), bad_area.data_ptr(), None, 15,
                                                                                ws.data_ptr(), ws.numel(), None, None))
    add("conserve_scratch_size.entries_n", lambda: lib.noahmp_hip_regrid_conserve_scratch_size(cp.cplan.data_ptr(), 9, _ref(b64)))
    add("conserve_scratch_size.bytes_null", lambda: lib.noahmp_hip_regrid_conserve_scratch_size(cp.cplan.data_ptr(), 1, None))
    add("conserve.source_differs", cv(grid=tr.source(5, 7, 0.0, 0.0, 1.0, 1.0)))
    add("conserve.scratch", cv(sc=None))

    def poison_kept():
        engine.stream_sync()
        torch.cuda.synchronize()
        return bool((series == 9.0).all() and (dst == POISON).all() and (scratch == -3.0).all() and b64.value == -5)
    return probes, poison_kept


def run(lib, probes):
    got = {}
    for name, fn in probes:
        assert name not in got, name
        rc = fn()
        got[name] = [int(rc), lib.noahmp_hip_last_error().decode()]
    return got


def _fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def test_host_refusals_have_their_text_and_touch_nothing():
    lib = abi.load_library()
    probes, pool, w64 = host_probes(lib)
    got = run(lib, probes)
    assert got == _fixture()["host"]
    assert all(rc < 0 and text for rc, text in got.values())
    assert all(p.ok() for p in pool.values()) and w64.value == -5


@pytest.mark.gpu
def test_gpu_refusals_behind_a_plan_have_their_text(engine):
    probes, poison_kept = device_probes(engine)
    got = run(engine.lib, probes)
    assert got == _fixture()["device"]
    assert all(rc < 0 and text for rc, text in got.values())
    assert poison_kept()


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    fixture = _fixture() if os.path.exists(FIXTURE) else {}
    lib_ = abi.load_library()
    fixture["host"] = run(lib_, host_probes(lib_)[0])
    import torch as _torch
    if _torch.cuda.is_available():
        from noahmp_amd.driver import Engine
        from noahmp_amd.tables import load_tables
        eng = Engine(load_tables("usgs")[0], device=0)
        fixture["device"] = run(eng.lib, device_probes(eng)[0])
    with open(path, "w") as f:
        json.dump(fixture, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%s: %d host, %d device refusals" % (path, len(fixture["host"]), len(fixture.get("device", {}))))
