"""What the terrain-adjusted wind costs: the slope / curvature stencil (once per terrain), the per-record wind call with and without the
turn, and -- in the same run -- the radiation call and forcing_interpolate_prep, whose bytes per second are the yardstick.

    python tools/wind_bench.py [--reps 30] [--window-ms 8] [--out profiles/wind_bench.md] [--json FILE] [--note FILE]

Shapes: 4608 x 1536 (the config-3 grid) and the 1152 x 768 tile of an 8-rank run, 1 km spacing, ncurv 3, the synthetic terrain with about
2 km relief of tools/shadow_bench.py; winds uniform in [-8, 8] m/s; the two maxima are those of the window.
Timed, each with two device events around a window of back-to-back calls (sized to --window-ms), ALTERNATING with the order rotated every
repetition:
  (a) noahmp_hip_wind_terrain, identity dst_index, no rotation planes (4 B read + 12 B written per cell at least: 16 B);
  (b) noahmp_hip_forcing_wind with NOAHMP_WIND_TURN (20 B read + 8 B written per column: 28 B);
  (c) noahmp_hip_forcing_wind without it (28 B);
  (d) noahmp_hip_forcing_radiation_sky, ZENITH with the three normals and every plane given (60 B per column): THE YARDSTICK, by its bytes
      per second;
  (e) noahmp_hip_forcing_interpolate_prep on the same shape (156 B per column).
Consecutive calls of a window work on different copies of all their planes (more than twice the 256 MB last-level cache in a round).  The
wind call works in place, and a column whose wind has decayed to zero is no longer written: the wind planes of (b) and (c) are restored
from a pristine copy before every window, outside the events (a window applies the call to one copy a few dozen times at most: a speed
stays a normal number).  Every case is warmed up first; --reps repetitions (at least 20); median, minimum, maximum and inter-quartile
range.  Nothing is enforced.  A process of its own: start it under `timeout -k 10 ...`.

Before anything is timed, the three terrain planes are compared bit for bit with the numpy restatement (tests/test_wind.py) on the 64 x
64 corner block of the full-size result (restated on that block plus ncurv cells), and the wind call with both flag values on a
4096-column sample.  Without a GPU it fails (there is nothing to measure on a CPU).
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))          # the restatement lives in the test modules, imported by their bare names
os.environ.setdefault("GPU_PINNED_MIN_XFER_SIZE", "1048576")

from tools.shortwave_bench import _stats, prep_set, CACHE_FLUSH_BYTES, HBM_ACHIEVABLE_GBS  # noqa: E402
from tools.shadow_bench import terrain, latlon, find_suns, NSTEP, DX, MU_MIN, PAR, START, SAMPLE, CORNER  # noqa: E402

F = np.float32
NCURV = 3
SIGMA = 5.67e-8
BYTES = dict(a=16, b=28, c=28, d=60, e=156)
NAMES = dict(a="wind_terrain, ncurv %d" % NCURV, b="forcing_wind with TURN", c="forcing_wind without TURN",
             d="forcing_radiation_sky, every plane given (yardstick)", e="forcing_interpolate_prep")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--window-ms", type=float, default=8.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wind_bench.md"))
    ap.add_argument("--json", default=None)
    ap.add_argument("--note", default=None)
    a = ap.parse_args()
    a.reps = max(a.reps, 20)
    import torch
    from noahmp_amd import abi
    from noahmp_amd.driver import Engine
    from noahmp_amd.shortwave import sample_times, normal_from_height
    from noahmp_amd.tables import load_tables
    import test_wind as tw
    if not torch.cuda.is_available():
        raise SystemExit("wind_bench: no GPU -- nothing to measure")
    eng = Engine(load_tables("usgs")[0], device=0)
    lib = eng.lib
    stream = torch.cuda.Stream()
    sh = stream.cuda_stream
    r = np.random.default_rng(1)
    results = []
    for cname, ni, nj in (("7 077 888 cells (4608 x 1536)", 4608, 1536), ("884 736-cell tile (1152 x 768)", 1152, 768)):
        ncell = ni * nj
        z = terrain(ni, nj)
        lat, lon = latlon(ni, nj)
        suns, mus = find_suns(float(lat[nj // 2, ni // 2]), float(lon[nj // 2, ni // 2]))
        now = suns["mid"]
        zd, latd, lond = (torch.from_numpy(v).cuda() for v in (z, lat, lon))
        rnd = lambda lo, hi: torch.from_numpy(r.uniform(lo, hi, ncell).astype(F)).cuda()      # noqa: E731
        new = lambda: torch.empty((nj, ni), dtype=torch.float32, device="cuda")               # noqa: E731

        # ---- correctness first: the corner block of the terrain planes, the wind call on a sample
        planes = [torch.full((nj, ni), 7.0, dtype=torch.float32, device="cuda") for _ in range(3)]
        torch.cuda.synchronize()
        eng.wind_terrain(eng.wind_terrain_block(zd, *planes, DX, DX, ncurv=NCURV), ncell)
        eng.stream_sync()
        w = CORNER + NCURV
        idx = np.full((w, w), -1, np.int32)
        idx[:CORNER, :CORNER] = np.arange(CORNER * CORNER, dtype=np.int32).reshape(CORNER, CORNER)
        want = tw.np_wind_terrain(z[:w, :w], DX, DX, NCURV, dst_index=idx, ndst=CORNER * CORNER)[:3]
        for name, p, wnt in zip(("sx", "sy", "curv"), planes, want):
            got = p[:CORNER, :CORNER].cpu().numpy()
            if not (got.view(np.uint32) == wnt[:CORNER, :CORNER].view(np.uint32)).all():
                raise SystemExit("wind_bench: %s of %s differs from the restatement" % (name, cname))
        slope_max = float(torch.sqrt(planes[0] * planes[0] + planes[1] * planes[1]).max().item())
        curv_max = float(planes[2].abs().max().item())
        u0, v0 = rnd(-8.0, 8.0), rnd(-8.0, 8.0)
        pick_d = torch.from_numpy(np.sort(r.choice(ncell, SAMPLE, replace=False))).cuda()
        xs = {k: t.reshape(-1)[pick_d].cpu().numpy() for k, t in zip(("u", "v", "sx", "sy", "curv"), [u0, v0] + planes)}
        share = {}
        for turn in (True, False):
            u, v = u0.clone(), v0.clone()
            torch.cuda.synchronize()
            eng.forcing_wind(eng.wind_block(u, v, *planes, slope_max, curv_max, turn=turn), ncell)
            eng.stream_sync()
            un, vn, parts = tw.np_forcing_wind(xs["u"], xs["v"], xs["sx"], xs["sy"], xs["curv"], slope_max, curv_max, flags=1 if turn else 0)
            for name, got, wnt in (("u", u[pick_d].cpu().numpy(), un), ("v", v[pick_d].cpu().numpy(), vn)):
                if not ((got.view(np.uint32) == wnt.view(np.uint32)) | (np.isnan(got) & np.isnan(wnt))).all():
                    raise SystemExit("wind_bench: %s of forcing_wind (turn %s) of %s differs from the restatement" % (name, turn, cname))
            share[turn] = float((torch.abs(torch.sqrt(u * u + v * v) / torch.sqrt(u0 * u0 + v0 * v0) - 1) > 0.05).float().mean().item())

        # ---- the planes of the radiation call (tools/skyview_bench.py)
        ne, nn, nu, _, _ = normal_from_height(zd, DX, DX)
        d = dict(lat=latd.reshape(-1), lon=lond.reshape(-1), ne=ne.reshape(-1).contiguous(), nn=nn.reshape(-1).contiguous(), nu=nu.reshape(-1).contiguous(),
                 sw_a=rnd(0.0, 1000.0), mean_a=torch.empty(ncell, dtype=torch.float32, device="cuda"))
        y = dict(albedo=rnd(0.05, 0.9), glw=rnd(150.0, 450.0), tsurf=rnd(230.0, 320.0), emiss=rnd(0.85, 1.0))
        torch.cuda.synchronize()
        eng.cosz_mean(d["lat"], d["lon"], [t[1:] for t in sample_times(START, 10800, 36)], d["mean_a"])
        lit, svf = new(), new()
        eng.forcing_shadow(eng.shadow_block(zd, latd, lond, lit, DX, DX, nstep=NSTEP, mu_min=MU_MIN, height_max=float(z.max())), ncell, now)
        eng.skyview(eng.skyview_block(zd, svf, DX, DX, nstep=NSTEP, ndir=16), ncell)
        eng.stream_sync()
        y["lit"], y["svf"] = lit.reshape(-1), svf.reshape(-1)

        def sw_block(dd, dst):
            return eng.shortwave_block(dd["sw_a"], dd["lat"], dd["lon"], dst, mean_a=dd["mean_a"], normal=(dd["ne"], dd["nn"], dd["nu"]), mode="zenith",
                                       max_ratio=PAR[0], mu_min=PAR[1], max_terrain_ratio=PAR[2], solar_constant=PAR[3])

        def rad_block(yy):
            return eng.sky_block(yy["svf"], lit=yy["lit"], albedo=yy["albedo"], glw=yy["glw"], tsurf=yy["tsurf"], emiss=yy["emiss"], sigma=SIGMA)

        # ---- the rings of plane copies
        nset = {k: -(-CACHE_FLUSH_BYTES // (BYTES[k] * ncell)) for k in BYTES}
        ring_a = [eng.wind_terrain_block(zd.clone(), new(), new(), new(), DX, DX, ncurv=NCURV) for _ in range(nset["a"])]
        sets_w = [dict(u=u0.clone(), v=v0.clone(), p=[p.clone() for p in planes]) for _ in range(nset["b"])]
        ring_w = {turn: [eng.wind_block(s["u"], s["v"], *s["p"], slope_max, curv_max, turn=turn) for s in sets_w] for turn in (True, False)}
        sets_t = [({k: v.clone() for k, v in d.items()}, torch.empty(ncell, dtype=torch.float32, device="cuda")) for _ in range(nset["d"])]
        ring_t = [sw_block(dd, dst) for dd, dst in sets_t]
        sets_y = [{k: v.clone() for k, v in y.items()} for _ in range(nset["d"])]
        ring_y = [rad_block(yy) for yy in sets_y]
        plane = lambda: torch.rand(ncell, dtype=torch.float32, device="cuda")      # noqa: E731
        preps = [prep_set(abi, torch, plane, ncell, ni, nj, d["lat"].clone()) for _ in range(nset["e"])]
        jul = C.c_float(0)
        torch.cuda.synchronize()
        turns = dict(a=0, b=0, c=0, d=0, e=0)

        def terrain_call():
            eng.wind_terrain(ring_a[turns["a"] % nset["a"]], ncell, stream=sh)
            turns["a"] += 1

        def wind_of(key, turn):
            def go():
                eng.forcing_wind(ring_w[turn][turns[key] % nset["b"]], ncell, stream=sh)
                turns[key] += 1
            return go

        def radiation():
            q = turns["d"] % nset["d"]
            turns["d"] += 1
            eng.forcing_radiation_sky(ring_t[q], ring_y[q], ncell, now, stream=sh)

        def prep():
            sa, recs, rain, lon_p = preps[turns["e"] % nset["e"]][:4]
            turns["e"] += 1
            rc = lib.noahmp_hip_forcing_interpolate_prep(C.byref(sa), C.byref(recs[0]), C.byref(recs[1]), 5400, 10800, rain.data_ptr(),
                                                         lon_p.data_ptr(), now[0], now[1], now[2], now[3], 10.0, 1, C.byref(jul), abi.MEM_DEVICE, sh, None)
            if rc:
                raise RuntimeError("noahmp_hip_forcing_interpolate_prep: %d %s" % (rc, lib.noahmp_hip_last_error().decode()))
        fns = dict(a=terrain_call, b=wind_of("b", True), c=wind_of("c", False), d=radiation, e=prep)

        def restore():
            with torch.cuda.stream(stream):
                for s in sets_w:
                    s["u"].copy_(u0)
                    s["v"].copy_(v0)

        def window(k, calls):
            if k in "bc":
                restore()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(calls):
                fns[k]()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1) / calls
        keys = list(fns)
        for k in keys:
            window(k, 5)
        calls = {k: max(3, int(a.window_ms / max(window(k, 5), 1e-3)) + 1) for k in keys}
        ms = {k: [] for k in keys}
        for rep in range(a.reps):
            for q in range(len(keys)):
                k = keys[(rep + q) % len(keys)]
                ms[k].append(window(k, calls[k]))
        st = {k: _stats(v) for k, v in ms.items()}
        gbs = {k: BYTES[k] * ncell / st[k]["median"] / 1e6 for k in keys}
        results.append(dict(case=cname, ni=ni, nj=nj, ncell=ncell, slope_max=slope_max, curv_max=curv_max, changed_share=share[True], plane_sets=nset,
                            stats=st, calls_per_window=calls, gbs=gbs, wind_over_yardstick=dict(b=gbs["b"] / gbs["d"], c=gbs["c"] / gbs["d"])))
        print(json.dumps(results[-1]), flush=True)
        del ring_a, sets_w, ring_w, sets_t, ring_t, sets_y, ring_y, preps, fns, d, y
        torch.cuda.empty_cache()
    eng.stream_sync()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)
    fmt = lambda s: "%.4f (%.4f .. %.4f, %.4f)" % (s["median"], s["min"], s["max"], s["iqr"])      # noqa: E731
    lines = ["# Terrain-adjusted wind: the slope / curvature stencil and the wind call", "",
             "`tools/wind_bench.py` on one MI355X, one run.  1 km spacing, ncurv %d, synthetic terrain with about 2 km relief, winds uniform in" % NCURV,
             "[-8, 8] m/s, the two maxima those of the window.  Device events around windows of back-to-back calls (>= %g ms), the cases" % a.window_ms,
             "alternating with the order rotated, %d repetitions after a warm-up; ms per call: median (min .. max, inter-quartile range)." % a.reps,
             "Consecutive calls of a window work on different copies of all their planes (more than 512 MB in a round), so nothing is found in the",
             "last-level cache; the wind planes are restored before every window, outside the events.  GB/s = the least bytes per column over the",
             "median (%.1f TB/s is what a streaming kernel reaches on this chip).  The terrain planes were first compared bit for bit with the" % (HBM_ACHIEVABLE_GBS / 1e3),
             "numpy restatement on a %d x %d corner block, the wind call with both flag values on a %d-column sample." % (CORNER, CORNER, SAMPLE), ""]
    for x in results:
        lines += ["## %s" % x["case"], "",
                  "slope_max %.4f rad, curv_max %.4g; columns whose speed changes by more than 5 %%: %.1f %%." % (
                      x["slope_max"], x["curv_max"], 100 * x["changed_share"]), "",
                  "| call | ms | GB/s (least bytes) | calls per window |", "|---|---|---|---|"]
        for k in x["stats"]:
            lines.append("| %s | %s | %.0f | %d |" % (NAMES[k], fmt(x["stats"][k]), x["gbs"][k], x["calls_per_window"][k]))
        lines += ["", "forcing_wind reaches %.2f (with TURN) and %.2f (without) of the bytes per second of forcing_radiation_sky in this run." % (
            x["wind_over_yardstick"]["b"], x["wind_over_yardstick"]["c"]), ""]
    if a.note and os.path.exists(a.note):
        lines.append(open(a.note).read().rstrip())
        lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
