"""What runoff routing costs: the per-step linear-reservoir call in both forms of its neighbour loads, the once-per-terrain calls, one
pass of the upstream count, and -- in the same run -- a device-to-device copy of the call's bytes, the wind call, the radiation call and
forcing_interpolate_prep, whose bytes per second are the yardsticks.

    python tools/routing_bench.py [--reps 30] [--window-ms 8] [--out profiles/routing_bench.md] [--json FILE] [--note FILE]

Shapes: 4608 x 1536 (the config-3 grid) and the 1152 x 768 tile of an 8-rank run, 1 km spacing, the synthetic terrain with about 2 km
relief of tools/shadow_bench.py; the network is that terrain's (no pit filling: the pits are outlets); release uniform in [0.05, 0.6].
Timed, each with two device events around a window of back-to-back calls (sized to --window-ms), ALTERNATING with the order rotated every
repetition:
  (f) noahmp_hip_route_runoff of the library (loads all eight neighbours and selects), col_index = identity, runoff_b given.  Least bytes
      per cell: inmask 1, col_index 4, area 4, release 4, storage 4 + 4, out_old 4 (every element once), out_new 4, two runoff planes 8: 37;
  (g) the same call of the variant library (-DNMP_ROUTE_LOAD_ALL=0: loads only the neighbours whose bit is set);
  (h) (f) with col_index a random permutation: the runoff of a SORTED store (two 4-byte gathers per cell instead of two streams);
  (a) noahmp_hip_flow_terrain (4 + 1 = 5 B per cell);   (i) noahmp_hip_flow_inmask (1 + 1 = 2 B);
  (j) one pass of noahmp_hip_flow_accumulate (1 + 4 + 4 = 9 B);
  (y) a device-to-device copy that moves the 37 B per cell of (f): 18.5 read and 18.5 written;
  (b) noahmp_hip_forcing_wind with NOAHMP_WIND_TURN (28 B per column);
  (d) noahmp_hip_forcing_radiation_sky, ZENITH with the three normals and every plane given (60 B per column): THE YARDSTICK, by its bytes
      per second;
  (e) noahmp_hip_forcing_interpolate_prep on the same shape (156 B per column).
Consecutive calls of a window work on different copies of all their planes (more than twice the 256 MB last-level cache in a round).
Every case is warmed up first; --reps repetitions (at least 20); median, minimum, maximum and inter-quartile range.  Nothing is enforced.
A process of its own: start it under `timeout -k 10 ...`.

Before anything is timed, dir and inmask are compared byte for byte with the numpy restatement (tests/test_routing.py) on the 64 x 64 corner
block of the full-size result (restated on that block plus 2 cells), and 3 calls of both forms of the routing call in every word on the
1152 x 768 tile.  The passes the upstream count needs on the terrain are then counted with the flag read after every pass, next to the
passes FlowNetwork.upstream_cells makes with its read every 64.  Without a GPU it fails (there is nothing to measure
on a CPU).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))          # the restatement lives in the test modules, imported by their bare names
os.environ.setdefault("GPU_PINNED_MIN_XFER_SIZE", "1048576")

from tools.shortwave_bench import _stats, prep_set, CACHE_FLUSH_BYTES, HBM_ACHIEVABLE_GBS  # noqa: E402
from tools.shadow_bench import terrain, latlon, find_suns, NSTEP, DX, MU_MIN, PAR, START, CORNER  # noqa: E402

F = np.float32
NCURV = 3
SIGMA = 5.67e-8
SCALE = 3.6
BYTES = dict(f=37, g=37, h=37, a=5, i=2, j=9, y=37, b=28, d=60, e=156)
NAMES = dict(f="route_runoff, loads all eight neighbours (the library)", g="route_runoff, loads the set bits' neighbours (variant library)",
             h="route_runoff of the library, col_index a random permutation", a="flow_terrain", i="flow_inmask", j="flow_accumulate, one pass",
             y="device-to-device copy of 37 B per cell", b="forcing_wind with TURN", d="forcing_radiation_sky, every plane given (yardstick)",
             e="forcing_interpolate_prep")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--window-ms", type=float, default=8.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "routing_bench.md"))
    ap.add_argument("--json", default=None)
    ap.add_argument("--note", default=None)
    a = ap.parse_args()
    a.reps = max(a.reps, 20)
    import torch
    from noahmp_amd import abi
    from noahmp_amd.driver import Engine
    from noahmp_amd.routing import FlowNetwork
    from noahmp_amd.shortwave import sample_times, normal_from_height
    from noahmp_amd.tables import load_tables
    import test_routing as trt
    if not torch.cuda.is_available():
        raise SystemExit("routing_bench: no GPU -- nothing to measure")
    if not os.path.exists(trt.LIB_MASKED):
        raise SystemExit("routing_bench: %s missing: __graft_entry__.build() compiles it" % trt.LIB_MASKED)
    T = load_tables("usgs")[0]
    eng = Engine(T, device=0)
    eng_var = Engine(T, device=0, lib_path=trt.LIB_MASKED)
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
        rnd2 = lambda lo, hi: rnd(lo, hi).reshape(nj, ni)                                      # noqa: E731
        new = lambda: torch.empty((nj, ni), dtype=torch.float32, device="cuda")               # noqa: E731

        # ---- correctness first: the corner block of dir and inmask; three calls of both forms on the tile
        net = FlowNetwork(eng, ni, nj)
        net.set_terrain(zd, DX, DX)
        w = CORNER + 2
        dwant = trt.np_flow_dir(z[:w, :w], DX, DX)
        if not (net.dir[:CORNER + 1, :CORNER + 1].cpu().numpy() == dwant[:CORNER + 1, :CORNER + 1]).all():
            raise SystemExit("routing_bench: dir of %s differs from the restatement" % cname)
        if not (net.inmask[:CORNER, :CORNER].cpu().numpy() == trt.np_inmask(dwant[:CORNER + 1, :CORNER + 1])[:CORNER, :CORNER]).all():
            raise SystemExit("routing_bench: inmask of %s differs from the restatement" % cname)
        dir_h = net.dir.cpu().numpy()
        indeg = np.unpackbits(net.inmask.cpu().numpy()).sum() / ncell
        ident = torch.arange(ncell, dtype=torch.int32, device="cuda").reshape(nj, ni)
        permd = torch.from_numpy(r.permutation(ncell).astype(np.int32)).cuda().reshape(nj, ni)
        ops = dict(area=rnd2(0.5e6, 1.5e6), release=rnd2(0.05, 0.6), storage=rnd2(0.0, 5.0e3), out=rnd2(0.0, 2.0e3), runoff_a=rnd(0.0, 2.0e-3),
                   runoff_b=rnd(0.0, 1.0e-3))
        if ncell < 1000000:
            xh = dict(inmask=net.inmask.cpu().numpy(), ncol=ncell, scale=SCALE, **{k: v.cpu().numpy() for k, v in ops.items() if k not in ("storage", "out")})
            for cn, col in (("identity", ident), ("permutation", permd)):
                ws, wo = trt.np_run(dict(xh, col_index=col.cpu().numpy()), ops["storage"].cpu().numpy(), ops["out"].cpu().numpy(), 3)
                for en, e in (("library", eng), ("variant", eng_var)):
                    sd, o = ops["storage"].clone(), [ops["out"].clone(), ops["out"].clone()]
                    torch.cuda.synchronize()
                    for t in range(3):
                        e.route_runoff(e.route_block(net.inmask, col, ops["area"], ops["release"], sd, o[t % 2], o[1 - t % 2], ops["runoff_a"],
                                                     ops["runoff_b"], SCALE), ncell)
                    e.stream_sync()
                    for name, got, wnt in (("storage", sd.cpu().numpy(), ws), ("out", o[1].cpu().numpy(), wo)):
                        if not (got.view(np.uint32) == wnt.view(np.uint32)).all():
                            raise SystemExit("routing_bench: %s of route_runoff (%s, %s) differs from the restatement" % (name, en, cn))
        t0 = time.perf_counter()
        try:
            net.upstream_cells(max_pass=16 * (ni + nj))
            passes = net.passes
        except RuntimeError:
            passes = -1
        upstream_s = time.perf_counter() - t0
        # the count itself: the flag read after EVERY pass (the first pass that changes nothing is the longest flow path's cell count)
        longest = -1
        if passes > 0:
            a0 = torch.ones((nj, ni), dtype=torch.int32, device="cuda")
            a1 = torch.empty_like(a0)
            flag = torch.zeros(1, dtype=torch.int32, device="cuda")
            for n in range(1, passes + 1):
                flag.zero_()
                torch.cuda.synchronize()
                eng.flow_accumulate(net.inmask, a0, a1, flag)
                eng.stream_sync()
                a0, a1 = a1, a0
                if int(flag.item()) == 0:
                    longest = n
                    break
            acc_max = int(a0.max().item())

        # ---- the planes of the wind and radiation calls (tools/wind_bench.py)
        wplanes = [new() for _ in range(3)]
        torch.cuda.synchronize()
        eng.wind_terrain(eng.wind_terrain_block(zd, *wplanes, DX, DX, ncurv=NCURV), ncell)
        eng.stream_sync()
        slope_max = float(torch.sqrt(wplanes[0] * wplanes[0] + wplanes[1] * wplanes[1]).max().item())
        curv_max = float(wplanes[2].abs().max().item())
        u0, v0 = rnd(-8.0, 8.0), rnd(-8.0, 8.0)
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
        nr = nset["f"]
        sets_r = []
        for _ in range(nr):
            s = dict(inmask=net.inmask.clone(), ident=ident.clone(), perm=permd.clone(), area=ops["area"].clone(), release=ops["release"].clone(),
                     storage=ops["storage"].clone(), out=[ops["out"].clone(), ops["out"].clone()], ra=ops["runoff_a"].clone(), rb=ops["runoff_b"].clone())
            sets_r.append(s)

        def route_ring(e, col):
            return [[e.route_block(s["inmask"], s[col], s["area"], s["release"], s["storage"], s["out"][p], s["out"][1 - p], s["ra"], s["rb"], SCALE)
                     for p in (0, 1)] for s in sets_r]
        ring_r = dict(f=route_ring(eng, "ident"), g=route_ring(eng_var, "ident"), h=route_ring(eng, "perm"))
        engs = dict(f=eng, g=eng_var, h=eng)
        ring_a = [eng.flow_terrain_block(zd.clone(), torch.empty((nj, ni), dtype=torch.uint8, device="cuda"), DX, DX) for _ in range(nset["a"])]
        ring_i = [(net.dir.clone(), torch.empty_like(net.inmask)) for _ in range(nset["i"])]
        ring_j = [(net.inmask.clone(), torch.ones((nj, ni), dtype=torch.int32, device="cuda"), torch.ones((nj, ni), dtype=torch.int32, device="cuda"),
                   torch.zeros(1, dtype=torch.int32, device="cuda")) for _ in range(nset["j"])]
        half = (37 * ncell) // 2
        ring_y = [(torch.empty(half, dtype=torch.uint8, device="cuda"), torch.empty(half, dtype=torch.uint8, device="cuda")) for _ in range(nset["y"])]
        sets_w = [dict(u=u0.clone(), v=v0.clone(), p=[p.clone() for p in wplanes]) for _ in range(nset["b"])]
        ring_w = [eng.wind_block(s["u"], s["v"], *s["p"], slope_max, curv_max, turn=True) for s in sets_w]
        sets_t = [({k: v.clone() for k, v in d.items()}, torch.empty(ncell, dtype=torch.float32, device="cuda")) for _ in range(nset["d"])]
        ring_t = [sw_block(dd, dst) for dd, dst in sets_t]
        sets_y = [{k: v.clone() for k, v in y.items()} for _ in range(nset["d"])]
        ring_sky = [rad_block(yy) for yy in sets_y]
        plane = lambda: torch.rand(ncell, dtype=torch.float32, device="cuda")      # noqa: E731
        preps = [prep_set(abi, torch, plane, ncell, ni, nj, d["lat"].clone()) for _ in range(nset["e"])]
        jul = C.c_float(0)
        torch.cuda.synchronize()
        turns = {k: 0 for k in BYTES}

        def route_of(key):
            def go():
                n = turns[key]
                turns[key] += 1
                engs[key].route_runoff(ring_r[key][n % nr][(n // nr) % 2], ncell, stream=sh)      # a set's two out planes swap at its every visit
            return go

        def terrain_call():
            eng.flow_terrain(ring_a[turns["a"] % nset["a"]], stream=sh)
            turns["a"] += 1

        def inmask_call():
            dd, mm = ring_i[turns["i"] % nset["i"]]
            turns["i"] += 1
            eng.flow_inmask(dd, mm, stream=sh)

        def acc_call():
            mm, a0, a1, ch = ring_j[turns["j"] % nset["j"]]
            turns["j"] += 1
            eng.flow_accumulate(mm, a0, a1, ch, stream=sh)

        def copy_call():
            src, dst = ring_y[turns["y"] % nset["y"]]
            turns["y"] += 1
            with torch.cuda.stream(stream):
                dst.copy_(src)

        def wind_call():
            eng.forcing_wind(ring_w[turns["b"] % nset["b"]], ncell, stream=sh)
            turns["b"] += 1

        def radiation():
            q = turns["d"] % nset["d"]
            turns["d"] += 1
            eng.forcing_radiation_sky(ring_t[q], ring_sky[q], ncell, now, stream=sh)

        def prep():
            sa, recs, rain, lon_p = preps[turns["e"] % nset["e"]][:4]
            turns["e"] += 1
            rc = lib.noahmp_hip_forcing_interpolate_prep(C.byref(sa), C.byref(recs[0]), C.byref(recs[1]), 5400, 10800, rain.data_ptr(),
                                                         lon_p.data_ptr(), now[0], now[1], now[2], now[3], 10.0, 1, C.byref(jul), abi.MEM_DEVICE, sh, None)
            if rc:
                raise RuntimeError("noahmp_hip_forcing_interpolate_prep: %d %s" % (rc, lib.noahmp_hip_last_error().decode()))
        fns = dict(f=route_of("f"), g=route_of("g"), h=route_of("h"), a=terrain_call, i=inmask_call, j=acc_call, y=copy_call, b=wind_call,
                   d=radiation, e=prep)

        def restore():
            with torch.cuda.stream(stream):
                for s in sets_w:
                    s["u"].copy_(u0)
                    s["v"].copy_(v0)

        def window(k, calls):
            if k == "b":
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
        results.append(dict(case=cname, ni=ni, nj=nj, ncell=ncell, mean_in_degree=float(indeg), outlets=int((dir_h == 0).sum()), passes=passes, passes_needed=longest,
                            largest_count=acc_max if passes > 0 else -1,
                            upstream_seconds=upstream_s, plane_sets=nset, stats=st, calls_per_window=calls, gbs=gbs,
                            over_radiation={k: gbs[k] / gbs["d"] for k in "fghy"}, over_copy={k: gbs[k] / gbs["y"] for k in "fgh"}))
        print(json.dumps(results[-1]), flush=True)
        del sets_r, ring_r, ring_a, ring_i, ring_j, ring_y, sets_w, ring_w, sets_t, ring_t, sets_y, ring_sky, preps, fns, d, y, net
        torch.cuda.empty_cache()
    eng.stream_sync()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)
    fmt = lambda s: "%.4f (%.4f .. %.4f, %.4f)" % (s["median"], s["min"], s["max"], s["iqr"])      # noqa: E731
    lines = ["# Runoff routing: the linear-reservoir call, the network calls, and their yardsticks", "",
             "`tools/routing_bench.py` on one MI355X, one run.  1 km spacing, synthetic terrain with about 2 km relief, the network that terrain",
             "gives (pits are outlets), release uniform in [0.05, 0.6].  Device events around windows of back-to-back calls (>= %g ms), the cases" % a.window_ms,
             "alternating with the order rotated, %d repetitions after a warm-up; ms per call: median (min .. max, inter-quartile range)." % a.reps,
             "Consecutive calls of a window work on different copies of all their planes (more than 512 MB in a round), so nothing is found in the",
             "last-level cache.  GB/s = the least bytes per cell over the median (%.1f TB/s is what a streaming kernel reaches on this chip)." % (HBM_ACHIEVABLE_GBS / 1e3),
             "dir and inmask were first compared byte for byte with the numpy restatement on a %d x %d corner block, and three calls of both forms" % (CORNER, CORNER),
             "of the routing call in every word on the tile.", ""]
    for x in results:
        lines += ["## %s" % x["case"], "",
                  "Mean in-degree %.3f, %d cells without a direction.  The upstream count needs %d passes (the flag read after every pass: the longest" % (
                      x["mean_in_degree"], x["outlets"], x["passes_needed"]),
                  "flow path has that many cells; the largest count is %d cells); FlowNetwork.upstream_cells, which reads the flag every 64 passes," % x["largest_count"],
                  "made %s (%.4f s wall, launches and the flag reads included)." % (
                      x["passes"] if x["passes"] >= 0 else "more than 16*(ni+nj)", x["upstream_seconds"]), "",
                  "| call | ms | GB/s (least bytes) | calls per window |", "|---|---|---|---|"]
        for k in x["stats"]:
            lines.append("| %s | %s | %.0f | %d |" % (NAMES[k], fmt(x["stats"][k]), x["gbs"][k], x["calls_per_window"][k]))
        lines += ["", "Bytes per second as a share of forcing_radiation_sky's in this run: route_runoff %.2f (library), %.2f (loads the set bits' neighbours), %.2f (permuted"
                  % (x["over_radiation"]["f"], x["over_radiation"]["g"], x["over_radiation"]["h"]),
                  "col_index); the device-to-device copy %.2f.  As a share of the copy's: %.2f, %.2f, %.2f." % (
                      x["over_radiation"]["y"], x["over_copy"]["f"], x["over_copy"]["g"], x["over_copy"]["h"]), ""]
    if a.note and os.path.exists(a.note):
        lines.append(open(a.note).read().rstrip())
        lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
