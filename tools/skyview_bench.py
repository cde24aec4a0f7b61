"""What the sky-view factor costs: the horizon scan (once per terrain) with 1, 2 and 4 steps in flight, and the per-step radiation call
against the lit shortwave call plus a copy of the bytes it moves beyond that call, in one run.

    python tools/skyview_bench.py [--reps 30] [--window-ms 8] [--out profiles/skyview_bench.md] [--json FILE] [--note FILE] [--build-only]

Shapes: 4608 x 1536 (the config-3 grid) and the 1152 x 768 tile of an 8-rank run, 1 km spacing, nstep 25, ndir 16, the synthetic terrain
with about 2 km relief of tools/shadow_bench.py; the whole grid sits at one sun (mu about 0.5).
Timed, each with two device events around a window of back-to-back calls (sized to --window-ms), ALTERNATING with the order rotated every
repetition:
  (a/nfN) noahmp_hip_skyview from a library built with N = 1, 2, 4 steps in flight (the default library has one of them; the others are
        built next to it from the same objects, --build-only builds them without a GPU);
  (b)   noahmp_hip_forcing_radiation_sky, ZENITH with the three normals and EVERY plane given: svf, lit, albedo, glw, tsurf, emiss
        (36 B of the lit call + 24 B per column);
  (c)   noahmp_hip_forcing_shortwave_lit on the same planes (36 B per column);
  (d)   a device-to-device copy of 12 B per column: 24 B moved, the bytes (b) moves beyond (c) -- what the longwave as a launch of its
        own could at best cost;
  (e)   noahmp_hip_forcing_interpolate_prep on the same shape (156 B per column).
Consecutive calls of a window work on different copies of all their planes (more than twice the 256 MB last-level cache in a round).
Every case is warmed up first; --reps repetitions (at least 20); median, minimum, maximum and inter-quartile range.  The yardstick of
(b) is (c) + (d) of the same run; nothing is enforced.  A process of its own: start it under `timeout -k 10 ...`.

Before anything is timed, the sky-view plane of every library form is compared bit for bit with the numpy restatement
(tests/test_skyview.py) on the 64 x 64 corner block of the full-size result (restated on that block plus nstep cells), and the radiation
call on a 4096-column sample.  Without a GPU it fails (there is nothing to measure on a CPU).
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))          # the restatement lives in the test modules, imported by their bare names
os.environ.setdefault("GPU_PINNED_MIN_XFER_SIZE", "1048576")

from tools.shortwave_bench import _stats, prep_set, CACHE_FLUSH_BYTES, HBM_ACHIEVABLE_GBS  # noqa: E402
from tools.shadow_bench import terrain, latlon, find_suns, NSTEP, DX, MU_MIN, PAR, START, SAMPLE, CORNER  # noqa: E402

F = np.float32
NDIR = 16
FORMS = (1, 2, 4)
SIGMA = 5.67e-8
BYTES = dict(a=8, b=60, c=36, d=24, e=156)
NAMES = dict(b="forcing_radiation_sky, every plane given", c="forcing_shortwave_lit (yardstick)",
             d="device-to-device copy of 12 B per column (24 B moved; yardstick)", e="forcing_interpolate_prep (yardstick)")


def variant(nf, rebuild):
    """The library with nf steps in flight in the horizon scan: noahmp_skyview.hip compiled with the switch, linked with the objects of
    the default library.  A measuring run takes the form that is there and builds only a missing one; --build-only brings a stale one up
    to date (run it after a change to the scan)."""
    from noahmp_amd import build as b
    path = os.path.join(b.CSRC, "variants", "lib_skyview_nf%d.so" % nf)
    if os.path.exists(path) and not rebuild:
        return path
    b.build()
    deps = [os.path.join(b.CSRC, f) for f in ("noahmp_skyview.hip", "nmp_dev_skyview.hpp", "nmp_dev_shadow.hpp")] + [b.LIB]
    if os.path.exists(path) and os.path.getmtime(path) >= max(os.path.getmtime(d) for d in deps):
        return path
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objdir = path + ".obj"
    os.makedirs(objdir, exist_ok=True)
    obj = os.path.join(objdir, "noahmp_skyview.o")
    subprocess.check_call([hipcc] + b.FLAGS + ["-DNMP_SKYVIEW_INFLIGHT=%d" % nf, "-c", os.path.join(b.CSRC, "noahmp_skyview.hip"), "-o", obj])
    objs = [obj if s == "noahmp_skyview.hip" else os.path.join(b.OBJ, s.replace(".hip", ".o")) for s in b._sources()]
    missing = [o for o in objs if not os.path.exists(o)]
    if missing:
        raise SystemExit("skyview_bench: the objects of the default library are not here (%s): build the variants where it was built" % missing[0])
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-o", path, "-lhiprtc", "-ldl", "-lpthread"])
    return path


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--window-ms", type=float, default=8.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "skyview_bench.md"))
    ap.add_argument("--json", default=None)
    ap.add_argument("--note", default=None)
    ap.add_argument("--build-only", action="store_true", help="build the library forms and stop (needs no GPU)")
    a = ap.parse_args()
    a.reps = max(a.reps, 20)
    paths = {nf: variant(nf, a.build_only) for nf in FORMS}
    if a.build_only:
        print("built", paths)
        return
    import torch
    from noahmp_amd import abi
    from noahmp_amd.driver import Engine
    from noahmp_amd.shortwave import sample_times, normal_from_height
    from noahmp_amd.tables import load_tables
    import test_shortwave as ts
    import test_skyview as tsk
    if not torch.cuda.is_available():
        raise SystemExit("skyview_bench: no GPU -- nothing to measure")
    eng = Engine(load_tables("usgs")[0], device=0)
    lib = eng.lib
    libs = {nf: abi.load_library(p) for nf, p in paths.items()}
    stream = torch.cuda.Stream()
    sh = stream.cuda_stream
    r = np.random.default_rng(1)
    gx, gy = Engine.skyview_directions(NDIR)
    results = []
    for cname, ni, nj in (("7 077 888 cells (4608 x 1536)", 4608, 1536), ("884 736-cell tile (1152 x 768)", 1152, 768)):
        ncell = ni * nj
        z = terrain(ni, nj)
        lat, lon = latlon(ni, nj)
        suns, mus = find_suns(float(lat[nj // 2, ni // 2]), float(lon[nj // 2, ni // 2]))
        now = suns["mid"]
        zd, latd, lond = (torch.from_numpy(v).cuda() for v in (z, lat, lon))
        ne, nn, nu, _, _ = normal_from_height(zd, DX, DX)
        rnd = lambda lo, hi: torch.from_numpy(r.uniform(lo, hi, ncell).astype(F)).cuda()      # noqa: E731
        d = dict(lat=latd.reshape(-1), lon=lond.reshape(-1), ne=ne.reshape(-1).contiguous(), nn=nn.reshape(-1).contiguous(), nu=nu.reshape(-1).contiguous(),
                 sw_a=rnd(0.0, 1000.0), mean_a=torch.empty(ncell, dtype=torch.float32, device="cuda"))
        y = dict(albedo=rnd(0.05, 0.9), glw=rnd(150.0, 450.0), tsurf=rnd(230.0, 320.0), emiss=rnd(0.85, 1.0))
        torch.cuda.synchronize()
        eng.cosz_mean(d["lat"], d["lon"], [t[1:] for t in sample_times(START, 10800, 36)], d["mean_a"])
        lit = torch.empty((nj, ni), dtype=torch.float32, device="cuda")
        eng.forcing_shadow(eng.shadow_block(zd, latd, lond, lit, DX, DX, nstep=NSTEP, mu_min=MU_MIN, height_max=float(z.max())), ncell, now)
        eng.stream_sync()
        y["lit"] = lit.reshape(-1)

        def sky_block(zz, dst):
            return eng.skyview_block(zz, dst, DX, DX, nstep=NSTEP, dir_x=gx, dir_y=gy)

        # ---- correctness first: the corner block of the sky-view plane from every form, the radiation call on a sample
        w = CORNER + NSTEP
        idx = np.full((w, w), -1, np.int32)
        idx[:CORNER, :CORNER] = np.arange(CORNER * CORNER, dtype=np.int32).reshape(CORNER, CORNER)
        want = tsk.np_skyview(z[:w, :w], gx, gy, DX, DX, NSTEP, dst_index=idx, ndst=CORNER * CORNER)[0][:CORNER, :CORNER]
        for nf, L in libs.items():
            svf = torch.full((nj, ni), 7.0, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            rc = L.noahmp_hip_skyview(C.byref(sky_block(zd, svf)), ncell, sh)
            if rc:
                raise SystemExit("skyview_bench: noahmp_hip_skyview rc=%d %s" % (rc, L.noahmp_hip_last_error().decode()))
            stream.synchronize()
            got = svf[:CORNER, :CORNER].cpu().numpy()
            if not (got.view(np.uint32) == want.view(np.uint32)).all():
                raise SystemExit("skyview_bench: the sky-view plane of %s, %d in flight differs from the restatement in %d cells"
                                 % (cname, nf, (got != want).sum()))
        y["svf"] = svf.reshape(-1)
        share = float((svf < 1).float().mean().item())
        mean_svf = float(svf.mean().item())
        pick_d = torch.from_numpy(np.sort(r.choice(ncell, SAMPLE, replace=False))).cuda()
        x = {k: d[k][pick_d].cpu().numpy() for k in ("sw_a", "mean_a", "lat", "lon", "ne", "nn", "nu")}
        x["sw_b"] = x["sw_a"]
        ys = {k: v[pick_d].cpu().numpy() for k, v in y.items()}
        out = torch.full((ncell,), 7.0, dtype=torch.float32, device="cuda")

        def sw_block(dd, dst):
            return eng.shortwave_block(dd["sw_a"], dd["lat"], dd["lon"], dst, mean_a=dd["mean_a"], normal=(dd["ne"], dd["nn"], dd["nu"]), mode="zenith",
                                       max_ratio=PAR[0], mu_min=PAR[1], max_terrain_ratio=PAR[2], solar_constant=PAR[3])

        def rad_block(yy):
            return eng.sky_block(yy["svf"], lit=yy["lit"], albedo=yy["albedo"], glw=yy["glw"], tsurf=yy["tsurf"], emiss=yy["emiss"], sigma=SIGMA)
        glw = y["glw"].clone()
        torch.cuda.synchronize()
        eng.forcing_radiation_sky(sw_block(d, out), rad_block(dict(y, glw=glw)), ncell, now)
        eng.stream_sync()
        sw_want, lw_want = tsk.np_radiation_sky(x, ys["svf"], ys["lit"], ys["albedo"], ys["glw"], ys["tsurf"], ys["emiss"], SIGMA, ts.ZENITH, False, True,
                                                ts.np_suntime(now), PAR)
        for name, got, wnt in (("swdown", out[pick_d].cpu().numpy(), sw_want), ("glw", glw[pick_d].cpu().numpy(), lw_want)):
            if not ((got.view(np.uint32) == wnt.view(np.uint32)) | (np.isnan(got) & np.isnan(wnt))).all():
                raise SystemExit("skyview_bench: %s of forcing_radiation_sky of %s differs from the restatement" % (name, cname))

        # ---- the rings of plane copies
        nset_a = -(-CACHE_FLUSH_BYTES // (BYTES["a"] * ncell))
        nset_t = -(-CACHE_FLUSH_BYTES // (BYTES["c"] * ncell))
        nset_d = -(-CACHE_FLUSH_BYTES // (BYTES["d"] * ncell))
        nset_p = -(-CACHE_FLUSH_BYTES // (BYTES["e"] * ncell))
        ring_a = [sky_block(zd.clone(), torch.empty((nj, ni), dtype=torch.float32, device="cuda")) for _ in range(nset_a)]
        sets_t = [({k: v.clone() for k, v in d.items()}, torch.empty(ncell, dtype=torch.float32, device="cuda")) for _ in range(nset_t)]
        ring_t = [sw_block(dd, dst) for dd, dst in sets_t]
        sets_y = [{k: v.clone() for k, v in y.items()} for _ in range(nset_t)]
        ring_y = [rad_block(yy) for yy in sets_y]
        ring_d = [(torch.empty(3 * ncell, dtype=torch.float32, device="cuda"), torch.rand(3 * ncell, dtype=torch.float32, device="cuda")) for _ in range(nset_d)]
        plane = lambda: torch.rand(ncell, dtype=torch.float32, device="cuda")      # noqa: E731
        preps = [prep_set(abi, torch, plane, ncell, ni, nj, d["lat"].clone()) for _ in range(nset_p)]
        jul = C.c_float(0)
        torch.cuda.synchronize()
        turn = dict(a=0, b=0, c=0, d=0, e=0)

        def scan_of(L):
            def go():
                rc = L.noahmp_hip_skyview(C.byref(ring_a[turn["a"] % nset_a]), ncell, sh)
                assert rc == 0, rc
                turn["a"] += 1
            return go

        def radiation():
            q = turn["b"] % nset_t
            turn["b"] += 1
            eng.forcing_radiation_sky(ring_t[q], ring_y[q], ncell, now, stream=sh)

        def lit_call():
            q = turn["c"] % nset_t
            turn["c"] += 1
            eng.forcing_shortwave_lit(ring_t[q], sets_y[q]["lit"], ncell, now, stream=sh)

        def copy():
            dst, src = ring_d[turn["d"] % nset_d]
            turn["d"] += 1
            with torch.cuda.stream(stream):
                dst.copy_(src)

        def prep():
            sa, recs, rain, lon_p = preps[turn["e"] % nset_p][:4]
            turn["e"] += 1
            rc = lib.noahmp_hip_forcing_interpolate_prep(C.byref(sa), C.byref(recs[0]), C.byref(recs[1]), 5400, 10800, rain.data_ptr(),
                                                         lon_p.data_ptr(), now[0], now[1], now[2], now[3], 10.0, 1, C.byref(jul), abi.MEM_DEVICE, sh, None)
            if rc:
                raise RuntimeError("noahmp_hip_forcing_interpolate_prep: %d %s" % (rc, lib.noahmp_hip_last_error().decode()))
        fns = {"a/nf%d" % nf: scan_of(L) for nf, L in libs.items()}
        fns.update(b=radiation, c=lit_call, d=copy, e=prep)

        def window(fn, calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(calls):
                fn()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1) / calls
        keys = list(fns)
        for k in keys:
            window(fns[k], 5)
        calls = {k: max(3, int(a.window_ms / max(window(fns[k], 5), 1e-3)) + 1) for k in keys}
        ms = {k: [] for k in keys}
        for rep in range(a.reps):
            for q in range(len(keys)):
                k = keys[(rep + q) % len(keys)]
                ms[k].append(window(fns[k], calls[k]))
        st = {k: _stats(v) for k, v in ms.items()}
        med = {k: v["median"] for k, v in st.items()}
        results.append(dict(case=cname, ni=ni, nj=nj, ncell=ncell, sun=list(now), mu=mus[0.5], closed_share=share, mean_svf=mean_svf,
                            plane_sets=dict(a=nset_a, t=nset_t, d=nset_d, p=nset_p), stats=st, calls_per_window=calls,
                            yardstick=med["c"] + med["d"], excess=med["b"] - (med["c"] + med["d"]), spread=max(st[k]["iqr"] for k in "bcd")))
        print(json.dumps(results[-1]), flush=True)
        del ring_a, sets_t, ring_t, sets_y, ring_y, ring_d, preps, fns, d, y
        torch.cuda.empty_cache()
    eng.stream_sync()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)
    fmt = lambda s: "%.4f (%.4f .. %.4f, %.4f)" % (s["median"], s["min"], s["max"], s["iqr"])      # noqa: E731
    lines = ["# Sky-view factor: the horizon scan and the radiation call", "",
             "`tools/skyview_bench.py` on one MI355X, one run.  1 km spacing, nstep %d, ndir %d, synthetic terrain with about 2 km relief; the whole" % (NSTEP, NDIR),
             "grid sits at one sun.  Device events around windows of back-to-back calls (>= %g ms), the cases alternating with the order rotated," % a.window_ms,
             "%d repetitions after a warm-up; ms per call: median (min .. max, inter-quartile range).  Consecutive calls of a window work on" % a.reps,
             "different copies of all their planes (more than 512 MB in a round), so nothing is found in the last-level cache.  GB/s = bytes per",
             "column over the median (%.1f TB/s is what a streaming kernel reaches on this chip); the scan is no stream, its column shows the 8 B" % (HBM_ACHIEVABLE_GBS / 1e3),
             "per cell it must move at least.  The sky-view plane of every library form was first compared bit for bit with the numpy restatement",
             "on a %d x %d corner block, the radiation call (SWDOWN and GLW) on a %d-column sample." % (CORNER, CORNER, SAMPLE), ""]
    for x in results:
        lines += ["## %s" % x["case"], "",
                  "Sun (iday, ihour, iminute, isecond) %s, mu at the centre %.3f.  Cells that see less than the hemisphere: %.1f %%; mean factor %.4f." % (
                      tuple(x["sun"]), x["mu"], 100 * x["closed_share"], x["mean_svf"]), "",
                  "| call | ms | GB/s (minimum bytes) | calls per window |", "|---|---|---|---|"]
        for k in x["stats"]:
            nm = NAMES.get(k) or "noahmp_hip_skyview, steps in flight: %s" % k[4:]
            lines.append("| %s | %s | %.0f | %d |" % (nm, fmt(x["stats"][k]), BYTES[k[0]] * x["ncell"] / x["stats"][k]["median"] / 1e6, x["calls_per_window"][k]))
        lines += ["", "Yardstick of the radiation call, (c) + (d): %.4f ms; the call: %.4f ms; difference %+.4f ms; largest inter-quartile range of the three: %.4f ms." % (
            x["yardstick"], x["stats"]["b"]["median"], x["excess"], x["spread"]), ""]
    if a.note and os.path.exists(a.note):
        lines.append(open(a.note).read().rstrip())
        lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
