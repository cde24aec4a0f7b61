"""What the forcing regrid replaces and what it costs: fine planes over PCIe against coarse planes plus one regrid launch, in one run.

    python tools/regrid_bench.py [--reps 30] [--window-ms 8] [--out profiles/regrid_bench.md] [--json FILE] [--note FILE]

Shapes: the config-3 grid 4608 x 1536 fed from a 464 x 224 source at 0.125 degrees (NLDAS-2 like); the config-5 grid 3600 x 1800 fed
from a periodic 1440 x 721 source at 0.25 degrees with a 35 % ocean mask; the 1152 x 768 tile of an 8-rank run against the config-3
source.  The tool makes its own XLAT / XLONG.  Eight planes per record, precipitation taken from the nearest cell, temperature with a
lapse-rate adjustment plane.

  (a) what the feature replaces: eight fine float32 planes from page-locked host memory to the device with the engine's own copy call
      (noahmp_hip_memcpy, which returns when the bytes have arrived);
  (b) what it costs: eight coarse planes uploaded the same way, then one noahmp_hip_forcing_regrid of 8 entries and a wait for it.
  (c) the same with the elevation adjustment: the coarse upload, then one noahmp_hip_forcing_regrid_met -- t, p, q, lw as the met group
      (dz = the adjust plane of (b)) plus u, v, sw, pcp as four ordinary entries: the same eight planes -- and a wait for it.
(a), (b) and (c) are host wall-clock times of the whole sequence, ALTERNATING repetition by repetition with the order rotated every time.
The launches alone are timed with two device events around a window of back-to-back calls (sized to --window-ms), alternating:
  (i)   noahmp_hip_forcing_regrid, 8 entries, t with the adjust plane (the launch of (b));
  (ii)  noahmp_hip_forcing_regrid_met, the met group + 4 entries (the launch of (c)); it runs one column per thread;
  (iii) ONE hipMemcpyAsync device-to-device whose bytes read plus written are the bytes (i) and (ii) both move: 24 B of plan + 4 B of
        adjust / dz + 4 B per plane and column; the source reads stay in cache and are not counted.
Every case is warmed up first; --reps repetitions (at least 20); median, minimum, maximum and inter-quartile range.  No pass mark is
set on (ii)/(i) or (ii)/(iii): they are reported.  A process of its own: start it under `timeout -k 10 ...`.

Before a case is timed, the plan and all eight destination planes of (b) and of (c) are compared bit for bit with the
numpy restatement of the contract (tests/test_regrid.py: np_plan, np_regrid; tests/test_regrid_met.py: np_met with glibc's expf / powf)
on a 4096-column sample of the full-size result, and the unfilled count with a count of the plan's negative bases.  Without a GPU it
fails (there is nothing to measure on a CPU).

The markdown it writes also takes notes (--note FILE: text appended as it is, e.g. bench.py's headline before and after the change).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))          # the restatements live in the test modules, imported by their bare names
os.environ.setdefault("GPU_PINNED_MIN_XFER_SIZE", "1048576")

F = np.float32
HBM_ACHIEVABLE_GBS = 6300.0          # what a streaming kernel reaches on this chip (the microarchitecture notes' figure)
HIP_MEMCPY_D2D = 3
NAMES = ("t", "q", "u", "v", "p", "lw", "sw", "pcp")
MET = ("t", "p", "q", "lw")
RANGES = dict(t=(250.0, 310.0), q=(1e-3, 2e-2), u=(-10.0, 10.0), v=(-10.0, 10.0), p=(6.0e4, 1.05e5), lw=(150.0, 450.0), sw=(0.0, 900.0),
              pcp=(0.0, 1e-3))
SAMPLE = 4096


def cases():
    """name, ni, nj, (nx, ny, lon0, lat0, dlon, dlat, periodic), ocean fraction, xlat / xlon makers"""
    def conus(ni, nj, i0=0, j0=0, gi=4608, gj=1536):
        j, i = np.meshgrid(np.arange(j0, j0 + nj), np.arange(i0, i0 + ni), indexing="ij")
        lat = 25.2 + (52.5 - 25.2) * j / (gj - 1) + 0.3 * np.sin(i / gi * 3.0)         # a gently curved 1 km grid inside the source
        lon = -124.7 + (-67.4 + 124.7) * i / (gi - 1) + 0.2 * np.sin(j / gj * 2.0)
        return lat.astype(F), lon.astype(F)

    def globe(ni, nj):
        j, i = np.meshgrid(np.arange(nj), np.arange(ni), indexing="ij")
        return (-89.95 + 0.1 * j).astype(F), (-179.95 + 0.1 * i).astype(F)               # longitudes -180 .. 180 against a 0 .. 360 source
    nldas = (464, 224, -124.9375, 25.0625, 0.125, 0.125, False)
    return [("config 3 grid from 0.125 deg", 4608, 1536, nldas, 0.0, lambda: conus(4608, 1536)),
            ("config 5 grid from periodic 0.25 deg, 35 % ocean", 3600, 1800, (1440, 721, 0.0, 90.0, 0.25, -0.25, True), 0.35, lambda: globe(3600, 1800)),
            ("8-rank tile from 0.125 deg", 1152, 768, nldas, 0.0, lambda: conus(1152, 768, i0=1152, j0=768))]


def _hip_runtime():
    """The HIP runtime this process already runs on (torch's copy): a second one must not be loaded."""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    raise RuntimeError("no HIP runtime mapped into this process")


def _stats(ms):
    q = statistics.quantiles(ms, n=4)
    return dict(median=statistics.median(ms), min=min(ms), max=max(ms), iqr=q[2] - q[0], n=len(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--window-ms", type=float, default=8.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "regrid_bench.md"))
    ap.add_argument("--json", default=None)
    ap.add_argument("--note", default=None)
    a = ap.parse_args()
    a.reps = max(a.reps, 20)
    import torch
    from noahmp_amd.driver import Engine
    from noahmp_amd.tables import load_tables
    from test_regrid import np_plan, np_regrid, BIL, NEAR
    from test_regrid_met import np_met, filled
    if not torch.cuda.is_available():
        raise SystemExit("regrid_bench: no GPU -- nothing to measure")
    eng = Engine(load_tables("usgs")[0], device=0)
    lib = eng.lib
    hip = _hip_runtime()
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    stream = torch.cuda.Stream()
    sh = stream.cuda_stream
    r = np.random.default_rng(1)
    results = []
    for cname, ni, nj, grid, ocean, make in cases():
        ncell = ni * nj
        g = Engine.regrid_source(*grid)
        nxny = g.nx * g.ny
        xlat, xlon = make()
        valid = (r.random(nxny) >= ocean).astype(np.uint8) if ocean else None
        xlat_d, xlon_d = torch.from_numpy(xlat).cuda(), torch.from_numpy(xlon).cuda()
        valid_d = torch.from_numpy(valid).cuda() if valid is not None else None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        plan, unfilled = eng.regrid_plan(xlat_d, xlon_d, g, valid=valid_d, search_radius=4)
        plan_ms = (time.perf_counter() - t0) * 1e3
        coarse_h = [torch.from_numpy(np.where(valid.astype(bool), x, np.nan).astype(F) if valid is not None else x).pin_memory()
                    for x in (r.uniform(*RANGES[nm], nxny).astype(F) for nm in NAMES)]              # ocean cells hold NaN
        coarse_d = [torch.empty(nxny, dtype=torch.float32, device="cuda") for _ in NAMES]
        fine_h = [torch.empty(ncell, dtype=torch.float32).pin_memory() for _ in NAMES]
        for t in fine_h:
            t.uniform_(250.0, 310.0)
        fine_d = [torch.empty(ncell, dtype=torch.float32, device="cuda") for _ in NAMES]
        adjust = (torch.rand(ncell, device="cuda") * 1000.0 - 500.0).contiguous()
        modes = [NEAR if nm == "pcp" else BIL for nm in NAMES]
        adjs = [adjust if nm == "t" else None for nm in NAMES]
        ents = eng.regrid_entries([(coarse_d[f], fine_d[f], modes[f], adjs[f], -0.0065, -1.0e33) for f in range(len(NAMES))])
        # the met call: the same eight planes
        ix = {nm: f for f, nm in enumerate(NAMES)}
        dst_m = {nm: torch.empty(ncell, dtype=torch.float32, device="cuda") for nm in NAMES}
        met = eng.regrid_met(*[coarse_d[ix[nm]] for nm in ("t", "p", "q")], *[dst_m[nm] for nm in ("t", "p", "q")], adjust,
                             src_lw=coarse_d[ix["lw"]], dst_lw=dst_m["lw"], lapse=-0.0065, fill=-1.0e33)
        rest = eng.regrid_entries([(coarse_d[ix[nm]], dst_m[nm], modes[ix[nm]], None, 0.0, -1.0e33) for nm in NAMES if nm not in MET])
        torch.cuda.synchronize()

        def upload(dst, src):
            for d, s in zip(dst, src):
                rc = lib.noahmp_hip_memcpy(d.data_ptr(), s.data_ptr(), s.numel() * 4, 0)
                if rc:
                    raise RuntimeError("noahmp_hip_memcpy: %d" % rc)

        def leg_a():
            upload(fine_d, fine_h)

        def leg_b():
            upload(coarse_d, coarse_h)
            eng.forcing_regrid(plan, ncell, g, ents)
            eng.stream_sync()

        def leg_c():
            upload(coarse_d, coarse_h)
            eng.forcing_regrid_met(plan, ncell, g, met, rest)
            eng.stream_sync()

        def wall(fn):
            t0 = time.perf_counter()
            fn()
            return (time.perf_counter() - t0) * 1e3

        # faster and different is not faster: the full-size result against the restatement on a sample of columns
        for t in fine_d:
            t.fill_(7.0)
        torch.cuda.synchronize()
        leg_b()
        pick = np.sort(r.choice(ncell, SAMPLE, replace=False))
        want_plan, _ = np_plan(xlat.ravel()[pick], xlon.ravel()[pick], g, valid, 4)
        got_plan = plan[:6 * ncell].view(6, ncell)[:, torch.from_numpy(pick).cuda()].cpu().numpy()
        if not np.array_equal(got_plan, want_plan):
            raise SystemExit("regrid_bench: the plan of %s differs from the restatement" % cname)
        if unfilled != int((plan[:ncell] < 0).sum().item()):
            raise SystemExit("regrid_bench: unfilled count of %s" % cname)
        adj_h = adjust.cpu().numpy()[pick]
        for f, nm in enumerate(NAMES):
            want = np_regrid(want_plan, g, coarse_h[f].numpy(), modes[f], adj_h if adjs[f] is not None else None, -0.0065, -1.0e33)
            got = fine_d[f].cpu().numpy()[pick]
            if not np.array_equal(got.view(np.uint32), want.view(np.uint32)):
                raise SystemExit("regrid_bench: plane %s of %s differs from the restatement" % (nm, cname))
        for t in dst_m.values():
            t.fill_(7.0)
        torch.cuda.synchronize()
        fl = filled(want_plan, g)
        coarse_s = {nm: np_regrid(want_plan, g, coarse_h[ix[nm]].numpy(), BIL) for nm in MET}
        want_m = dict(zip(MET, np_met(*[coarse_s[nm] for nm in MET], adj_h, -0.0065)))
        want_c = {nm: np.where(fl, F(-1.0e33), want_m[nm]).astype(F) if nm in MET else
                  np_regrid(want_plan, g, coarse_h[ix[nm]].numpy(), modes[ix[nm]], None, 0.0, -1.0e33) for nm in NAMES}
        leg_c()
        for nm in NAMES:
            got, want = dst_m[nm].cpu().numpy()[pick], want_c[nm]
            same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
            if not same.all():
                bad = np.flatnonzero(~same)
                raise SystemExit("regrid_bench: met call, plane %s of %s differs from the restatement in %d of %d columns, first %r vs %r"
                                 % (nm, cname, bad.size, got.size, got[bad[0]], want[bad[0]]))

        legs = (leg_a, leg_b, leg_c)
        for fn in legs:                                    # warm-up
            for _ in range(3):
                fn()
        ms = {fn: [] for fn in legs}
        for rep in range(a.reps):                          # alternating, the order rotated every repetition
            for q in range(3):
                fn = legs[(rep + q) % 3]
                ms[fn].append(wall(fn))
        sa, sb, sc3 = _stats(ms[leg_a]), _stats(ms[leg_b]), _stats(ms[leg_c])

        # the launch alone against a device-to-device copy of the bytes it moves
        nbytes = ncell * (24 + 4 * len(NAMES) + 4)
        cp_src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda").fill_(1)
        cp_dst = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

        def kernel():
            eng.forcing_regrid(plan, ncell, g, ents, stream=sh)

        def kernel_met():
            eng.forcing_regrid_met(plan, ncell, g, met, rest, stream=sh)

        def copy():
            rc = hip.hipMemcpyAsync(cp_dst.data_ptr(), cp_src.data_ptr(), nbytes // 2, HIP_MEMCPY_D2D, sh)
            if rc:
                raise RuntimeError("hipMemcpyAsync: %d" % rc)

        def window(fn, calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(calls):
                fn()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1) / calls

        timed = (kernel, kernel_met, copy)
        for fn in timed:
            window(fn, 5)
        calls = {fn: max(3, int(a.window_ms / max(window(fn, 5), 1e-3)) + 1) for fn in timed}
        km = {fn: [] for fn in timed}
        for rep in range(a.reps):
            for q in range(len(timed)):
                fn = timed[(rep + q) % len(timed)]
                km[fn].append(window(fn, calls[fn]))
        sk, sc = _stats(km[kernel]), _stats(km[copy])
        sm = _stats(km[kernel_met])
        results.append(dict(case=cname, ni=ni, nj=nj, nx=g.nx, ny=g.ny, unfilled=unfilled, plan_ms=plan_ms,
                            fine_mb=ncell * 4 * len(NAMES) / 1e6, coarse_mb=nxny * 4 * len(NAMES) / 1e6, a=sa, b=sb,
                            c=sc3, c_over_a=sc3["median"] / sa["median"], met=sm,
                            met_over_kernel=sm["median"] / sk["median"], met_over_copy=sm["median"] / sc["median"],
                            b_over_a=sb["median"] / sa["median"], a_gbs=ncell * 4 * len(NAMES) / sa["median"] / 1e6,
                            kernel=sk, copy=sc, kernel_bytes=nbytes, kernel_gbs=nbytes / sk["median"] / 1e6, copy_gbs=nbytes / sc["median"] / 1e6,
                            hbm_fraction=nbytes / sk["median"] / 1e6 / HBM_ACHIEVABLE_GBS, calls_per_window=dict(kernel=calls[kernel], copy=calls[copy])))
        print(json.dumps(results[-1]), flush=True)
        del coarse_h, coarse_d, fine_h, fine_d, dst_m, cp_src, cp_dst, plan, adjust, ents, met, rest
        torch.cuda.empty_cache()
    eng.stream_sync()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)
    fmt = lambda s: "%.3f (%.3f .. %.3f, %.3f)" % (s["median"], s["min"], s["max"], s["iqr"])
    lines = ["# Forcing regrid: what it replaces and what it costs", "",
             "`tools/regrid_bench.py` on one MI355X, one run.  (a) eight fine float32 planes from page-locked host memory to the device with",
             "`noahmp_hip_memcpy`; (b) eight coarse planes uploaded the same way + one `noahmp_hip_forcing_regrid` of 8 entries (seven bilinear,",
             "precipitation nearest, temperature with an adjust plane) + the wait for it; (c) the same with one `noahmp_hip_forcing_regrid_met`",
             "instead: t, p, q, lw as the elevation-adjusted met group, u, v, sw, pcp as four ordinary entries.  Host wall-clock of the whole",
             "sequence, (a), (b) and (c) alternating, %d repetitions after a warm-up; ms: median (min .. max, inter-quartile range).  Every plane" % a.reps,
             "of (b) and of (c) and the plan were first compared bit for bit with the numpy restatement on a %d-column" % SAMPLE,
             "sample of the full-size result.", "",
             "| case | fine MB | coarse MB | (a) fine upload ms | (a) GB/s | (b) coarse upload + regrid ms | (b)/(a) | (c) coarse upload + met regrid ms | (c)/(a) | plan ms (once) | unfilled |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for x in results:
        lines.append("| %s: %d x %d from %d x %d | %.1f | %.2f | %s | %.1f | %s | %.3f | %s | %.3f | %.1f | %d |" % (
            x["case"], x["ni"], x["nj"], x["nx"], x["ny"], x["fine_mb"], x["coarse_mb"], fmt(x["a"]), x["a_gbs"], fmt(x["b"]), x["b_over_a"],
            fmt(x["c"]), x["c_over_a"], x["plan_ms"], x["unfilled"]))
    lines += ["", "The launch alone (device events around windows of back-to-back calls, >= %g ms) against one `hipMemcpyAsync` device-to-device with" % a.window_ms,
              "the same bytes read + written (24 B of plan + 4 B per entry and column + 4 B of adjust; the source planes stay in cache and are not",
              "counted), alternating; fraction = kernel GB/s / %.0f GB/s, the rate a streaming kernel reaches on this chip." % HBM_ACHIEVABLE_GBS, "",
              "| case | MB moved | kernel ms | kernel GB/s | copy ms | copy GB/s | copy / kernel | fraction of %.1f TB/s |" % (HBM_ACHIEVABLE_GBS / 1e3),
              "|---|---|---|---|---|---|---|---|"]
    for x in results:
        lines.append("| %s | %.1f | %s | %.0f | %s | %.0f | %.2f | %.2f |" % (
            x["case"], x["kernel_bytes"] / 1e6, fmt(x["kernel"]), x["kernel_gbs"], fmt(x["copy"]), x["copy_gbs"],
            x["copy"]["median"] / x["kernel"]["median"], x["hbm_fraction"]))
    lines += ["", "The elevation-adjusted launch in the same windows: (i) the launch above, (ii) `noahmp_hip_forcing_regrid_met` with the met group + 4",
              "entries (the same eight planes, the same bytes; one column per thread), (iii) the copy above.  The chain makes five expf and two",
              "powf per column, all in float64.", "",
              "| case | (i) ms | (ii) ms | (iii) ms | (ii)/(i) | (ii)/(iii) |",
              "|---|---|---|---|---|---|"]
    for x in results:
        lines.append("| %s | %s | %s | %s | %.2f | %.2f |" % (
            x["case"], fmt(x["kernel"]), fmt(x["met"]), fmt(x["copy"]), x["met_over_kernel"], x["met_over_copy"]))
    lines.append("")
    worst = max(results, key=lambda x: max(x["b_over_a"], x["c_over_a"]))
    worst_r = max(worst["b_over_a"], worst["c_over_a"])
    lines.append("Condition: (b) and (c) shorter than (a) in the same run.  Largest of (b)/(a), (c)/(a): %.3f (%s) -- %s." % (
        worst_r, worst["case"], "met in every case" if worst_r < 1.0 else "NOT MET"))
    lines.append("")
    if a.note and os.path.exists(a.note):
        lines.append(open(a.note).read().rstrip())
        lines.append("")
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("wrote", a.out)
    if worst_r >= 1.0:
        raise SystemExit("regrid_bench: (b) or (c) is not shorter than (a)")


if __name__ == "__main__":
    main()
