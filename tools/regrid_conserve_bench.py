"""What the budget-preserving regrid of precipitation costs, against what a caller uses today and against a copy of its bytes.

    python tools/regrid_conserve_bench.py [--reps 20] [--window-ms 8] [--copies 3] [--out profiles/regrid_conserve_bench.md] [--json FILE]
                                         [--lib OTHER_BUILD.so]

Shapes: 4608 x 1536 (7 077 888 window cells, the config-3 grid) and 1152 x 768 (884 736, the tile of an 8-rank run), both fed from a
464 x 224 source at 0.125 degrees (NLDAS-2 like): about 150 model cells per source cell.  The tool makes its own XLAT / XLONG.

Timed, each a median over --reps windows of back-to-back calls between two device events (windows sized to --window-ms), the cases
alternating with the order rotated every repetition, consecutive calls on different copies of their destination and pattern planes:
  plan       noahmp_hip_regrid_conserve_plan (host wall-clock: the call waits), with an area plane;
  record     noahmp_hip_forcing_regrid_conserve with 1 and 3 entries, without and with a pattern, in tile order (dst_index NULL) and
             through a random permutation as dst_index (a sorted column order);
  nearest    noahmp_hip_forcing_regrid with ONE NEAREST entry on the same regrid plan: what a caller uses for precipitation today;
  copy       ONE hipMemcpyAsync device-to-device whose bytes read plus written are the bytes the two passes of the one-entry record call
             must move: level 1 reads 4 B of member index, 20 B of plan and 4 B of area per member, the apply pass reads 4 B of group and
             20 B of plan and writes 4 B per cell; the source planes and the per-group table stay in cache and are not counted.
  prep       noahmp_hip_forcing_interpolate_prep on the same shape (tools/shortwave_bench.py's hand-made argument blocks, 156 B per
             column): the yardstick of the forcing calls.
Before anything is timed the full-size result of the three-entry call is compared with the numpy restatement of the contract
(tests/test_regrid_conserve.py) on the groups of a sample of source cells, bit for bit.  Without a GPU it fails (nothing to measure).
A process of its own: start it under `timeout -k 10 ...`."""
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
HIP_MEMCPY_D2D = 3
NLDAS = (464, 224, -124.9375, 25.0625, 0.125, 0.125, False)
SAMPLE_GROUPS = 12


def conus(ni, nj, i0=0, j0=0, gi=4608, gj=1536):
    j, i = np.meshgrid(np.arange(j0, j0 + nj), np.arange(i0, i0 + ni), indexing="ij")
    lat = 25.2 + (52.5 - 25.2) * j / (gj - 1) + 0.3 * np.sin(i / gi * 3.0)             # a gently curved 1 km grid inside the source
    lon = -124.7 + (-67.4 + 124.7) * i / (gi - 1) + 0.2 * np.sin(j / gj * 2.0)
    return lat.astype(F), lon.astype(F)


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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--window-ms", type=float, default=8.0)
    ap.add_argument("--copies", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "regrid_conserve_bench.md"))
    ap.add_argument("--json", default=None)
    ap.add_argument("--lib", default=None, help="another build of the library (A/B of a tuning knob)")
    a = ap.parse_args()
    import torch
    from noahmp_amd.driver import Engine
    from noahmp_amd.tables import load_tables
    from noahmp_amd import abi
    from test_regrid import np_plan
    from tools.shortwave_bench import prep_set, IDTS, IDTS2, NOW
    from test_regrid_conserve import np_conserve, np_groups
    if not torch.cuda.is_available():
        raise SystemExit("regrid_conserve_bench: no GPU -- nothing to measure")
    eng = Engine(load_tables("usgs")[0], device=0, lib_path=a.lib)
    hip = _hip_runtime()
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    stream = torch.cuda.Stream()
    sh = stream.cuda_stream
    r = np.random.default_rng(1)
    g = Engine.regrid_source(*NLDAS)
    nxny = g.nx * g.ny
    results = []
    for cname, ni, nj, make in (("config 3 grid", 4608, 1536, lambda: conus(4608, 1536)),
                                ("8-rank tile", 1152, 768, lambda: conus(1152, 768, i0=1152, j0=768))):
        ncell = ni * nj
        xlat, xlon = make()
        plan, unfilled = eng.regrid_plan(torch.from_numpy(xlat).cuda(), torch.from_numpy(xlon).cuda(), g)
        area_h = r.uniform(0.9e6, 1.1e6, ncell).astype(F)
        area = torch.from_numpy(area_h).cuda()
        perm = torch.randperm(ncell, device="cuda").to(torch.int32).contiguous()
        torch.cuda.synchronize()
        plan_ms = []
        for _ in range(5):
            t0 = time.perf_counter()
            cp = eng.regrid_conserve_plan(plan, ni, nj, g, area=area)
            plan_ms.append((time.perf_counter() - t0) * 1e3)
        srcs_h = [r.uniform(0.0, 1e-3, nxny).astype(F) for _ in range(3)]
        for s in srcs_h:
            s[r.random(nxny) < 0.3] = 0.0
        srcs = [torch.from_numpy(s).cuda() for s in srcs_h]
        pats_h = [r.uniform(0.5, 2.0, ncell).astype(F) for _ in range(a.copies)]
        pats = [torch.from_numpy(p).cuda() for p in pats_h]
        dsts = [[torch.full((ncell,), 7.0, dtype=torch.float32, device="cuda") for _ in range(3)] for _ in range(a.copies)]
        ents = {(n, pt, k): eng.regrid_conserve_entries([(srcs[f], dsts[k][f], pats[k] if pt else None, -1.0e33) for f in range(n)])
                for n in (1, 3) for pt in (False, True) for k in range(a.copies)}
        near = [eng.regrid_entries([(srcs[0], dsts[k][0], "nearest", None, 0.0, -1.0e33)]) for k in range(a.copies)]
        eng.forcing_regrid_conserve(cp, ents[3, True, 0])
        eng.stream_sync()

        # faster and different is not faster: the groups of a sample of source cells against the restatement
        grp_all = plan[ncell:2 * ncell].cpu().numpy()
        plan_h = plan[:6 * ncell].cpu().numpy().reshape(6, ncell)
        owners = r.choice(np.unique(grp_all[grp_all >= 0]), SAMPLE_GROUPS, replace=False)
        pick = np.flatnonzero(np.isin(grp_all, owners))
        want_plan, _ = np_plan(xlat.ravel()[pick], xlon.ravel()[pick], g)
        if not np.array_equal(want_plan, plan_h[:, pick]):
            raise SystemExit("regrid_conserve_bench: the plan of %s differs from the restatement" % cname)
        for f in range(3):
            want, _, _ = np_conserve(want_plan, g, srcs_h[f], area_h[pick], pats_h[0][pick], -1.0e33, np_groups(want_plan, g))
            got = dsts[0][f].cpu().numpy()[pick]
            if not np.array_equal(got.view(np.uint32), want.view(np.uint32)):
                raise SystemExit("regrid_conserve_bench: entry %d of %s differs from the restatement" % (f, cname))

        nmember = int((grp_all >= 0).sum())
        nbytes = nmember * 28 + ncell * 28
        cp_src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda").fill_(1)
        cp_dst = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        turn = [0]

        def record(n, pt, sorted_order):
            def fn():
                turn[0] = (turn[0] + 1) % a.copies
                eng.forcing_regrid_conserve(cp, ents[n, pt, turn[0]], dst_index=perm if sorted_order else None, stream=sh)
            return fn

        def nearest():
            turn[0] = (turn[0] + 1) % a.copies
            eng.forcing_regrid(plan, ncell, g, near[turn[0]], stream=sh)

        def copy():
            rc = hip.hipMemcpyAsync(cp_dst.data_ptr(), cp_src.data_ptr(), nbytes // 2, HIP_MEMCPY_D2D, sh)
            if rc:
                raise RuntimeError("hipMemcpyAsync: %d" % rc)

        plane = lambda: torch.rand(ncell, dtype=torch.float32, device="cuda")
        lat_d = torch.from_numpy(xlat.ravel()).cuda()
        preps = [prep_set(abi, torch, plane, ncell, ni, nj, lat_d) for _ in range(2)]
        jul = C.c_float(0)
        torch.cuda.synchronize()

        def prep():
            turn[0] = (turn[0] + 1) % a.copies
            sa, recs, rain, lon_p = preps[turn[0] % 2][:4]
            rc = eng.lib.noahmp_hip_forcing_interpolate_prep(C.byref(sa), C.byref(recs[0]), C.byref(recs[1]), IDTS, IDTS2, rain.data_ptr(),
                                                             lon_p.data_ptr(), NOW[0], NOW[1], NOW[2], NOW[3], 10.0, 1, C.byref(jul),
                                                             abi.MEM_DEVICE, sh, None)
            if rc:
                raise RuntimeError("noahmp_hip_forcing_interpolate_prep: %d %s" % (rc, eng.lib.noahmp_hip_last_error().decode()))

        def window(fn, calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(calls):
                fn()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1) / calls

        timed = {"record n=%d%s%s" % (n, " pattern" if pt else "", " sorted" if so else ""): record(n, pt, so)
                 for n in (1, 3) for pt in (False, True) for so in (False, True)}
        timed["nearest n=1"] = nearest
        timed["copy"] = copy
        timed["prep"] = prep
        keys = list(timed)
        for k in keys:
            window(timed[k], 5)
        calls = {k: max(3, int(a.window_ms / max(window(timed[k], 5), 1e-3)) + 1) for k in keys}
        ms = {k: [] for k in keys}
        for rep in range(max(a.reps, 10)):
            for q in range(len(keys)):
                k = keys[(rep + q) % len(keys)]
                ms[k].append(window(timed[k], calls[k]))
        st = {k: _stats(v) for k, v in ms.items()}
        results.append(dict(case=cname, ni=ni, nj=nj, ncell=ncell, nmember=nmember, unfilled=unfilled, plan_ms=_stats(plan_ms), bytes_n1=nbytes,
                            times=st, levels=3 if ncell > 0 and max(np.bincount(grp_all[grp_all >= 0])) > 65536 else 2))
        print(json.dumps(results[-1]), flush=True)
        del dsts, pats, ents, near, cp, plan, cp_src, cp_dst, preps
        torch.cuda.empty_cache()
    eng.stream_sync()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)
    fmt = lambda s: "%.4f (%.4f .. %.4f, %.4f)" % (s["median"], s["min"], s["max"], s["iqr"])
    lines = ["# Budget-preserving regrid: what it costs", "",
             "`tools/regrid_conserve_bench.py` on one MI355X, one run.  Device events around windows of back-to-back calls (>= %g ms)," % a.window_ms,
             "the cases alternating, consecutive calls on %d different copies of their destination and pattern planes;" % a.copies,
             "ms: median (min .. max, inter-quartile range).  The three-entry result was first compared bit for bit with the numpy",
             "restatement on the groups of %d source cells.  `nearest`: one NEAREST entry of `noahmp_hip_forcing_regrid` on the same plan" % SAMPLE_GROUPS,
             "(this library's kernel; the change does not touch it).  `copy`: one device-to-device copy of the bytes both passes of the",
             "one-entry record call must move (56 B per cell).  `prep`: `noahmp_hip_forcing_interpolate_prep` on the same shape."]
    for x in results:
        t = x["times"]
        lines += ["", "## %s: %d x %d = %d window cells from 464 x 224" % (x["case"], x["ni"], x["nj"], x["ncell"]), "",
                  "Plan call (host wall-clock, 5 calls): %s ms." % fmt(x["plan_ms"]), "",
                  "| call | ms | / nearest | / copy | / prep |", "|---|---|---|---|---|"]
        for k, s in t.items():
            lines.append("| %s | %s | %.2f | %.2f | %.2f |" % (k, fmt(s), s["median"] / t["nearest n=1"]["median"], s["median"] / t["copy"]["median"],
                                                           s["median"] / t["prep"]["median"]))
        lines.append("")
        lines.append("Copy: %.1f MB in %.4f ms = %.0f GB/s." % (x["bytes_n1"] / 1e6, t["copy"]["median"], x["bytes_n1"] / t["copy"]["median"] / 1e6))
    lines.append("")
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
