"""What the shortwave forcing costs per step and per record, against the interpolation launch it follows, in one run.

    python tools/shortwave_bench.py [--reps 30] [--window-ms 8] [--out profiles/shortwave_bench.md] [--json FILE] [--note FILE]

Shapes: 7 077 888 columns (the 4608 x 1536 config-3 grid) and the 884 736-column tile (1152 x 768) of an 8-rank run.  The tool makes its
own XLAT / XLONG (a 1 km grid over the conterminous US), normals from slopes up to 35 degrees of every aspect, and shortwave records.
Timed, each with two device events around a window of back-to-back calls (sized to --window-ms), ALTERNATING with the order rotated every
repetition:
  (l)  noahmp_hip_forcing_shortwave, NOAHMP_SW_LINEAR with sw_b (12 B per column);
  (z)  NOAHMP_SW_ZENITH (20 B per column);
  (t)  NOAHMP_SW_ZENITH with the three normals (32 B per column);
  (l1) (l) into a destination offset by one float: the one-column path instead of the four-column path that only this pure stream has;
  (m12) (m36)  noahmp_hip_forcing_cosz_mean with 12 and with 36 samples (12 B per column);
  (p)  noahmp_hip_forcing_interpolate_prep on the same shape, record a with fpar and lai: the yardstick (156 B per column).
The calls of a window walk through as many copies of all their planes as it takes to exceed twice the 256 MB last-level cache, so that
no call finds its planes there, as in a run, where the column kernel streams gigabytes between two forcing calls.
Every case is warmed up first; --reps repetitions (at least 20); median, minimum, maximum and inter-quartile range.  The expectation that
(t) stays below (p) is recorded, not enforced.  A process of its own: start it under `timeout -k 10 ...`.

Before a case is timed, the results of (l), (z), (t), (l1) and (m36) are compared bit for bit with the numpy restatement of
the contract (tests/test_shortwave.py: np_shortwave, np_mean with glibc's sinf / cosf) on a 4096-column sample of the full-size result.
Without a GPU it fails (there is nothing to measure on a CPU).

The markdown it writes also takes notes (--note FILE: text appended as it is, e.g. bench.py's headline before and after the change).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))          # the restatement lives in the test module, imported by its bare name
os.environ.setdefault("GPU_PINNED_MIN_XFER_SIZE", "1048576")

F = np.float32
HBM_ACHIEVABLE_GBS = 6300.0          # what a streaming kernel reaches on this chip (the microarchitecture notes' figure)
CACHE_FLUSH_BYTES = 640 * 1000 * 1000      # more than twice the 256 MB last-level cache
SAMPLE = 4096
START = (2001, 171, 18, 0, 0)
NOW = (171, 19, 30, 0)
IDTS, IDTS2 = 5400, 10800
PAR = (10.0, 0.05, 5.0, 1361.0)
# interpolate_prep: 10 + 7 record planes read, 10 planes of interp_cell written, then 5 level-2 copies, RAINBL, 2 x DZ8W, VEGFRA read and
# written, COSZIN, and XLAT / LON read: 39 words per column (what it re-reads of its own stores comes from the cache)
BYTES = dict(l=12, l1=12, z=20, t=32, m12=12, m36=12, p=156)


def _stats(ms):
    q = statistics.quantiles(ms, n=4)
    return dict(median=statistics.median(ms), min=min(ms), max=max(ms), iqr=q[2] - q[0], n=len(ms))


def prep_set(abi, torch, plane, ncell, ni, nj, lat):
    """One argument block, record pair, rain plane and longitude plane of noahmp_hip_forcing_interpolate_prep over ni x nj columns."""
    sa = abi.StepArgs()
    keep = {}
    for nm in ("t3d", "qv3d", "u_phy", "v_phy", "p8w3d", "dz8w"):
        keep[nm] = torch.zeros(2 * ncell, dtype=torch.float32, device="cuda")
    for nm in ("glw", "swdown", "vegfra", "xlaixy", "rainbl", "coszin", "eahxy", "tahxy", "chxy", "cmxy"):
        keep[nm] = torch.zeros(ncell, dtype=torch.float32, device="cuda")
    keep["xlatin"] = lat
    for nm, t in keep.items():
        setattr(sa, nm, t.data_ptr())
    sa.dt = 1800.0
    sa.ims = sa.its = sa.ids = 1
    sa.ime = sa.ite = sa.ide = ni
    sa.jms = sa.jts = sa.jds = 1
    sa.jme = sa.jte = sa.jde = nj
    sa.kms = sa.kts = sa.kds = 1
    sa.kme = sa.kte = sa.kde = 2
    recs = []
    for fields in (abi.FORCING_RECORD_FIELDS, abi.FORCING_RECORD_FIELDS[:7]):
        rec = abi.ForcingRecord()
        rec._keep = [plane() for _ in fields]
        for nm, t in zip(fields, rec._keep):
            setattr(rec, nm, t.data_ptr())
        recs.append(rec)
    return sa, recs, torch.zeros(ncell, dtype=torch.float32, device="cuda"), plane(), keep


def grid(ni, nj, i0=0, j0=0, gi=4608, gj=1536):
    j, i = np.meshgrid(np.arange(j0, j0 + nj), np.arange(i0, i0 + ni), indexing="ij")
    lat = 25.2 + (52.5 - 25.2) * j / (gj - 1) + 0.3 * np.sin(i / gi * 3.0)
    lon = -124.7 + (-67.4 + 124.7) * i / (gi - 1) + 0.2 * np.sin(j / gj * 2.0)
    return lat.astype(F), lon.astype(F)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--window-ms", type=float, default=8.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shortwave_bench.md"))
    ap.add_argument("--json", default=None)
    ap.add_argument("--note", default=None)
    a = ap.parse_args()
    a.reps = max(a.reps, 20)
    import torch
    from noahmp_amd import abi
    from noahmp_amd.driver import Engine
    from noahmp_amd.shortwave import sample_times
    from noahmp_amd.tables import load_tables
    import test_shortwave as ts
    if not torch.cuda.is_available():
        raise SystemExit("shortwave_bench: no GPU -- nothing to measure")
    eng = Engine(load_tables("usgs")[0], device=0)
    lib = eng.lib
    stream = torch.cuda.Stream()
    sh = stream.cuda_stream
    r = np.random.default_rng(1)
    results = []
    for cname, ni, nj, i0, j0 in (("7 077 888 columns (4608 x 1536)", 4608, 1536, 0, 0), ("884 736-column tile (1152 x 768)", 1152, 768, 1152, 768)):
        ncell = ni * nj
        lat, lon = grid(ni, nj, i0, j0)
        slope, asp = r.uniform(0.0, 0.6, ncell), r.uniform(0.0, 2 * np.pi, ncell)
        h = dict(lat=lat.ravel(), lon=lon.ravel(), ne=(np.sin(slope) * np.sin(asp)).astype(F), nn=(np.sin(slope) * np.cos(asp)).astype(F),
                 nu=np.cos(slope).astype(F), sw_a=r.uniform(0.0, 1000.0, ncell).astype(F), sw_b=r.uniform(0.0, 1000.0, ncell).astype(F))
        d = {k: torch.from_numpy(v).cuda() for k, v in h.items()}
        d["mean_a"] = torch.empty(ncell, dtype=torch.float32, device="cuda")
        pool = torch.full((ncell + 8,), 7.0, dtype=torch.float32, device="cuda")
        dst = {0: pool[4:4 + ncell], 1: pool[5:5 + ncell]}
        # the timed calls walk through nset copies of every plane, so that a call finds none of its planes in the last-level cache
        nset = -(-CACHE_FLUSH_BYTES // (36 * ncell))
        nsetp = -(-CACHE_FLUSH_BYTES // (BYTES["p"] * ncell))
        t12 = [t[1:] for t in sample_times(START, 10800, 12)]
        t36 = [t[1:] for t in sample_times(START, 10800, 36)]
        torch.cuda.synchronize()
        eng.cosz_mean(d["lat"], d["lon"], t36, d["mean_a"])
        eng.stream_sync()
        pick = np.sort(r.choice(ncell, SAMPLE, replace=False))
        pick_d = torch.from_numpy(pick).cuda()
        x = {k: v[pick] for k, v in h.items()}
        x["mean_a"] = ts.np_mean(x["lat"], x["lon"], [ts.np_suntime(t) for t in t36])

        def same(got, want, what):
            ok = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
            if not ok.all():
                bad = np.flatnonzero(~ok)
                raise SystemExit("shortwave_bench: %s of %s differs from the restatement in %d of %d columns, first %r vs %r"
                                 % (what, cname, bad.size, got.size, got[bad[0]], want[bad[0]]))
        same(d["mean_a"][pick_d].cpu().numpy(), x["mean_a"], "the interval mean")

        def block(mode, terrain, off, d=d, dst=dst):
            return eng.shortwave_block(d["sw_a"], d["lat"], d["lon"], dst[off], sw_b=d["sw_b"] if mode == "linear" else None,
                                       mean_a=d["mean_a"] if mode == "zenith" else None, normal=(d["ne"], d["nn"], d["nu"]) if terrain else None,
                                       idts=IDTS, idts2=IDTS2, mode=mode, max_ratio=PAR[0], mu_min=PAR[1], max_terrain_ratio=PAR[2],
                                       solar_constant=PAR[3])
        blocks = {}
        for key, mode, terrain in (("l", "linear", False), ("z", "zenith", False), ("t", "zenith", True)):
            want = ts.np_shortwave(x, abi.SW_MODE[mode], mode == "linear", terrain, ts.np_suntime(NOW), PAR, IDTS, IDTS2)
            for off in ((0, 1) if key == "l" else (0,)):
                b = blocks[key + ("1" if off else "")] = block(mode, terrain, off)
                pool.fill_(7.0)
                torch.cuda.synchronize()
                eng.forcing_shortwave(b, ncell, NOW)
                eng.stream_sync()
                same(dst[off][pick_d].cpu().numpy(), want, "mode %s terrain %d offset %d" % (mode, terrain, off))

        sets = [(d, dst)]
        for _ in range(nset - 1):
            dd = {k: v.clone() for k, v in d.items()}
            pp = torch.full((ncell + 8,), 7.0, dtype=torch.float32, device="cuda")
            sets.append((dd, {0: pp[4:4 + ncell], 1: pp[5:5 + ncell]}))
        ring = {key: [block(mode, terrain, off, dd, ds) for dd, ds in sets]
                for key, mode, terrain, off in (("l", "linear", False, 0), ("l1", "linear", False, 1), ("z", "zenith", False, 0), ("t", "zenith", True, 0))}

        # the yardstick: noahmp_hip_forcing_interpolate_prep on the same shape, from hand-made argument blocks
        plane = lambda: torch.rand(ncell, dtype=torch.float32, device="cuda")
        preps = []
        for _ in range(nsetp):
            preps.append(prep_set(abi, torch, plane, ncell, ni, nj, d["lat"].clone()))
        jul = C.c_float(0)
        torch.cuda.synchronize()
        turn = dict(p=0, m=0)

        def prep():
            sa, recs, rain, lon_p = preps[turn["p"] % nsetp][:4]
            turn["p"] += 1
            rc = lib.noahmp_hip_forcing_interpolate_prep(C.byref(sa), C.byref(recs[0]), C.byref(recs[1]), IDTS, IDTS2, rain.data_ptr(),
                                                         lon_p.data_ptr(), NOW[0], NOW[1], NOW[2], NOW[3], 10.0, 1, C.byref(jul),
                                                         abi.MEM_DEVICE, sh, None)
            if rc:
                raise RuntimeError("noahmp_hip_forcing_interpolate_prep: %d %s" % (rc, lib.noahmp_hip_last_error().decode()))
        t12a, t36a = Engine.sun_times(t12), Engine.sun_times(t36)

        def shortwave_of(key):
            state = dict(i=0)

            def go():
                eng.forcing_shortwave(ring[key][state["i"] % nset], ncell, NOW, stream=sh)
                state["i"] += 1
            return go

        def mean_of(times):
            def go():
                dd, ds = sets[turn["m"] % nset]
                turn["m"] += 1
                eng.cosz_mean(dd["lat"], dd["lon"], times, ds[0], stream=sh)
            return go
        fns = {k: shortwave_of(k) for k in ring}
        fns["m12"], fns["m36"], fns["p"] = mean_of(t12a), mean_of(t36a), prep

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
        results.append(dict(case=cname, ni=ni, nj=nj, ncell=ncell, plane_sets=nset, prep_sets=nsetp, stats=st, calls_per_window=calls,
                            gbs={k: BYTES[k] * ncell / st[k]["median"] / 1e6 for k in keys},
                            t_over_p=st["t"]["median"] / st["p"]["median"]))
        print(json.dumps(results[-1]), flush=True)
        del d, pool, dst, blocks, sets, ring, preps, fns
        torch.cuda.empty_cache()
    eng.stream_sync()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)
    fmt = lambda s: "%.4f (%.4f .. %.4f, %.4f)" % (s["median"], s["min"], s["max"], s["iqr"])
    names = dict(l="LINEAR with sw_b (four columns per thread)", z="ZENITH", t="ZENITH + terrain", l1="LINEAR with sw_b, one column per thread", m12="cosz_mean, 12 samples", m36="cosz_mean, 36 samples",
                 p="forcing_interpolate_prep (yardstick)")
    lines = ["# Shortwave forcing: the per-step and the per-record launch", "",
             "`tools/shortwave_bench.py` on one MI355X, one run.  Device events around windows of back-to-back calls (>= %g ms), the cases" % a.window_ms,
             "alternating with the order rotated, %d repetitions after a warm-up; ms per call: median (min .. max, inter-quartile range).  GB/s = the" % a.reps,
             "bytes the call must move per column (B/col) over the median; %.1f TB/s is what a streaming kernel reaches on this chip.  The aligned" % (HBM_ACHIEVABLE_GBS / 1e3),
             "LINEAR call takes its four-column path, the same call into a destination offset by one float the one-column path every other call has.",
             "Consecutive calls of a window work on different copies of all their planes (more than 512 MB in a round), so nothing is found in",
             "the last-level cache.  The results of every",
             "shortwave case and of the 36-sample mean were first compared bit for bit with the numpy restatement on a %d-column sample." % SAMPLE, ""]
    for x in results:
        lines += ["## %s" % x["case"], "", "| call | B/col | ms | GB/s | calls per window |", "|---|---|---|---|---|"]
        for k in x["stats"]:
            lines.append("| %s | %d | %s | %.0f | %d |" % (names[k], BYTES[k], fmt(x["stats"][k]), x["gbs"][k], x["calls_per_window"][k]))
        lines += ["", "ZENITH + terrain / forcing_interpolate_prep = %.2f (expected below 1: about a third of the bytes) -- %s." % (
            x["t_over_p"], "as expected" if x["t_over_p"] < 1.0 else "NOT as expected"), ""]
    if a.note and os.path.exists(a.note):
        lines.append(open(a.note).read().rstrip())
        lines.append("")
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
