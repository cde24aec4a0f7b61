"""What cast shadows cost per step: the terrain ray march and the lit shortwave call against the unshaded call and the interpolation
launch, in one run.

    python tools/shadow_bench.py [--reps 30] [--window-ms 8] [--out profiles/shadow_bench.md] [--json FILE] [--note FILE] [--forms 2,4]

Shapes: 4608 x 1536 (the config-3 grid) and the 1152 x 768 tile of an 8-rank run, 1 km spacing, nstep 25 (WRF's shadlen of 25 km), a
synthetic terrain with about 2 km relief (three superposed wave trains of 125, 20 and 7 cells).  The latitude / longitude planes span less
than half a degree, so that the WHOLE grid sits at the stated sun -- the worst case everywhere, which a real CONUS grid with its 57 degrees
of longitude never is.  Suns, found with the restatement at the grid's centre on day 171: night, mu about 0.10 (the worst case: long
shadows, long marches), mu about 0.5, noon.
Timed, each with two device events around a window of back-to-back calls (sized to --window-ms), ALTERNATING with the order rotated every
repetition:
  (s_night) (s_low) (s_mid) (s_noon)  noahmp_hip_forcing_shadow at the four suns (12 B per cell read once, 4 B written; the march re-reads
        heights through the caches);
  (s_low/nfN) (s_mid/nfN)  the same from a library built with N steps in flight (--forms; the default library has 1);
  (t)   noahmp_hip_forcing_shortwave, ZENITH with the three normals: the unshaded call, a yardstick (32 B per column);
  (tl_low) (tl_mid)  noahmp_hip_forcing_shortwave_lit with the lit plane of that sun (36 B per column);
  (tl_one) the same with a plane of ones;
  (p)   noahmp_hip_forcing_interpolate_prep on the same shape: the second yardstick (156 B per column).
Consecutive calls of a window work on different copies of all their planes (more than twice the 256 MB last-level cache in a round).
Every case is warmed up first; --reps repetitions (at least 20); median, minimum, maximum and inter-quartile range.  Nothing is enforced.
A process of its own: start it under `timeout -k 10 ...`.

Before anything is timed, the lit plane of the low and the mid sun is compared bit for bit with the numpy restatement (tests/test_shadow.py)
on the 64 x 64 corner block of the full-size result (restated on that block plus nstep cells), from every library form, and the lit
shortwave call on a 4096-column sample.  Without a GPU it fails (there is nothing to measure on a CPU).
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

F = np.float32
NSTEP = 25
DX = 1000.0
MU_MIN = 0.05
PAR = (10.0, 0.05, 5.0, 1361.0)
START = (2001, 171, 18, 0, 0)
SAMPLE = 4096
CORNER = 64
BYTES = dict(s=16, t=32, tl=36, p=156)


def terrain(ni, nj):
    j, i = np.meshgrid(np.arange(nj), np.arange(ni), indexing="ij")
    z = 1500.0 + 550.0 * np.sin(i * 0.05) * np.cos(j * 0.043) + 300.0 * np.sin(i * 0.31 + j * 0.17) + 150.0 * np.sin(i * 0.9) * np.sin(j * 1.1)
    return z.astype(F)


def latlon(ni, nj):
    j, i = np.meshgrid(np.arange(nj), np.arange(ni), indexing="ij")
    return (39.0 + 1e-4 * j).astype(F), (-105.0 + 1e-4 * i).astype(F)


def find_suns(lat, lon):
    """night, mu ~ 0.10, mu ~ 0.5 and noon of day 171 at (lat, lon), by the restatement."""
    import test_shortwave as ts
    la, lo = np.array([lat], F), np.array([lon], F)
    best = {}
    for minute in range(19 * 60, 27 * 60, 2):                                # local noon .. evening at 105 W
        t = (171 + minute // 1440, (minute // 60) % 24, minute % 60, 0)
        mu = float(ts.max0(ts.np_sun(la, lo, ts.np_suntime(t))[2])[0])
        for target in (0.10, 0.5):
            if target not in best or abs(mu - target) < best[target][0]:
                best[target] = (abs(mu - target), t, mu)
    return dict(night=(171, 8, 0, 0), low=best[0.10][1], mid=best[0.5][1], noon=(171, 19, 0, 0)), {k: v[2] for k, v in best.items()}


def variant(nf):
    """The library with nf steps in flight, built on demand next to the default one."""
    from noahmp_amd import build as b
    path = os.path.join(b.CSRC, "variants", "lib_shadow_nf%d.so" % nf)
    if not os.path.exists(path) or os.path.getmtime(path) < max(os.path.getmtime(os.path.join(b.CSRC, f)) for f in ("noahmp_shadow.hip", "nmp_dev_shadow.hpp")):
        b.build(extra_flags=["-DNMP_SHADOW_INFLIGHT=%d" % nf], lib=path, jobs=8)
    return path


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--window-ms", type=float, default=8.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shadow_bench.md"))
    ap.add_argument("--json", default=None)
    ap.add_argument("--note", default=None)
    ap.add_argument("--forms", default="2,4", help="other numbers of steps in flight to measure next to the built-in 1 ('' for none)")
    ap.add_argument("--build-only", action="store_true", help="build the variant libraries of --forms and stop (needs no GPU)")
    a = ap.parse_args()
    a.reps = max(a.reps, 20)
    forms = [int(v) for v in a.forms.split(",") if v]
    paths = {nf: variant(nf) for nf in forms}
    if a.build_only:
        print("built", paths)
        return
    import torch
    from noahmp_amd import abi
    from noahmp_amd.driver import Engine
    from noahmp_amd.shortwave import sample_times, normal_from_height
    from noahmp_amd.tables import load_tables
    import test_shortwave as ts
    import test_shadow as tsh
    if not torch.cuda.is_available():
        raise SystemExit("shadow_bench: no GPU -- nothing to measure")
    eng = Engine(load_tables("usgs")[0], device=0)
    lib = eng.lib
    libs = {nf: abi.load_library(p) for nf, p in paths.items()}
    stream = torch.cuda.Stream()
    sh = stream.cuda_stream
    r = np.random.default_rng(1)
    results = []
    for cname, ni, nj in (("7 077 888 cells (4608 x 1536)", 4608, 1536), ("884 736-cell tile (1152 x 768)", 1152, 768)):
        ncell = ni * nj
        z = terrain(ni, nj)
        lat, lon = latlon(ni, nj)
        suns, mus = find_suns(float(lat[nj // 2, ni // 2]), float(lon[nj // 2, ni // 2]))
        hmax = float(z.max())
        zd, latd, lond = (torch.from_numpy(v).cuda() for v in (z, lat, lon))
        ne, nn, nu, _, _ = normal_from_height(zd, DX, DX)
        d = dict(lat=latd.reshape(-1), lon=lond.reshape(-1), ne=ne.reshape(-1).contiguous(), nn=nn.reshape(-1).contiguous(), nu=nu.reshape(-1).contiguous(),
                 sw_a=torch.from_numpy(r.uniform(0.0, 1000.0, ncell).astype(F)).cuda(), mean_a=torch.empty(ncell, dtype=torch.float32, device="cuda"))
        t36 = [t[1:] for t in sample_times(START, 10800, 36)]
        torch.cuda.synchronize()
        eng.cosz_mean(d["lat"], d["lon"], t36, d["mean_a"])
        eng.stream_sync()

        def shadow_block(zz, la, lo, lit):
            return eng.shadow_block(zz, la, lo, lit, DX, DX, nstep=NSTEP, mu_min=MU_MIN, height_max=hmax)

        # ---- correctness first: the corner block of the lit plane from every form, the lit shortwave call on a sample
        lits = {}
        w = CORNER + NSTEP
        idx = np.full((w, w), -1, np.int32)
        idx[:CORNER, :CORNER] = np.arange(CORNER * CORNER, dtype=np.int32).reshape(CORNER, CORNER)
        shares = {}
        for key in ("night", "low", "mid", "noon"):
            want, _ = tsh.np_cells(z[:w, :w], lat[:w, :w], lon[:w, :w], ts.np_suntime(suns[key]), DX, DX, NSTEP, MU_MIN, hmax, dst_index=idx,
                                   ndst=CORNER * CORNER)
            want = tsh.lit_of(want[:CORNER, :CORNER])
            for nf, L in [(1, lib)] + list(libs.items()):
                lit = torch.full((nj, ni), 7.0, dtype=torch.float32, device="cuda")
                torch.cuda.synchronize()
                rc = L.noahmp_hip_forcing_shadow(C.byref(shadow_block(zd, latd, lond, lit)), ncell, Engine.sun_times([suns[key]]), sh)
                if rc:
                    raise SystemExit("shadow_bench: noahmp_hip_forcing_shadow rc=%d %s" % (rc, L.noahmp_hip_last_error().decode()))
                stream.synchronize()
                got = lit[:CORNER, :CORNER].cpu().numpy()
                if not (got.view(np.uint32) == want.view(np.uint32)).all():
                    raise SystemExit("shadow_bench: the lit plane of %s, sun %s, %d in flight differs from the restatement in %d cells"
                                     % (cname, key, nf, (got != want).sum()))
                if nf == 1:
                    lits[key] = lit
                    shares[key] = float((lit == 0).float().mean().item())
        pick = np.sort(r.choice(ncell, SAMPLE, replace=False))
        pick_d = torch.from_numpy(pick).cuda()
        x = {k: d[k][pick_d].cpu().numpy() for k in ("sw_a", "mean_a", "lat", "lon", "ne", "nn", "nu")}
        x["sw_b"] = x["sw_a"]
        out = torch.full((ncell,), 7.0, dtype=torch.float32, device="cuda")

        def sw_block(dd, dst):
            return eng.shortwave_block(dd["sw_a"], dd["lat"], dd["lon"], dst, mean_a=dd["mean_a"], normal=(dd["ne"], dd["nn"], dd["nu"]), mode="zenith",
                                       max_ratio=PAR[0], mu_min=PAR[1], max_terrain_ratio=PAR[2], solar_constant=PAR[3])
        for key in ("low", "mid"):
            eng.forcing_shortwave_lit(sw_block(d, out), lits[key].reshape(-1), ncell, suns[key])
            eng.stream_sync()
            want, _ = tsh.np_lit(x, lits[key].reshape(-1)[pick_d].cpu().numpy(), ts.ZENITH, False, True, ts.np_suntime(suns[key]), PAR)
            got = out[pick_d].cpu().numpy()
            if not ((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))).all():
                raise SystemExit("shadow_bench: forcing_shortwave_lit of %s, sun %s differs from the restatement" % (cname, key))

        # ---- the rings of plane copies
        nset_s = -(-CACHE_FLUSH_BYTES // (BYTES["s"] * ncell))
        nset_t = -(-CACHE_FLUSH_BYTES // (BYTES["tl"] * ncell))
        nset_p = -(-CACHE_FLUSH_BYTES // (BYTES["p"] * ncell))
        ring_s = [shadow_block(zd.clone(), latd.clone(), lond.clone(), torch.empty((nj, ni), dtype=torch.float32, device="cuda")) for _ in range(nset_s)]
        sets_t = [({k: v.clone() for k, v in d.items()}, torch.empty(ncell, dtype=torch.float32, device="cuda")) for _ in range(nset_t)]
        ring_t = [sw_block(dd, dst) for dd, dst in sets_t]
        ones = [torch.ones(ncell, dtype=torch.float32, device="cuda") for _ in range(nset_t)]
        lit_ring = {key: [lits[key].reshape(-1).clone() for _ in range(nset_t)] for key in ("low", "mid")}
        lit_ring["one"] = ones
        plane = lambda: torch.rand(ncell, dtype=torch.float32, device="cuda")
        preps = [prep_set(abi, torch, plane, ncell, ni, nj, d["lat"].clone()) for _ in range(nset_p)]
        jul = C.c_float(0)
        torch.cuda.synchronize()
        now_of = {k: Engine.sun_times([t]) for k, t in suns.items()}

        def shadow_of(L, key):
            state = dict(i=0)

            def go():
                rc = L.noahmp_hip_forcing_shadow(C.byref(ring_s[state["i"] % nset_s]), ncell, now_of[key], sh)
                assert rc == 0, rc
                state["i"] += 1
            return go

        def unshaded():
            state = dict(i=0)

            def go():
                eng.forcing_shortwave(ring_t[state["i"] % nset_t], ncell, suns["low"], stream=sh)
                state["i"] += 1
            return go

        def lit_of(key):
            state = dict(i=0)
            sun = suns["low" if key == "one" else key]

            def go():
                q = state["i"] % nset_t
                eng.forcing_shortwave_lit(ring_t[q], lit_ring[key][q], ncell, sun, stream=sh)
                state["i"] += 1
            return go
        turn = dict(p=0)

        def prep():
            sa, recs, rain, lon_p = preps[turn["p"] % nset_p][:4]
            turn["p"] += 1
            now = suns["low"]
            rc = lib.noahmp_hip_forcing_interpolate_prep(C.byref(sa), C.byref(recs[0]), C.byref(recs[1]), 5400, 10800, rain.data_ptr(),
                                                         lon_p.data_ptr(), now[0], now[1], now[2], now[3], 10.0, 1, C.byref(jul), abi.MEM_DEVICE, sh, None)
            if rc:
                raise RuntimeError("noahmp_hip_forcing_interpolate_prep: %d %s" % (rc, lib.noahmp_hip_last_error().decode()))
        fns = {"s_" + k: shadow_of(lib, k) for k in ("night", "low", "mid", "noon")}
        for nf, L in libs.items():
            for k in ("low", "mid"):
                fns["s_%s/nf%d" % (k, nf)] = shadow_of(L, k)
        fns["t"] = unshaded()
        for k in ("low", "mid", "one"):
            fns["tl_" + k] = lit_of(k)
        fns["p"] = prep

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
        results.append(dict(case=cname, ni=ni, nj=nj, ncell=ncell, suns={k: list(v) for k, v in suns.items()}, mu=mus, shadowed=shares,
                            plane_sets=dict(s=nset_s, t=nset_t, p=nset_p), stats=st, calls_per_window=calls,
                            ratios={k: dict(over_t=med[k] / med["t"], over_p=med[k] / med["p"]) for k in keys}))
        print(json.dumps(results[-1]), flush=True)
        del ring_s, sets_t, ring_t, ones, lit_ring, preps, fns, lits, d
        torch.cuda.empty_cache()
    eng.stream_sync()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)
    fmt = lambda s: "%.4f (%.4f .. %.4f, %.4f)" % (s["median"], s["min"], s["max"], s["iqr"])

    def name(k):
        what = dict(s="shadow launch", t="forcing_shortwave ZENITH + terrain (unshaded, yardstick)", tl="forcing_shortwave_lit", p="forcing_interpolate_prep (yardstick)")
        head, _, tail = k.partition("_")
        sun, _, nf = tail.partition("/")
        return what[head] + ((", " + dict(night="night", low="mu ~ 0.10", mid="mu ~ 0.5", noon="noon", one="plane of ones")[sun]) if sun else "") + (
            (", %s steps in flight" % nf[2:]) if nf else (", 1 step in flight (built in)" if head == "s" else ""))
    lines = ["# Cast shadows: the ray march and the lit shortwave call", "",
             "`tools/shadow_bench.py` on one MI355X, one run.  1 km spacing, nstep %d, synthetic terrain with about 2 km relief; the whole grid sits at" % NSTEP,
             "the stated sun (latitude / longitude planes span less than half a degree).  Device events around windows of back-to-back calls",
             "(>= %g ms), the cases alternating with the order rotated, %d repetitions after a warm-up; ms per call: median (min .. max," % (a.window_ms, a.reps),
             "inter-quartile range).  Consecutive calls of a window work on different copies of all their planes (more than 512 MB in a round), so",
             "nothing is found in the last-level cache.  GB/s of the streams = bytes per column over the median (%.1f TB/s is what a streaming kernel" % (HBM_ACHIEVABLE_GBS / 1e3),
             "reaches on this chip); the shadow launch is no stream, its column shows the 16 B per cell it must move at least.  The lit planes of",
             "every sun and every library form were first compared bit for bit with the numpy restatement on a %d x %d corner block, the lit" % (CORNER, CORNER),
             "shortwave call on a %d-column sample." % SAMPLE, ""]
    for x in results:
        lines += ["## %s" % x["case"], "",
                  "Suns (iday, ihour, iminute, isecond): %s; mu at the centre: low %.3f, mid %.3f.  Shadowed share of the grid: %s." % (
                      ", ".join("%s %s" % (k, tuple(v)) for k, v in x["suns"].items()), x["mu"][0.10], x["mu"][0.5],
                      ", ".join("%s %.1f %%" % (k, 100 * v) for k, v in x["shadowed"].items())), "",
                  "| call | ms | GB/s (minimum bytes) | / unshaded | / interpolate_prep | calls per window |", "|---|---|---|---|---|---|"]
        for k in x["stats"]:
            b = BYTES[k.partition("_")[0]]
            lines.append("| %s | %s | %.0f | %.2f | %.2f | %d |" % (name(k), fmt(x["stats"][k]), b * x["ncell"] / x["stats"][k]["median"] / 1e6,
                                                                  x["ratios"][k]["over_t"], x["ratios"][k]["over_p"], x["calls_per_window"][k]))
        lines.append("")
    if a.note and os.path.exists(a.note):
        lines.append(open(a.note).read().rstrip())
        lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
