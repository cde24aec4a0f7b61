"""What the lakes cost on the device: noahmp_hip_lake_take + noahmp_hip_lake_release after a routing launch, and -- in the same run, on
the same network -- noahmp_hip_route_kinematic, a device-to-device copy of the bytes the take moves, and the take of the library built
with -DNMP_LAKES_PER_LANE=1 (every lane sends its own atomic).

    python tools/lakes_bench.py [--reps 7] [--eps 1e-3] [--min-depth 1.0] [--out profiles/lakes_bench.md] [--json FILE] [--variant LIB]
    python tools/lakes_bench.py --from-json profiles/lakes_bench.json      re-renders the table from a saved run, without a GPU

Shapes: 4608 x 1536 (7 077 888 cells, the config-3 grid) and the 1152 x 768 tile of an 8-rank run (884 736 cells), 1 km spacing, the
synthetic terrain with about 2 km relief of tools/shadow_bench.py, filled (FlowNetwork.set_terrain(fill=eps)).  Two inputs per shape:
  from_fill   the lakes Lakes.from_fill finds (filled - raw >= --min-depth, at least 4 cells), outlets by the upstream count, through
              Lakes.set_lakes: the list sorted by lake, every lake padded to whole waves;
  one lake    the worst case for the atomics: ONE lake of 1/16 of all cells (the first rows of the window).
Every member holds between 0 and 5000 m3 before every timed take (the storage planes are copied back between the windows), so every
entry takes something.  Medians of --reps windows of 6 consecutive calls between two device events (launch gaps included), each
call of a window on ANOTHER copy of storage, inflow, volume and out (six sets):
  pair          take then release, as the hook of routing.Lakes enqueues them;     take / release: one of the two alone;
  per lane      the take of the --variant library;
  kinematic     noahmp_hip_route_kinematic with depth and diag on the same network, 60 s per call;
  copy          a device-to-device copy of 16 B per list entry, half read, half written (member_cell 4, member_lake 4, storage 4 + 4).
Before anything is timed the two libraries' takes give the same inflow words from the same start.  A process of its own: start it under
`timeout -k 10 ...`.  Without a GPU it fails.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_PINNED_MIN_XFER_SIZE", "1048576")

from tools.shadow_bench import terrain, DX  # noqa: E402

NSET, WINDOW, DT, Q = 6, 6, 60.0, 2.0 ** -10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--eps", type=float, default=1e-3)
    ap.add_argument("--min-depth", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lakes_bench.md"))
    ap.add_argument("--json", default=None)
    ap.add_argument("--variant", default=None, help="a library built with -DNMP_LAKES_PER_LANE=1, timed next to the default one")
    ap.add_argument("--from-json", default=None, help="re-render --out from a saved --json file; needs no GPU")
    a = ap.parse_args()
    if a.from_json:
        saved = json.load(open(a.from_json))
        with open(a.out, "w") as fh:
            fh.write(render(saved["results"], saved["device"], saved["eps"], saved["min_depth"], saved["reps"]))
        print("wrote", a.out)
        return
    import torch
    from noahmp_amd.driver import Engine
    from noahmp_amd.routing import ChannelFlow, FlowNetwork, Lakes, Upstream, LAKE_PARAMS
    from noahmp_amd.tables import load_tables
    if not torch.cuda.is_available():
        raise SystemExit("lakes_bench: no GPU -- nothing to measure")
    T = load_tables("usgs")[0]
    eng = Engine(T, device=0)
    var = Engine(T, lib_path=a.variant) if a.variant else None
    stream = torch.cuda.Stream()
    sh = stream.cuda_stream
    med = statistics.median
    results = []

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            e0.record()
            fn()
            e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for cname, ni, nj in (("7 077 888 cells (4608 x 1536)", 4608, 1536), ("884 736 cells (1152 x 768)", 1152, 768)):
        ncell = ni * nj
        z = terrain(ni, nj)
        net = FlowNetwork(eng, ni, nj)
        net.set_terrain(torch.from_numpy(z).cuda(), DX, DX, fill=a.eps)
        net.set_input_columns(None)
        ch = ChannelFlow(net)
        ch.set_geometry(20.0, 0.05)
        up = Upstream(net).cells().cpu().numpy()
        lake_id, outlet_ij, area = Lakes.from_fill(z, net.filled.cpu().numpy(), up, a.min_depth, min_cells=4, cell_area=DX * DX)
        nlake = int(area.size)
        par = dict(area=area, weir_h=np.full(nlake, 0.5), weir_c=np.full(nlake, 1.7), weir_l=np.full(nlake, 20.0), orifice_h=np.zeros(nlake),
                   orifice_c=np.full(nlake, 0.6), orifice_a=np.full(nlake, 1.0))
        lakes = Lakes(ch)
        lakes.set_lakes(lake_id, par, outlet_ij)
        counts = np.bincount(lake_id[lake_id > 0] - 1, minlength=nlake)
        g = torch.Generator(device="cpu")
        g.manual_seed(ni)
        rnd = lambda lo, hi, shape: (lo + (hi - lo) * torch.rand(shape, generator=g)).cuda()      # noqa: E731
        ra, rb = rnd(0.0, 2e-3, (ncell,)), rnd(0.0, 1e-3, (ncell,))
        start = rnd(0.0, 5e3, (nj, ni))
        big = ncell // 16
        one = dict(mc=torch.arange(big, dtype=torch.int32, device="cuda"), ml=torch.zeros(big, dtype=torch.int32, device="cuda"), nlake=1,
                   par={k: torch.tensor([v], dtype=torch.float64, device="cuda") for k, v in
                        zip(LAKE_PARAMS, (big * DX * DX, 0.5, 1.7, 20.0, 0.0, 0.6, 1.0))},
                   oc=torch.tensor([big - 1], dtype=torch.int32, device="cuda"))
        found = dict(mc=lakes.member_cell, ml=lakes.member_lake, nlake=nlake, par=lakes.params, oc=lakes.outlet_cell)
        sets = [dict(storage=start.clone(), out=[torch.zeros_like(start), torch.zeros_like(start)], depth=torch.zeros_like(start),
                     diag=torch.zeros(2, dtype=torch.int32, device="cuda")) for _ in range(NSET)]
        row = dict(case=cname, ni=ni, nj=nj, nlake=nlake, members=int(counts.sum()), largest=int(counts.max()) if nlake else 0,
                   entries=int(lakes.member_cell.numel()), one_lake_members=big, fill_calls=net.fill_calls)

        def reset():
            for s in sets:
                s["storage"].copy_(start)
            torch.cuda.synchronize()

        for iname, inp in (("found", found), ("one", one)):
            if inp["nlake"] == 0:
                continue
            words = [dict(volume=torch.zeros(inp["nlake"], dtype=torch.int64, device="cuda"), inflow=torch.zeros(inp["nlake"], dtype=torch.int64, device="cuda"),
                          diag=torch.zeros(1, dtype=torch.int32, device="cuda")) for _ in range(NSET)]
            tb = {e: [e.lake_take_block(inp["mc"], inp["ml"], s["storage"], w["inflow"], Q) for s, w in zip(sets, words)] for e in (eng, var) if e}
            rbk = [eng.lake_release_block(w["volume"], w["inflow"], inp["par"], inp["oc"], s["out"][0], Q, DT, diag=w["diag"]) for s, w in zip(sets, words)]
            # ---- the check: both forms of the take give the same words
            got = {}
            for e in tb:
                reset()
                words[0]["inflow"].zero_()
                torch.cuda.synchronize()
                e.lake_take(tb[e][0], stream=sh)
                torch.cuda.synchronize()
                got[e] = (words[0]["inflow"].clone(), sets[0]["storage"].clone())
            if var and not (torch.equal(got[eng][0], got[var][0]) and torch.equal(got[eng][1].view(torch.int32), got[var][1].view(torch.int32))):
                raise SystemExit("lakes_bench: the two forms of the take differ (%s, %s)" % (cname, iname))
            row[iname + "_quanta"] = int(got[eng][0].sum().item())

            def pair():
                for n in range(WINDOW):
                    eng.lake_take(tb[eng][n % NSET], stream=sh)
                    eng.lake_release(rbk[n % NSET], stream=sh)

            def take(e):
                def go():
                    for n in range(WINDOW):
                        e.lake_take(tb[e][n % NSET], stream=sh)
                return go

            def release():
                for n in range(WINDOW):
                    eng.lake_release(rbk[n % NSET], stream=sh)

            cases = [("pair", pair), ("take", take(eng)), ("release", release)] + ([("per_lane", take(var))] if var else [])
            ms = {k: [] for k, _ in cases}
            for _ in range(a.reps):                                      # alternating: every repetition times every case once
                for k, fn in cases:
                    reset()
                    ms[k].append(timed(fn) / WINDOW)
            row.update({"%s_%s_ms" % (iname, k): med(v) for k, v in ms.items()})
            half = 8 * int(inp["mc"].numel())
            src = [torch.zeros(half, dtype=torch.uint8, device="cuda") for _ in range(NSET)]
            dst = [torch.empty(half, dtype=torch.uint8, device="cuda") for _ in range(NSET)]

            def copy():
                for n in range(WINDOW):
                    dst[n % NSET].copy_(src[n % NSET])
            row[iname + "_copy_ms"] = med([timed(copy) / WINDOW for _ in range(a.reps)])
            del src, dst, words, tb, rbk
        kb = [[eng.route_kinematic_block(net.inmask, net.col_index, net.area, ch.width, ch.length, ch.conv, s["storage"], s["out"][k], s["out"][1 - k],
                                         ra, rb, DT * 1e-3, DT, depth=s["depth"], diag=s["diag"]) for k in (0, 1)] for s in sets]

        def kinematic():
            for n in range(WINDOW):
                eng.route_kinematic(kb[n % NSET][0], ncell, stream=sh)
        kms = []
        for _ in range(a.reps):
            reset()
            kms.append(timed(kinematic) / WINDOW)
        row["kinematic_ms"] = med(kms)
        results.append(row)
        print(row, flush=True)
        del sets, kb, net, ch, lakes

    text = render(results, torch.cuda.get_device_name(0), a.eps, a.min_depth, a.reps)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(dict(device=torch.cuda.get_device_name(0), eps=a.eps, min_depth=a.min_depth, reps=a.reps, results=results), fh, indent=1)
    print("wrote", a.out)


def render(results, device, eps, min_depth, reps):
    """The text of profiles/lakes_bench.md from the results (also from a saved --json: --from-json re-renders without a GPU)."""
    f = lambda r, k: ("%.4f" % r[k]) if k in r else "unmeasured"      # noqa: E731
    o = ["# Lakes: take + release against the kinematic wave and a copy", "",
         "Written by `tools/lakes_bench.py` (its docstring says what every column is) on %s, one device, filled terrain (fill eps = %g m), lakes "
         "where filled - raw >= %g m with at least 4 cells, quantum 2^-10 m3, %g s per call, medians of %d windows of %d consecutive calls on %d "
         "rotating sets of planes, the cases alternating.  Device milliseconds span back-to-back launches, launch gaps included."
         % (device, eps, min_depth, DT, reps, WINDOW, NSET), "",
         "| cells | input | lakes | members (share of cells) | largest lake | list entries | take + release ms | take ms | release ms | take, per-lane atomics ms | "
         "copy 16 B per entry ms | `route_kinematic` ms | pair / `route_kinematic` |", "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in results:
        for iname, label, nl, mem, largest, entries in (("found", "from_fill", r["nlake"], r["members"], r["largest"], r["entries"]),
                                                        ("one", "one lake of 1/16", 1, r["one_lake_members"], r["one_lake_members"], r["one_lake_members"])):
            if iname + "_pair_ms" not in r:
                o.append("| %s | %s | %d | no lakes found | | | | | | | | %s | |" % (r["case"], label, nl, f(r, "kinematic_ms")))
                continue
            o.append("| %s | %s | %d | %d (%.2f %%) | %d | %d | %s | %s | %s | %s | %s | %s | %.2f |"
                     % (r["case"], label, nl, mem, 100.0 * mem / (r["ni"] * r["nj"]), largest, entries, f(r, iname + "_pair_ms"), f(r, iname + "_take_ms"),
                        f(r, iname + "_release_ms"), f(r, iname + "_per_lane_ms"), f(r, iname + "_copy_ms"), f(r, "kinematic_ms"),
                        r[iname + "_pair_ms"] / r["kinematic_ms"]))
    o += ["", "Quanta taken by one take from the start state: %s." % "; ".join(
        "%s: %s" % (r["case"].split(" (")[0], ", ".join("%s %d" % (k, r[k + "_quanta"]) for k in ("found", "one") if k + "_quanta" in r)) for r in results), ""]
    if not all(("one_per_lane_ms" in r) for r in results):
        o += ["*UNMEASURED:* the take with per-lane atomics (`-DNMP_LAKES_PER_LANE=1`).", ""]
    o += ["*UNMEASURED:* a decomposed run over several processes with the real exchange and the sum of the inflow words over the ranks.", "", ""]
    return "\n".join(o)


if __name__ == "__main__":
    main()
