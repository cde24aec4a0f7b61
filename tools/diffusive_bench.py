"""What diffusive-wave routing costs on the device: noahmp_hip_route_diffusive with and without its diag words and in both forms of the
downstream-depth access, and -- in the same run, on the same network -- noahmp_hip_route_kinematic, a device-to-device copy of the
bytes per cell the diffusive call moves, noahmp_hip_flow_drop and noahmp_hip_lake_depth.

    python tools/diffusive_bench.py [--reps 7] [--eps 1e-3] [--out profiles/diffusive_bench.md] [--json FILE] [--variant LIB]
    python tools/diffusive_bench.py --from-json profiles/diffusive_bench.json      re-renders the table from a saved run, without a GPU

Shapes, terrain, widths, n, the 60 s per call, the start storage and the timing scheme (medians of --reps windows of 12 consecutive calls
between two device events, launch gaps included, on three rotating sets of planes, the cases alternating) are those of
tools/channel_bench.py.  The depth planes start as storage / (width * length), the depth the start state has.
  diffusive             noahmp_hip_route_diffusive with diag (62 B per cell by the field list: the 45 B of the kinematic call, dir 1,
                        manning 4, drop 4, depth_old 4, depth_new 4);
  no diag               the same without the four words -- the figure the ratios are made from: on this start state about half the
                        cells are blocked, so with diag nearly every workgroup sends an atomic to the same word (the worst case);
  variant               the same call of the library given with --variant: the OTHER form of the downstream-depth access (the library's
                        own form is NMP_DIFFUSIVE_LOAD_ALL in noahmp_diffusive.hip; 0: one dependent load, 1: eight loads and a select);
  kinematic             noahmp_hip_route_kinematic without depth and diag on the same network (45 B);
  copy 62               a device-to-device copy of 62 B per cell (half read, half written);
  flow_drop             noahmp_hip_flow_drop from the filled heights (once per terrain);
  lake_depth            noahmp_hip_lake_depth on the lakes Lakes.from_fill finds (filled - raw >= --min-depth, at least 4 cells), the
                        list of Lakes.set_lakes (sorted by lake, padded to whole waves), after set_volume_m3 at the mean depth.
Before anything is timed: three calls from the same start with and without diag, and of the variant, give the same storage, out and depth
words; the celerity Courant number and the capped / limited / blocked counts after them are reported.  Nothing else is enforced.  A
process of its own: start it under `timeout -k 10 ...`.  Without a GPU it fails.
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

BYTES = 62               # the 45 of route_kinematic (tools/channel_bench.py), dir 1, manning 4, drop 4, depth_old 4, depth_new 4
BYTES_KIN = 45
NSET, WINDOW, DT, LIMIT = 3, 12, 60.0, 0.5
ISA = dict(diffusive_dependent=dict(vgpr=44, scratch=0, lds=576, waves=8), diffusive_load_all=dict(vgpr=60, scratch=0, lds=576, waves=8),
           flow_drop=dict(vgpr=12, scratch=0, lds=0, waves=8), lake_depth=dict(vgpr=18, scratch=0, lds=0, waves=8))      # from the gfx950 ISA of the build


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--eps", type=float, default=1e-3)
    ap.add_argument("--min-depth", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diffusive_bench.md"))
    ap.add_argument("--json", default=None)
    ap.add_argument("--variant", default=None, help="a library built with the other NMP_DIFFUSIVE_LOAD_ALL, timed next to the default one")
    ap.add_argument("--default-form", default="dependent", choices=("dependent", "load_all"), help="the form the default library was built with")
    ap.add_argument("--from-json", default=None, help="re-render --out from a saved --json file; needs no GPU")
    a = ap.parse_args()
    if a.from_json:
        saved = json.load(open(a.from_json))
        with open(a.out, "w") as fh:
            fh.write(render(saved))
        print("wrote", a.out)
        return
    import torch
    from noahmp_amd.driver import Engine
    from noahmp_amd.routing import DiffusiveFlow, FlowNetwork, Lakes, Upstream
    from noahmp_amd.tables import load_tables
    if not torch.cuda.is_available():
        raise SystemExit("diffusive_bench: no GPU -- nothing to measure")
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
        df = DiffusiveFlow(net)
        df.set_geometry(20.0, 0.05, limit=LIMIT)
        g = torch.Generator(device="cpu")
        g.manual_seed(ni)
        rnd = lambda lo, hi, shape: (lo + (hi - lo) * torch.rand(shape, generator=g)).cuda()      # noqa: E731
        ra, rb = rnd(0.0, 2e-3, (ncell,)), rnd(0.0, 1e-3, (ncell,))
        start = rnd(0.0, 5e3, (nj, ni))
        depth0 = start / (df.width * df.length)
        sets = []
        for _ in range(NSET):
            sets.append(dict(storage=start.clone(), out=[torch.zeros_like(start), torch.zeros_like(start)], depth=[depth0.clone(), depth0.clone()],
                             diag=torch.zeros(4, dtype=torch.int32, device="cuda"), area=net.area.clone(), width=df.width.clone(),
                             length=df.length.clone(), conv=df.conv.clone(), manning=df.manning.clone(), drop=df.drop.clone(),
                             inmask=net.inmask.clone(), dir=net.dir.clone(), col=net.col_index.clone()))

        def dblocks(e, diag):
            return [[e.route_diffusive_block(s["inmask"], s["col"], s["dir"], s["area"], s["width"], s["length"], s["conv"], s["manning"], s["drop"],
                                             s["storage"], s["out"][k], s["out"][1 - k], ra, rb, s["depth"][k], s["depth"][1 - k], DT * 1e-3, DT,
                                             limit=LIMIT, diag=s["diag"] if diag else None) for k in (0, 1)] for s in sets]

        def kblocks():
            return [[eng.route_kinematic_block(s["inmask"], s["col"], s["area"], s["width"], s["length"], s["conv"], s["storage"], s["out"][k],
                                               s["out"][1 - k], ra, rb, DT * 1e-3, DT) for k in (0, 1)] for s in sets]

        def reset():
            for s in sets:
                s["storage"].copy_(start)
                for o in s["out"]:
                    o.zero_()
                for h in s["depth"]:
                    h.copy_(depth0)
                s["diag"].zero_()
            torch.cuda.synchronize()

        # ---- the check: diag and the form of the downstream-depth access change no word of storage, out and depth
        words = []
        for e, diag in ((eng, True), (eng, False)) + (((var, True),) if var is not None else ()):
            reset()
            bl = dblocks(e, diag)
            for n in range(3):
                e.route_diffusive(bl[0][n & 1], ncell, stream=sh)
            torch.cuda.synchronize()
            words.append(tuple(t.clone().view(torch.int32) for t in (sets[0]["storage"], sets[0]["out"][1], sets[0]["depth"][1])))
            if e is eng and diag:
                w = sets[0]["diag"].cpu().numpy().view("uint32")
                courant, counts = 5.0 / 3.0 * float(w[:1].view("float32")[0]), [int(v) for v in w[1:]]
        for other in words[1:]:
            if not all(torch.equal(x, y) for x, y in zip(words[0], other)):
                raise SystemExit("diffusive_bench: diag or the variant changes the planes (%s)" % cname)

        def window_of(call, blocks):
            def go():
                for n in range(WINDOW):
                    call(blocks[n % NSET][(n // NSET) & 1], ncell, stream=sh)
            return go

        cases = [("diffusive", eng.route_diffusive, dblocks(eng, True)), ("bare", eng.route_diffusive, dblocks(eng, False)),
                 ("kinematic", eng.route_kinematic, kblocks())]
        if var is not None:
            cases += [("variant", var.route_diffusive, dblocks(var, True)), ("variant_bare", var.route_diffusive, dblocks(var, False))]
        ms = {k: [] for k, _, _ in cases}
        for _ in range(a.reps):                                          # alternating: every repetition times every case once
            for k, call, blocks in cases:
                reset()
                ms[k].append(timed(window_of(call, blocks)) / WINDOW)
        row = dict(case=cname, ni=ni, nj=nj, courant=courant, capped=counts[0], limited=counts[1], blocked=counts[2], fill_calls=net.fill_calls)
        row.update({k + "_ms": med(v) for k, v in ms.items()})
        for nbytes in (BYTES, BYTES_KIN):
            half = nbytes * ncell // 2
            src = [torch.zeros(half, dtype=torch.uint8, device="cuda") for _ in range(NSET)]
            dst = [torch.empty(half, dtype=torch.uint8, device="cuda") for _ in range(NSET)]

            def copy():
                for n in range(WINDOW):
                    dst[n % NSET].copy_(src[n % NSET])
            row["copy%d_ms" % nbytes] = med([timed(copy) / WINDOW for _ in range(a.reps)])
            del src, dst
        hs = [net.filled.clone() for _ in range(NSET)]
        gb = [eng.flow_drop_block(net.dir, s["drop"], DX, DX, height=hs[n]) for n, s in enumerate(sets)]

        def geom():
            for n in range(WINDOW):
                eng.flow_drop(gb[n % NSET], stream=sh)
        row["flow_drop_ms"] = med([timed(geom) / WINDOW for _ in range(a.reps)])
        # ---- the lake's stage on the lakes of the fill
        filled = net.filled.cpu().numpy()
        up = Upstream(net).cells().cpu().numpy()
        lake_id, outlet_ij, area = Lakes.from_fill(z, filled, up, a.min_depth, min_cells=4, cell_area=DX * DX)
        nlake = int(area.size)
        par = dict(area=area, weir_h=np.full(nlake, 0.5), weir_c=np.full(nlake, 1.7), weir_l=np.full(nlake, 20.0), orifice_h=np.zeros(nlake),
                   orifice_c=np.full(nlake, 0.6), orifice_a=np.full(nlake, 1.0))
        lakes = Lakes(df)
        lakes.set_lakes(lake_id, par, outlet_ij)
        datum = Lakes.datum_from_fill(z, filled, lake_id)
        lakes.set_datum(datum)
        member = lake_id > 0
        mean_depth = np.bincount(lake_id[member] - 1, weights=(filled - z)[member], minlength=nlake) / np.maximum(area / (DX * DX), 1.0)
        lakes.set_volume_m3(mean_depth * area)
        lb = [eng.lake_depth_block(lakes.member_cell, lakes.member_lake, lakes.volume, lakes.params["area"], lakes.datum, hs[n], s["depth"][0],
                                   lakes.quantum) for n, s in enumerate(sets)]

        def stage():
            for n in range(WINDOW):
                eng.lake_depth(lb[n % NSET], stream=sh)
        row["lake_depth_ms"] = med([timed(stage) / WINDOW for _ in range(a.reps)]) if nlake else 0.0
        row.update(nlake=nlake, members=int((lake_id > 0).sum()), entries=int(lakes.member_cell.numel()))
        results.append(row)
        print(row, flush=True)
        del sets, hs, gb, lb, net, df, lakes

    saved = dict(device=torch.cuda.get_device_name(0), eps=a.eps, min_depth=a.min_depth, reps=a.reps, default_form=a.default_form, isa=ISA,
                 results=results)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(render(saved))
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(saved, fh, indent=1)
    print("wrote", a.out)


def render(saved):
    """The text of profiles/diffusive_bench.md from a saved run (--from-json re-renders without a GPU)."""
    results, form = saved["results"], saved["default_form"]
    other = "load_all" if form == "dependent" else "dependent"
    names = dict(dependent="one dependent load", load_all="eight loads and a select")
    o = ["# Diffusive-wave routing against the kinematic wave and a copy", "",
         "Written by `tools/diffusive_bench.py` (its docstring says what every column is) on %s, one device, filled terrain (fill eps = %g m), "
         "width 20 m, n = 0.05, limit %g, %g s per call, medians of %d windows of %d consecutive calls on %d rotating sets of planes, the cases "
         "alternating.  Device milliseconds span back-to-back launches, launch gaps included.  The library's form of the downstream-depth "
         "access is `%s` (%s)." % (saved["device"], saved["eps"], LIMIT, DT, saved["reps"], WINDOW, NSET, form, names[form]), "",
         "| cells | `route_diffusive` ms (no diag, %d B) | with diag | `route_kinematic` ms (no depth, no diag, %d B) | copy %d B ms | copy %d B ms | "
         "diffusive / copy %d | diffusive / `route_kinematic` | kinematic / copy %d | with diag / without | `flow_drop` ms | "
         "`lake_depth` ms (lakes, entries) |" % (BYTES, BYTES_KIN, BYTES, BYTES_KIN, BYTES, BYTES_KIN), "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in results:
        o.append("| %s | %.4f | %.4f | %.4f | %.4f | %.4f | %.2f | %.2f | %.2f | %.1f | %.4f | %.4f (%d, %d) |"
                 % (r["case"], r["bare_ms"], r["diffusive_ms"], r["kinematic_ms"], r["copy%d_ms" % BYTES], r["copy%d_ms" % BYTES_KIN],
                    r["bare_ms"] / r["copy%d_ms" % BYTES], r["bare_ms"] / r["kinematic_ms"], r["kinematic_ms"] / r["copy%d_ms" % BYTES_KIN],
                    r["diffusive_ms"] / r["bare_ms"], r["flow_drop_ms"], r["lake_depth_ms"], r["nlake"], r["entries"]))
    o += ["", "The ratios against the copy and against `route_kinematic` are those of the call WITHOUT diag, like the kinematic call next to it.  "
          "With diag the start state of this run is the worst case for the atomics: %s of the (cell, call) pairs of the first three calls are "
          "blocked (random storage on a filled terrain: many a surface slopes against its direction), so nearly every one of the %s workgroups "
          "of 256 cells holds a blocked cell and sends an "
          "`atomicAdd` to the SAME word, and same-address atomics serialise at the memory side (`noahmp_route_kinematic` with every workgroup "
          "reporting: 1.24 / 0.120 ms, `profiles/channel_bench.md`).  `DiffusiveFlow.report = False` runs the launches without diag."
          % (" / ".join("%.0f %%" % (100.0 * r["blocked"] / (3.0 * r["ni"] * r["nj"])) for r in results),
             " / ".join("%d" % ((r["ni"] * r["nj"] + 255) // 256) for r in results))]
    o.append("")
    if all("variant_ms" in r for r in results):
        o += ["The downstream depth `hd`, the one access whose address depends on `dir[c]`: `%s` (the library) %s ms with diag and %s ms without; "
              "`%s` (the variant library, %s) %s ms and %s ms, in the same alternation." % (
                  form, " / ".join("%.4f" % r["diffusive_ms"] for r in results), " / ".join("%.4f" % r["bare_ms"] for r in results), other, names[other],
                  " / ".join("%.4f" % r["variant_ms"] for r in results), " / ".join("%.4f" % r["variant_bare_ms"] for r in results)), ""]
    else:
        o += ["*UNMEASURED:* the other form of the downstream-depth access (`%s`)." % other, ""]
    isa = saved["isa"]
    o += ["From the gfx950 ISA: `route_diffusive` %d VGPRs with one dependent load and %d with eight loads and a select, %d B of LDS, no scratch; "
          "`flow_drop` %d and `lake_depth` %d VGPRs, no scratch, no LDS; all at %d waves per SIMD (at most 64 VGPRs)." % (
              isa["diffusive_dependent"]["vgpr"], isa["diffusive_load_all"]["vgpr"], isa["diffusive_dependent"]["lds"], isa["flow_drop"]["vgpr"],
              isa["lake_depth"]["vgpr"], isa["diffusive_dependent"]["waves"]), ""]
    o += ["After three calls from the start state: %s." % "; ".join(
        "%s: celerity Courant number %.3g, %d capped, %d limited, %d blocked cells" % (r["case"].split(" (")[0], r["courant"], r["capped"],
                                                                                      r["limited"], r["blocked"]) for r in results),
        "*UNMEASURED:* a decomposed run over several processes with the real exchange (out and depth in one call).", "", ""]
    return "\n".join(o)


if __name__ == "__main__":
    main()
