"""What kinematic-wave routing costs on the device: noahmp_hip_route_kinematic with and without its depth plane and diag words, and -- in
the same run, on the same network -- noahmp_hip_route_runoff, a device-to-device copy of the bytes per cell the call moves, and
noahmp_hip_flow_channel.

    python tools/channel_bench.py [--reps 7] [--eps 1e-3] [--out profiles/channel_bench.md] [--json FILE] [--variant LIB]
    python tools/channel_bench.py --from-json profiles/channel_bench.json      re-renders the table from a saved run, without a GPU

Shapes: 4608 x 1536 (7 077 888 cells, the config-3 grid) and the 1152 x 768 tile of an 8-rank run (884 736 cells), 1 km spacing, the
synthetic terrain with about 2 km relief of tools/shadow_bench.py, filled (FlowNetwork.set_terrain(fill=eps)); width 20 m, n = 0.05, 60 s
per call (a celerity Courant number near 1 on this steep terrain: few cells are capped), storage between 0 and 5000 m3 so that nearly
every cell holds water and takes the powf.  Per shape, medians of --reps windows of 12 consecutive calls between two device events (launch gaps included), consecutive calls on DIFFERENT copies of their storage, out,
depth, width, length, conv, area and release planes (three sets), so that no call finds its planes in a cache the call before filled:
  kinematic             noahmp_hip_route_kinematic with depth and diag (49 B per cell by the field list);
  no depth, no diag     the same without both (45 B);  depth only / diag only: one of the two;
  600 s per call        the same with ten times the time step: about half the cells are capped, nearly every workgroup reports to
                        both diag words (the worst case for the two atomics);
  variant               the same call of the library given with --variant (built with -DNMP_CHANNEL_PIN=0: no scheduling barrier between
                        the loads and the arithmetic), when given;
  route_runoff          noahmp_hip_route_runoff on the same network (37 B);
  copy 45 / 49          a device-to-device copy of that many bytes per cell (half read, half written);
  flow_channel          noahmp_hip_flow_channel from the filled heights (once per terrain).
Before anything is timed: three calls from the same start with and without depth and diag give the same storage and out words; the
celerity Courant number and the capped count after them are reported.  Nothing else is enforced.  A process of its own: start it
under `timeout -k 10 ...`.  Without a GPU it fails.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_PINNED_MIN_XFER_SIZE", "1048576")

from tools.shadow_bench import terrain, DX  # noqa: E402

BYTES = 45               # inmask 1, col_index 4, area 4, width 4, length 4, conv 4, storage 4 + 4, out_old 4, out_new 4, runoff_a 4, runoff_b 4
BYTES_DEPTH = 49
BYTES_RUNOFF = 37        # release 4 instead of width, length and conv
NSET, WINDOW, DT = 3, 12, 60.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--eps", type=float, default=1e-3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "channel_bench.md"))
    ap.add_argument("--json", default=None)
    ap.add_argument("--variant", default=None, help="a library built with -DNMP_CHANNEL_PIN=0, timed next to the default one")
    ap.add_argument("--from-json", default=None, help="re-render --out from a saved --json file; needs no GPU")
    a = ap.parse_args()
    if a.from_json:
        saved = json.load(open(a.from_json))
        with open(a.out, "w") as fh:
            fh.write(render(saved["results"], saved["device"], saved["eps"], saved["reps"]))
        print("wrote", a.out)
        return
    import torch
    from noahmp_amd.driver import Engine
    from noahmp_amd.routing import ChannelFlow, FlowNetwork
    from noahmp_amd.tables import load_tables
    if not torch.cuda.is_available():
        raise SystemExit("channel_bench: no GPU -- nothing to measure")
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
        zd = torch.from_numpy(terrain(ni, nj)).cuda()
        net = FlowNetwork(eng, ni, nj)
        net.set_terrain(zd, DX, DX, fill=a.eps)
        net.set_input_columns(None)
        ch = ChannelFlow(net)
        ch.set_geometry(20.0, 0.05)
        g = torch.Generator(device="cpu")
        g.manual_seed(ni)
        rnd = lambda lo, hi, shape: (lo + (hi - lo) * torch.rand(shape, generator=g)).cuda()      # noqa: E731
        ra, rb = rnd(0.0, 2e-3, (ncell,)), rnd(0.0, 1e-3, (ncell,))
        start = rnd(0.0, 5e3, (nj, ni))
        release = rnd(0.0, 1.0, (nj, ni))
        sets = []
        for _ in range(NSET):
            sets.append(dict(storage=start.clone(), out=[torch.zeros_like(start), torch.zeros_like(start)], depth=torch.zeros_like(start),
                             diag=torch.zeros(2, dtype=torch.int32, device="cuda"), area=net.area.clone(), width=ch.width.clone(),
                             length=ch.length.clone(), conv=ch.conv.clone(), release=release.clone(), inmask=net.inmask.clone(),
                             col=net.col_index.clone()))
        scale = DT * 1e-3

        def kblocks(e, depth, diag, dt=DT):
            return [[e.route_kinematic_block(s["inmask"], s["col"], s["area"], s["width"], s["length"], s["conv"], s["storage"], s["out"][k],
                                             s["out"][1 - k], ra, rb, dt * 1e-3, dt, depth=s["depth"] if depth else None,
                                             diag=s["diag"] if diag else None) for k in (0, 1)] for s in sets]

        def rblocks():
            return [[eng.route_block(s["inmask"], s["col"], s["area"], s["release"], s["storage"], s["out"][k], s["out"][1 - k], ra, rb, scale)
                     for k in (0, 1)] for s in sets]

        def reset():
            for s in sets:
                s["storage"].copy_(start)
                for o in s["out"]:
                    o.zero_()
                s["diag"].zero_()
            torch.cuda.synchronize()

        # ---- the check: depth and diag change no word of storage and out
        words = {}
        for depth, diag in ((True, True), (False, False)):
            reset()
            bl = kblocks(eng, depth, diag)
            for n in range(3):
                eng.route_kinematic(bl[0][n & 1], ncell, stream=sh)
            torch.cuda.synchronize()
            words[depth] = (sets[0]["storage"].clone(), sets[0]["out"][1].clone())
            if diag:
                w = sets[0]["diag"].cpu().numpy().view("uint32")
                courant, capped = 5.0 / 3.0 * float(w[:1].view("float32")[0]), int(w[1])
        if not (torch.equal(words[True][0].view(torch.int32), words[False][0].view(torch.int32)) and
                torch.equal(words[True][1].view(torch.int32), words[False][1].view(torch.int32))):
            raise SystemExit("channel_bench: depth and diag change the planes (%s)" % cname)

        def window_of(call, blocks):
            def go():
                for n in range(WINDOW):
                    call(blocks[n % NSET][(n // NSET) & 1], ncell, stream=sh)
            return go

        cases = [("kinematic", eng.route_kinematic, kblocks(eng, True, True)), ("bare", eng.route_kinematic, kblocks(eng, False, False)),
                 ("depth_only", eng.route_kinematic, kblocks(eng, True, False)), ("diag_only", eng.route_kinematic, kblocks(eng, False, True)),
                 ("runoff", eng.route_runoff, rblocks()), ("capped", eng.route_kinematic, kblocks(eng, True, True, 10 * DT))]
        if var is not None:
            cases.append(("variant", var.route_kinematic, kblocks(var, True, True)))
        ms = {k: [] for k, _, _ in cases}
        for _ in range(a.reps):                                          # alternating: every repetition times every case once
            for k, call, blocks in cases:
                reset()
                ms[k].append(timed(window_of(call, blocks)) / WINDOW)
        row = dict(case=cname, ni=ni, nj=nj, courant=courant, capped=capped, fill_calls=net.fill_calls)
        row.update({k + "_ms": med(v) for k, v in ms.items()})
        for nbytes in (BYTES, BYTES_DEPTH, BYTES_RUNOFF):
            half = nbytes * ncell // 2
            src = [torch.zeros(half, dtype=torch.uint8, device="cuda") for _ in range(NSET)]
            dst = [torch.empty(half, dtype=torch.uint8, device="cuda") for _ in range(NSET)]

            def copy():
                for n in range(WINDOW):
                    dst[n % NSET].copy_(src[n % NSET])
            row["copy%d_ms" % nbytes] = med([timed(copy) / WINDOW for _ in range(a.reps)])
            del src, dst
        hs = [net.filled.clone() for _ in range(NSET)]
        gb = [eng.flow_channel_block(net.dir, ch.manning, s["length"], s["conv"], DX, DX, 1e-4, height=hs[n]) for n, s in enumerate(sets)]

        def geom():
            for n in range(WINDOW):
                eng.flow_channel(gb[n % NSET], stream=sh)
        row["flow_channel_ms"] = med([timed(geom) / WINDOW for _ in range(a.reps)])
        results.append(row)
        print(row, flush=True)
        del sets, hs, gb, net, ch

    text = render(results, torch.cuda.get_device_name(0), a.eps, a.reps)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(dict(device=torch.cuda.get_device_name(0), eps=a.eps, reps=a.reps, results=results), fh, indent=1)
    print("wrote", a.out)


def render(results, device, eps, reps):
    """The text of profiles/channel_bench.md from the results (also from a saved --json: --from-json re-renders without a GPU)."""
    o = ["# Kinematic-wave routing against the linear reservoirs and a copy", "",
         "Written by `tools/channel_bench.py` (its docstring says what every column is) on %s, one device, filled terrain (fill eps = %g m), "
         "width 20 m, n = 0.05, %g s per call, medians of %d windows of %d consecutive calls on %d rotating sets of planes, the cases "
         "alternating.  Device milliseconds span back-to-back launches, launch gaps included." % (device, eps, DT, reps, WINDOW, NSET), "",
         "| cells | `route_kinematic` ms (depth + diag, %d B) | no depth, no diag (%d B) | depth only | diag only | `route_runoff` ms (%d B) | "
         "copy %d B ms | copy %d B ms | kinematic / copy %d | bare / copy %d | kinematic / `route_runoff` | `flow_channel` ms |"
         % (BYTES_DEPTH, BYTES, BYTES_RUNOFF, BYTES, BYTES_DEPTH, BYTES_DEPTH, BYTES), "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in results:
        o.append("| %s | %.4f | %.4f | %.4f | %.4f | %.4f | %.4f | %.4f | %.2f | %.2f | %.2f | %.4f |"
                 % (r["case"], r["kinematic_ms"], r["bare_ms"], r["depth_only_ms"], r["diag_only_ms"], r["runoff_ms"], r["copy%d_ms" % BYTES],
                    r["copy%d_ms" % BYTES_DEPTH], r["kinematic_ms"] / r["copy%d_ms" % BYTES_DEPTH], r["bare_ms"] / r["copy%d_ms" % BYTES],
                    r["kinematic_ms"] / r["runoff_ms"], r["flow_channel_ms"]))
    o += ["", "`route_runoff` against a copy of its own %d B per cell: %s." % (
        BYTES_RUNOFF, ", ".join("%.2f" % (r["runoff_ms"] / r["copy%d_ms" % BYTES_RUNOFF]) for r in results)), ""]
    if all("variant_ms" in r for r in results):
        o += ["The scheduling barrier between the loads of a cell and its arithmetic (`NMP_CHANNEL_PIN`, the library's default is 1): with it "
              "%s ms, without it (the variant library) %s ms, in the same alternation." % (
                  " / ".join("%.4f" % r["kinematic_ms"] for r in results), " / ".join("%.4f" % r["variant_ms"] for r in results)), ""]
    else:
        o += ["*UNMEASURED:* the build without the scheduling barrier (`-DNMP_CHANNEL_PIN=0`).", ""]
    o += ["With %g s per call, where about half the cells are capped and nearly every workgroup reports to both diag words: %s ms with depth "
          "and diag." % (10 * DT, " / ".join("%.4f" % r["capped_ms"] for r in results)), ""]
    o += ["After three calls from the start state: %s." % "; ".join(
        "%s: celerity Courant number %.3g, %d capped cells" % (r["case"].split(" (")[0], r["courant"], r["capped"]) for r in results),
        "*UNMEASURED:* a decomposed run over several processes with the real exchange.", "", ""]
    return "\n".join(o)


if __name__ == "__main__":
    main()
