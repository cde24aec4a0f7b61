"""What delineating basins on the device costs: noahmp_hip_flow_basin_init, the doubling passes of noahmp_hip_flow_basin_jump to their fixed
point and noahmp_hip_flow_basin_resolve, and -- in the same run, on the same network -- the only traversal there was before,
FlowNetwork.upstream_cells (one Jacobi pass of noahmp_hip_flow_accumulate per cell of the longest flow path).

    python tools/basins_bench.py [--reps 5] [--eps 1e-3] [--sweeps 12] [--out profiles/basins_bench.md] [--json FILE]
    python tools/basins_bench.py --from-json profiles/basins_bench.json        re-renders the table from a saved run, without a GPU

Shapes: 4608 x 1536 (7 077 888 cells, the config-3 grid) and the 1152 x 768 tile of an 8-rank run (884 736 cells), 1 km spacing, the
synthetic terrain with about 2 km relief of tools/shadow_bench.py, raw (FlowNetwork.set_terrain) and filled (set_terrain(fill=eps)).
One gauge, at the cell with the largest upstream count.  Per shape and network:
  passes        doubling passes Basins.run made with the flag read after EVERY pass, the confirming one included, and the longest flow
                path in hops (hops.max());
  ms per pass   that many passes enqueued back to back between two device events, divided by their number (median of --reps): launch
                gaps included;
  init, resolve one launch each, the mean of a window of 10 (both are idempotent), median of --reps;
  total         init + the passes + resolve, device ms; run() wall: Basins.run() with its defaults (the first call tiled, a batch of
                passes per host wait);
  tiled         the same with the tiled form of the pass (sweeps = --sweeps in-tile iterations) as the FIRST call only and as EVERY call:
                calls to the fixed point and their device ms;
  upstream      passes FlowNetwork.upstream_cells made (flag read every 64) x the mean ms of one noahmp_hip_flow_accumulate pass in a window
                of 20, and the wall time of the call.
Before anything is timed, at full size: the cells labelled with the gauge are as many as its upstream count says, no cell is PENDING or
CYCLE, and passes == ceil(log2 max(hops.max(), 1)) + 1.  Nothing else is enforced.
A process of its own: start it under `timeout -k 10 ...`.  Without a GPU it fails (there is nothing to measure on a CPU).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_PINNED_MIN_XFER_SIZE", "1048576")

from tools.shadow_bench import terrain, DX  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--eps", type=float, default=1e-3)
    ap.add_argument("--sweeps", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "basins_bench.md"))
    ap.add_argument("--json", default=None)
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
    from noahmp_amd.routing import Basins, FlowNetwork
    from noahmp_amd.tables import load_tables
    if not torch.cuda.is_available():
        raise SystemExit("basins_bench: no GPU -- nothing to measure")
    eng = Engine(load_tables("usgs")[0], device=0)
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
        zd = torch.from_numpy(terrain(ni, nj)).cuda()
        for kind, fill in (("raw", None), ("filled", a.eps)):
            net = FlowNetwork(eng, ni, nj)
            net.set_terrain(zd, DX, DX, fill=fill)
            # ---- the figure to beat
            t0 = time.perf_counter()
            acc = net.upstream_cells(max_pass=ni * nj)
            up_s = time.perf_counter() - t0
            up_passes = net.passes
            two = [torch.ones((nj, ni), dtype=torch.int32, device="cuda"), torch.ones((nj, ni), dtype=torch.int32, device="cuda")]
            flag = torch.zeros(1, dtype=torch.int32, device="cuda")

            def accumulate():
                for n in range(20):
                    eng.flow_accumulate(net.inmask, two[n & 1], two[1 - (n & 1)], flag, stream=sh)
            acc_ms = med([timed(accumulate) / 20 for _ in range(a.reps)])
            top = int(acc.view(-1).argmax().item())
            largest = int(acc.view(-1)[top].item())
            # ---- the result and the exact pass count first
            b = Basins(net)
            b.set_gauges([(top % ni, top // ni)])
            b.run(check=1, sweeps=1)
            passes, longest = b.passes, int(b.hops.max().item())
            members = int((b.label == 0).sum().item())
            if members != largest:
                raise SystemExit("basins_bench: %d cells labelled with the gauge, its upstream count is %d (%s, %s)" % (members, largest, cname, kind))
            if b.unresolved() != (0, 0):
                raise SystemExit("basins_bench: unresolved cells %s (%s, %s)" % (b.unresolved(), cname, kind))
            if passes != (max(longest, 1) - 1).bit_length() + 1:
                raise SystemExit("basins_bench: %d passes for a longest path of %d hops (%s, %s)" % (passes, longest, cname, kind))
            want = (b.label.clone(), b.hops.clone())
            # ---- timed
            pass_ms, run_ms = [], []
            for _ in range(a.reps):
                b.begin()
                blocks = [b._block(cur, 0) for cur in (0, 1)]               # made before the clock starts

                def go():
                    for n in range(passes):
                        eng.flow_basin_jump(blocks[n & 1], stream=sh)
                pass_ms.append(timed(go))
                t0 = time.perf_counter()
                b.run()
                run_ms.append(1e3 * (time.perf_counter() - t0))
            if not (torch.equal(b.label, want[0]) and torch.equal(b.hops, want[1])):
                raise SystemExit("basins_bench: the timed run differs (%s, %s)" % (cname, kind))
            # ---- the tiled form of the pass: as the first call only, and as every call
            tiled = {}
            for name, ncalls in (("first", 1), ("every", None)):
                b.run(check=1, sweeps=a.sweeps, tiled_calls=ncalls)
                if not (torch.equal(b.label, want[0]) and torch.equal(b.hops, want[1])):
                    raise SystemExit("basins_bench: the tiled form (%s call) differs (%s, %s)" % (name, cname, kind))
                calls, ms = b.passes, []
                for _ in range(a.reps):
                    b.begin()
                    blk = [[b._block(cur, 0, sw) for cur in (0, 1)] for sw in (1, a.sweeps)]

                    def go_tiled():
                        for n in range(calls):
                            eng.flow_basin_jump(blk[1 if ncalls is None or n < ncalls else 0][n & 1], stream=sh)
                    ms.append(timed(go_tiled))
                tiled[name] = dict(calls=calls, ms=med(ms))
            b.run()
            init_block, res_block = b._block(1 - b.cur, 0), b._block(b.cur, b.cap)

            def init():
                for n in range(10):
                    eng.flow_basin_init(init_block, stream=sh)              # writes the plane the result does not live in

            def resolve():
                for n in range(10):
                    eng.flow_basin_resolve(res_block, stream=sh)
            res_ms = med([timed(resolve) / 10 for _ in range(a.reps)])
            if not (torch.equal(b.label, want[0]) and torch.equal(b.hops, want[1])):
                raise SystemExit("basins_bench: resolve is not idempotent (%s, %s)" % (cname, kind))
            init_ms = med([timed(init) / 10 for _ in range(a.reps)])
            row = dict(case=cname, kind=kind, ni=ni, nj=nj, passes=passes, longest=longest, pass_ms=med(pass_ms) / passes, passes_ms=med(pass_ms),
                       init_ms=init_ms, resolve_ms=res_ms, run_ms=med(run_ms), up_passes=up_passes, acc_ms=acc_ms, up_s=up_s,
                       members=members, fill_calls=net.fill_calls if fill else 0, tiled=tiled, sweeps=a.sweeps)
            row["total_ms"] = row["init_ms"] + row["passes_ms"] + row["resolve_ms"]
            results.append(row)
            print(row, flush=True)

    text = render(results, torch.cuda.get_device_name(0), a.eps, a.reps)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(dict(device=torch.cuda.get_device_name(0), eps=a.eps, reps=a.reps, results=results), fh, indent=1)
    print("wrote", a.out)


def render(results, device, eps, reps):
    """The text of profiles/basins_bench.md from the results (also from a saved --json: --from-json re-renders without a GPU)."""
    o = ["# Basins by pointer doubling against the Jacobi traversal", "",
         "Written by `tools/basins_bench.py` (its docstring says what every column is) on %s, one device, fill eps = %g m, %d repetitions."
         % (device, eps, reps),
         "One gauge at the cell of the largest upstream count; at full size the cells labelled with it are as many as that count, no cell is "
         "unresolved, and passes = ceil(log2 max(longest path, 1)) + 1.  Device milliseconds span back-to-back launches, launch gaps included.", "",
         "| cells | network | longest path (hops) | passes | ms per pass | init ms | resolve ms | total device ms | run() wall ms | "
         "`upstream_cells`: passes x ms per pass = device ms | its wall s | total / upstream |",
         "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in results:
        up = r["up_passes"] * r["acc_ms"]
        o.append("| %s | %s | %d | %d | %.4f | %.4f | %.4f | %.3f | %.2f | %d x %.4f = %.2f | %.2f | %.4f |"
                 % (r["case"], r["kind"], r["longest"], r["passes"], r["pass_ms"], r["init_ms"], r["resolve_ms"], r["total_ms"], r["run_ms"],
                    r["up_passes"], r["acc_ms"], up, r["up_s"], r["total_ms"] / up))
    o += ["", "## The tiled form of the pass (in-tile pre-contraction)", "",
          "`sweeps` = %d in-tile iterations at most.  Device ms of the calls to the fixed point, the confirming one included; init and "
          "resolve are the same for every form." % results[0]["sweeps"], "",
          "| cells | network | pinned: passes, ms | tiled first call, then pinned: calls, ms | tiled every call: calls, ms |", "|---|---|---|---|---|"]
    for r in results:
        t = r["tiled"]
        o.append("| %s | %s | %d, %.3f | %d, %.3f | %d, %.3f |" % (r["case"], r["kind"], r["passes"], r["passes_ms"], t["first"]["calls"], t["first"]["ms"],
                                                             t["every"]["calls"], t["every"]["ms"]))
    sums = dict(pinned=sum(r["passes_ms"] for r in results), first=sum(r["tiled"]["first"]["ms"] for r in results),
                every=sum(r["tiled"]["every"]["ms"] for r in results))
    o += ["", "Summed over the four networks: pinned %.3f ms, tiled first call %.3f ms, tiled every call %.3f ms.  `noahmp_amd.routing.BASIN_SWEEPS` "
          "(the in-tile iterations of the first call `Basins.run` makes; 1 = every call is the pinned pass) follows the smallest sum: %s."
          % (sums["pinned"], sums["first"], sums["every"],
             dict(pinned="the pinned pass in every call (1)", first="the tiled form as the first call (%d)" % results[0]["sweeps"],
                  every="the tiled form in every call")[min(sums, key=sums.get)])]
    o += ["", "A pass moves 24 B per cell (the cell's 8-byte word, its pointer's, one store); the planes of the larger shape (57 MB each) sit in "
          "the 256 MB last-level cache between passes, so bytes per second from these figures are cache figures, not HBM figures.", "",
          ""]
    return "\n".join(o)


if __name__ == "__main__":
    main()
