"""What conditioning a raw DEM on the device costs: noahmp_hip_flow_fill to its fixed point in the pinned form (sweeps = 1) and in the
tiled LDS form at several `sweeps`, and -- in the same run -- a device-to-device copy of the call's bytes as the yardstick.

    python tools/flow_fill_bench.py [--reps 5] [--sweeps 4,16,64,256] [--eps 1e-3] [--out profiles/flow_fill_bench.md] [--json FILE]
    python tools/flow_fill_bench.py --from-json profiles/flow_fill_bench.json        re-renders the table from a saved run, without a GPU

Shapes: 4608 x 1536 (7 077 888 cells, the config-3 grid) and the 1152 x 768 tile of an 8-rank run (884 736 cells), 1 km spacing, the
synthetic terrain with about 2 km relief of tools/shadow_bench.py, every window edge an outlet side.
Per shape and setting:
  calls        calls of noahmp_hip_flow_fill to the fixed point, the confirming one included, counted with the flag read after EVERY call;
  device ms    that many calls enqueued back to back between two device events (median of --reps, minimum and maximum); the span
               includes the gaps between the launches of hundreds of short kernels, not only their run time;
  ms per call  device ms / calls: the MEAN over the run -- a tiled call sweeps long at first and only copies at the end;
  run() ms     wall time of DepressionFill.run(sweeps=...) with its default flag read every 8 calls (median of --reps);
  idle call    one call at the fixed point (it changes nothing), median of a window of 20;
  copy         a device-to-device copy of the 13 B per cell a call must move at least (height 4, fixed 1, w_old 4, w_new 4): 6.5 read and
               6.5 written, a window of 20.
Before anything is timed every tiled result is compared with the sweeps = 1 result in EVERY WORD at full size, and noahmp_hip_flow_terrain
on the result must leave a cell without a direction only where fixed == 1.  Then: the share of cells raised, the largest raise, and the
passes FlowNetwork.upstream_cells needs on the filled network (read every 64).  Nothing is enforced beyond those two checks.
A process of its own: start it under `timeout -k 10 ...`.  Without a GPU it fails (there is nothing to measure on a CPU).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_PINNED_MIN_XFER_SIZE", "1048576")

from tools.shadow_bench import terrain, DX  # noqa: E402

BYTES = 13


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sweeps", default="4,16,64,256")
    ap.add_argument("--eps", type=float, default=1e-3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flow_fill_bench.md"))
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
    from noahmp_amd.routing import DepressionFill, FlowNetwork
    from noahmp_amd.tables import load_tables
    if not torch.cuda.is_available():
        raise SystemExit("flow_fill_bench: no GPU -- nothing to measure")
    eng = Engine(load_tables("usgs")[0], device=0)
    settings = [1] + [int(s) for s in a.sweeps.split(",")]
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
        f = DepressionFill(eng)
        rows, want = [], None
        for sweeps in settings:
            # ---- the result and the exact call count first
            f.begin(zd, a.eps)
            f.run(check=1, sweeps=sweeps)
            calls = f.calls
            got = f.surface.clone()
            if want is None:
                want = got
                fixed = f.fixed.clone()
                d = torch.empty((nj, ni), dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                eng.flow_terrain(eng.flow_terrain_block(want, d, DX, DX))
                eng.stream_sync()
                stuck = int(((d == 0) & (fixed != 1)).sum().item())
                if stuck:
                    raise SystemExit("flow_fill_bench: %d cells of %s have no direction and are no outlets" % (stuck, cname))
            elif not torch.equal(got.view(torch.int32), want.view(torch.int32)):
                raise SystemExit("flow_fill_bench: sweeps = %d differs from sweeps = 1 on %s" % (sweeps, cname))
            # ---- timed
            dev_ms, run_ms = [], []
            for _ in range(a.reps):
                f.begin(zd, a.eps)
                for cur in (0, 1):
                    f._block(cur, 0, sweeps)                             # the two argument blocks are made before the clock starts

                def go():
                    for n in range(calls):
                        eng.flow_fill(f._block(f.cur, 0, sweeps), stream=sh)
                        f.cur = 1 - f.cur
                dev_ms.append(timed(go))
                f.begin(zd, a.eps)
                t0 = time.perf_counter()
                f.run(sweeps=sweeps)
                run_ms.append(1e3 * (time.perf_counter() - t0))
            if not torch.equal(f.surface.view(torch.int32), want.view(torch.int32)):
                raise SystemExit("flow_fill_bench: the timed run of sweeps = %d differs on %s" % (sweeps, cname))

            def idle():
                for n in range(20):
                    eng.flow_fill(f._block(f.cur, 0, sweeps), stream=sh)
                    f.cur = 1 - f.cur
            idle_ms = med([timed(idle) / 20 for _ in range(a.reps)])
            rows.append(dict(sweeps=sweeps, calls=calls, dev_ms=med(dev_ms), dev_min=min(dev_ms), dev_max=max(dev_ms), run_ms=med(run_ms),
                             run_calls=f.calls, idle_ms=idle_ms))
            print(cname, rows[-1], flush=True)
        src = torch.empty(int(6.5 * ncell), dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)

        def copy():
            for n in range(20):
                dst.copy_(src)
        copy_ms = med([timed(copy) / 20 for _ in range(max(a.reps, 5))])
        raised = float((want > zd).float().mean().item())
        largest = float(torch.where(torch.isfinite(want), want - zd, torch.zeros_like(zd)).max().item())
        net = FlowNetwork(eng, ni, nj)
        net.set_directions(d, dx=DX, dy=DX)
        t0 = time.perf_counter()
        acc = net.upstream_cells(max_pass=ncell)
        up_s = time.perf_counter() - t0
        largest_up = int(acc.max().item())                                 # below 2^31: the words are read as int32
        results.append(dict(case=cname, ni=ni, nj=nj, rows=rows, copy_ms=copy_ms, raised=raised, largest=largest, free=f.free_cells,
                            upstream_passes=net.passes, upstream_s=up_s, largest_upstream=largest_up))
        print(cname, {k: v for k, v in results[-1].items() if k != "rows"}, flush=True)

    text = render(results, torch.cuda.get_device_name(0), a.eps, a.reps)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(dict(device=torch.cuda.get_device_name(0), eps=a.eps, reps=a.reps, results=results), fh, indent=1)
    print("wrote", a.out)


def render(results, device, eps, reps):
    """The text of profiles/flow_fill_bench.md from the results (also from a saved --json: --from-json re-renders without a GPU)."""
    best = {r["case"]: min(r["rows"], key=lambda x: x["dev_ms"])["sweeps"] for r in results}
    o = ["# noahmp_hip_flow_fill to the fixed point: pinned form against the tiled LDS kernel", "",
         "Written by `tools/flow_fill_bench.py` (its docstring says what every column is) on %s, one device, eps = %g m, %d repetitions."
         % (device, eps, reps),
         "Every tiled result equals the sweeps = 1 result in every word at full size; `noahmp_hip_flow_terrain` on it leaves a cell without "
         "a direction only where fixed == 1.  The device milliseconds span back-to-back launches, launch gaps included.", ""]
    for r in results:
        o += ["## %s" % r["case"], "",
              "| sweeps | calls | device ms to the fixed point (min .. max) | mean ms per call | run() wall ms (calls made) | idle call ms | idle call / copy |",
              "|---|---|---|---|---|---|---|"]
        for x in r["rows"]:
            o.append("| %d%s | %d | %.2f (%.2f .. %.2f) | %.4f | %.2f (%d) | %.4f | %.2f |"
                     % (x["sweeps"], " (pinned)" if x["sweeps"] == 1 else "", x["calls"], x["dev_ms"], x["dev_min"], x["dev_max"],
                        x["dev_ms"] / x["calls"], x["run_ms"], x["run_calls"], x["idle_ms"], x["idle_ms"] / r["copy_ms"]))
        o += ["", "Device-to-device copy of %d B per cell (6.5 read, 6.5 written): %.4f ms = %.0f GB/s." %
              (BYTES, r["copy_ms"], BYTES * r["ni"] * r["nj"] / r["copy_ms"] / 1e6),
              "Free cells %d; cells raised %.2f %%; largest raise %.3f m.  `FlowNetwork.upstream_cells` on the filled network: %d passes "
              "(flag read every 64) in %.2f s%s." % (r["free"], 100.0 * r["raised"], r["largest"], r["upstream_passes"], r["upstream_s"],
                                                    "; largest upstream count %d" % r["largest_upstream"] if r["largest_upstream"] >= 0 else ""),
              "Smallest device time to the fixed point: sweeps = %d." % best[r["case"]], ""]
    sums = {}
    for r in results:
        for x in r["rows"]:
            sums[x["sweeps"]] = sums.get(x["sweeps"], 0.0) + x["dev_ms"]
    choice = min(sums, key=sums.get)
    o += ["## The default", "",
          "Device ms to the fixed point summed over the shapes: " + ", ".join("sweeps = %d: %.2f" % (k, v) for k, v in sums.items()) + ".",
          "`noahmp_amd.routing.FILL_SWEEPS` is the setting with the smallest time at every shape where one exists, otherwise the one with the "
          "smallest sum: here sweeps = %d%s." % (choice, "" if len(set(best.values())) > 1 else " (the fastest at every shape)"),
          "", "The copy moves one source of 6.5 B per cell twenty times in a row and the idle calls cycle through two planes: at these sizes both "
          "sit in the 256 MB last-level cache, so their bytes per second are cache figures, not HBM figures.", ""]
    return "\n".join(o)



if __name__ == "__main__":
    main()
