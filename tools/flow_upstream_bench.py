"""What upstream sums by doubling cost on the device: noahmp_hip_flow_upstream_init and the passes of noahmp_hip_flow_upstream_pass to the
pass in which nobody pushes, and -- in the same run, on the same network -- FlowNetwork.upstream_cells (one Jacobi pass of
noahmp_hip_flow_accumulate per cell of the longest flow path), one pass of noahmp_hip_flow_basin_jump and a device-to-device copy of the
52 B per cell a pass moves.

    python tools/flow_upstream_bench.py [--reps 5] [--eps 1e-3] [--out profiles/flow_upstream_bench.md] [--json FILE]
    python tools/flow_upstream_bench.py --from-json profiles/flow_upstream_bench.json      re-renders the table from a saved run, without a GPU

Shapes: 4608 x 1536 (7 077 888 cells, the config-3 grid) and the 1152 x 768 tile of an 8-rank run (884 736 cells), 1 km spacing, the
synthetic terrain with about 2 km relief of tools/shadow_bench.py, filled (FlowNetwork.set_terrain(fill=eps)).  Weights: random uint32
below 2^20 (a quantised area).  Per shape:
  passes        passes Upstream.run made with the flag read after EVERY pass, the one that only folds included, and the longest flow
                path L in hops (Basins on the same network: hops.max());
  ms per pass   init outside the clock, then that many passes enqueued back to back between two device events, divided by their number
                (median of --reps): launch gaps included; and every pass on its own between events of its own (one repetition series,
                medians): the first pass is the one in which every cell with a downstream cell pushes;
  init          one launch, the mean of a window of 10, median of --reps;
  total         init + the passes between two device events; run() wall: Upstream.run() with its defaults (a batch of passes per host wait);
  upstream      passes FlowNetwork.upstream_cells made (flag read every 64) x the mean ms of one noahmp_hip_flow_accumulate pass in a window
                of 20, and the wall time of the call;
  basin_jump    one pinned pass of noahmp_hip_flow_basin_jump on the initial state of the same network, the mean of a window of 10;
  copy          a device-to-device copy of 26 B per cell (26 read, 26 written: the 52 B of a pass), the mean of a window of 10.
Before anything is timed, at full size: with unit weights the sums equal FlowNetwork.upstream_cells in every word, and
passes == bit_length(L) + 1; the timed weighted run gives the same words every repetition.  Nothing else is enforced.
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

PASS_BYTES = 52          # sum 8 + 8, pend_in 8 + 8, jump_old 4, the gather 4, the atomic 8, jump_new 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--eps", type=float, default=1e-3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flow_upstream_bench.md"))
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
    from noahmp_amd.routing import Basins, FlowNetwork, Upstream
    from noahmp_amd.tables import load_tables
    if not torch.cuda.is_available():
        raise SystemExit("flow_upstream_bench: no GPU -- nothing to measure")
    eng = Engine(load_tables("usgs")[0], device=0)
    stream = torch.cuda.Stream()
    sh = stream.cuda_stream
    med = statistics.median
    results = []

    def timed(fn, before=None):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            if before is not None:
                before()
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
        # ---- the figure to beat, and the check of the result
        t0 = time.perf_counter()
        acc = net.upstream_cells(max_pass=ncell)
        up_s = time.perf_counter() - t0
        up_passes = net.passes
        two = [torch.ones((nj, ni), dtype=torch.int32, device="cuda"), torch.ones((nj, ni), dtype=torch.int32, device="cuda")]
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")

        def accumulate():
            for n in range(20):
                eng.flow_accumulate(net.inmask, two[n & 1], two[1 - (n & 1)], flag, stream=sh)
        acc_ms = med([timed(accumulate) / 20 for _ in range(a.reps)])
        b = Basins(net)
        b.run(check=1, sweeps=1)
        longest = int(b.hops.max().item())
        u = Upstream(net)
        cells = u.cells(check=1)
        passes = u.passes
        if not torch.equal(cells, acc.to(torch.int64) & 0xFFFFFFFF):
            raise SystemExit("flow_upstream_bench: unit weights differ from upstream_cells (%s)" % cname)
        if passes != longest.bit_length() + 1:
            raise SystemExit("flow_upstream_bench: %d passes for a longest path of %d hops (%s)" % (passes, longest, cname))
        g = torch.Generator(device="cpu")
        g.manual_seed(ni)
        u.set_weight(torch.randint(0, 2 ** 20, (nj, ni), generator=g, dtype=torch.int32))
        want = u.run(check=1).clone()
        if u.passes != passes:
            raise SystemExit("flow_upstream_bench: the weighted run made %d passes, the unit run %d" % (u.passes, passes))
        # ---- timed
        u.begin()
        blocks = [u._block(cur, 0) for cur in (0, 1)]                       # made before the clock starts

        def init():
            eng.flow_upstream_init(blocks[0], stream=sh)

        def go():
            for n in range(passes):
                eng.flow_upstream_pass(blocks[n & 1], stream=sh)

        def both():
            init()
            go()
        passes_ms, total_ms, run_ms, each = [], [], [], []
        for _ in range(a.reps):
            passes_ms.append(timed(go, before=init))
            if not torch.equal(u.sum, want):
                raise SystemExit("flow_upstream_bench: a timed repetition differs (%s)" % cname)
            total_ms.append(timed(both))
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(passes + 1)]
            torch.cuda.synchronize()
            with torch.cuda.stream(stream):
                init()
                ev[0].record()
                for n in range(passes):
                    eng.flow_upstream_pass(blocks[n & 1], stream=sh)
                    ev[n + 1].record()
            ev[-1].synchronize()
            each.append([ev[n].elapsed_time(ev[n + 1]) for n in range(passes)])
            t0 = time.perf_counter()
            u.run()
            run_ms.append(1e3 * (time.perf_counter() - t0))
        init_ms = med([timed(lambda: [init() for _ in range(10)]) / 10 for _ in range(a.reps)])
        each_ms = [med([e[n] for e in each]) for n in range(passes)]
        # ---- next to it: one basin_jump pass, and a copy of the same bytes
        b.begin()
        jb = [b._block(cur, 0) for cur in (0, 1)]

        def jump():
            for n in range(10):
                eng.flow_basin_jump(jb[0], stream=sh)                       # state_old -> state_new of the initial state, every time
        jump_ms = med([timed(jump) / 10 for _ in range(a.reps)])
        half = PASS_BYTES // 2
        src = [torch.zeros(half * ncell, dtype=torch.uint8, device="cuda") for _ in range(2)]
        dst = [torch.empty(half * ncell, dtype=torch.uint8, device="cuda") for _ in range(2)]

        def copy():
            for n in range(10):
                dst[n & 1].copy_(src[n & 1])
        copy_ms = med([timed(copy) / 10 for _ in range(a.reps)])
        row = dict(case=cname, ni=ni, nj=nj, passes=passes, longest=longest, passes_ms=med(passes_ms), pass_ms=med(passes_ms) / passes,
                   each_ms=each_ms, init_ms=init_ms, total_ms=med(total_ms), run_ms=med(run_ms), up_passes=up_passes, acc_ms=acc_ms, up_s=up_s,
                   jump_ms=jump_ms, copy_ms=copy_ms, fill_calls=net.fill_calls)
        results.append(row)
        print(row, flush=True)
        del src, dst, two, u, b, net

    text = render(results, torch.cuda.get_device_name(0), a.eps, a.reps)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(dict(device=torch.cuda.get_device_name(0), eps=a.eps, reps=a.reps, results=results), fh, indent=1)
    print("wrote", a.out)


def render(results, device, eps, reps):
    """The text of profiles/flow_upstream_bench.md from the results (also from a saved --json: --from-json re-renders without a GPU)."""
    o = ["# Upstream sums by doubling against the Jacobi count", "",
         "Written by `tools/flow_upstream_bench.py` (its docstring says what every column is) on %s, one device, filled terrain (fill eps = %g m), "
         "random uint32 weights below 2^20, %d repetitions." % (device, eps, reps),
         "At full size, before the clock: with unit weights every word equals `FlowNetwork.upstream_cells`, passes = bit_length(longest path) + 1, "
         "and every timed repetition gives the same words.  Device milliseconds span back-to-back launches, launch gaps included.", "",
         "| cells | longest path (hops) | passes | ms per pass (mean) | init ms | total device ms (init + passes) | run() wall ms | "
         "`upstream_cells`: passes x ms per pass = device ms | its wall s | total / upstream |",
         "|---|---|---|---|---|---|---|---|---|---|"]
    for r in results:
        up = r["up_passes"] * r["acc_ms"]
        o.append("| %s | %d | %d | %.4f | %.4f | %.3f | %.2f | %d x %.4f = %.2f | %.2f | %.4f |"
                 % (r["case"], r["longest"], r["passes"], r["pass_ms"], r["init_ms"], r["total_ms"], r["run_ms"], r["up_passes"], r["acc_ms"], up,
                    r["up_s"], r["total_ms"] / up))
    o += ["", "## One pass next to its neighbours", "",
          "The first pass is the one in which every cell that has a downstream cell pushes (one 64-bit integer atomic per cell, to "
          "neighbouring cells); in the later passes fewer cells push, further away, and the cells where streams join take many adds.", "",
          "| cells | first pass ms | slowest pass: number, ms | last pass (folds only) ms | one `basin_jump` pass (24 B per cell) ms | "
          "device-to-device copy of %d B per cell ms | first pass / copy | first pass / basin_jump |" % PASS_BYTES, "|---|---|---|---|---|---|---|---|"]
    for r in results:
        e = r["each_ms"]
        worst = max(range(len(e)), key=lambda n: e[n])
        o.append("| %s | %.4f | %d, %.4f | %.4f | %.4f | %.4f | %.2f | %.2f |" % (r["case"], e[0], worst + 1, e[worst], e[-1], r["jump_ms"], r["copy_ms"],
                                                                                   e[0] / r["copy_ms"], e[0] / r["jump_ms"]))
    o += ["", "Every pass, ms (medians):", ""]
    for r in results:
        o.append("* %s: %s" % (r["case"], ", ".join("%.4f" % v for v in r["each_ms"])))
    o += ["", "The form that zeroes a plane and adds everything atomically (no deferred fold) was not built, so there is no second timing: the "
          "deferred fold is the only form.  *UNMEASURED:* a decomposed run over several processes with the real exchange.", "", ""]
    return "\n".join(o)


if __name__ == "__main__":
    main()
