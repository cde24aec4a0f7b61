"""What a step pays for its history: noahmp_hip_history_step against a device-to-device copy of the same traffic, in one run.

    python tools/history_bench.py [--reps 30] [--window-ms 8] [--out profiles/history_bench.md] [--json FILE] [--note FILE]

Shapes: the 4608 x 1536 block (config 3, 7.08 M columns) and the 1152 x 768 tile of an 8-rank run, all columns land.  Cases: 4, 16 and
32 two-dimensional entries (ops in turn SUM_DT, SUM, MIN, MAX, LAST) with the count plane, plus 256 probe points x 8 fields -- one
launch per call.  The kernel reads 8 B and writes 4 B per entry and column, and reads 8 B of class planes and reads + writes 8 B of
count per column: 12 B per entry-column + 24 B per column.  The comparator is ONE hipMemcpyAsync device-to-device whose bytes read plus
bytes written are the same (it copies half of them), on the same stream, ALTERNATING with the kernel repetition by repetition.

Timing: two device events around a window of back-to-back calls on one stream (the window is sized to --window-ms from a first
estimate, so that it does not measure the clock); every shape and case is warmed up first; --reps repetitions (at least 20); median,
minimum, maximum and the inter-quartile range are reported, in ms per call, with GB/s = bytes / median.  A process of its own: start
it under `timeout -k 10 ...`.  Before a case is timed, one call on fresh planes is compared bit for bit with the same float32 operations
done by torch at the full size (all entries, the count plane, the probe slot).  Without a GPU it fails (there is nothing to measure on a CPU).

The markdown it writes also takes notes (--note FILE: text appended as it is, e.g. bench.py's headline before and after the change).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_PINNED_MIN_XFER_SIZE", "1048576")

SHAPES = (("config 3 block", 4608, 1536, 3.25), ("8-rank tile", 1152, 768, 0.538))     # name, ni, nj, the step's ms (README)
ENTRY_COUNTS = (4, 16, 32)
OPS = ("sum_dt", "sum", "min", "max", "last")
NPOINT, NFIELD, NSLOT = 256, 8, 8
HIP_MEMCPY_D2D = 3


def kernel_bytes(ncol, nent):
    return ncol * (12 * nent + 24)


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "history_bench.md"))
    ap.add_argument("--json", default=None)
    ap.add_argument("--note", default=None)
    a = ap.parse_args()
    a.reps = max(a.reps, 20)
    import torch
    from noahmp_amd import abi
    from noahmp_amd.driver import Engine
    from noahmp_amd.tables import load_tables
    if not torch.cuda.is_available():
        raise SystemExit("history_bench: no GPU -- nothing to measure")
    eng = Engine(load_tables("usgs")[0], device=0)
    hip = _hip_runtime()
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    stream = torch.cuda.Stream()
    sh = stream.cuda_stream
    results = []
    with torch.cuda.stream(stream):
        for sname, ni, nj, step_ms in SHAPES:
            ncol = ni * nj
            xland = torch.ones((nj, ni), device="cuda")
            xice = torch.zeros((nj, ni), device="cuda")
            count = torch.zeros((nj, ni), dtype=torch.int32, device="cuda")
            nmax = max(ENTRY_COUNTS)
            src = [torch.rand((nj, ni), device="cuda") * 1e-4 for _ in range(nmax)]
            acc = [torch.zeros((nj, ni), device="cuda") for _ in range(nmax)]
            blk = abi.StepArgs()
            blk.ims = blk.its = blk.ids = blk.jms = blk.jts = blk.jds = 1
            blk.ime = blk.ite = blk.ide = ni
            blk.jme = blk.jte = blk.jde = nj
            blk.xland, blk.xice, blk.xice_thres = xland.data_ptr(), xice.data_ptr(), 0.5
            cols = torch.randint(0, ncol, (NPOINT,), dtype=torch.int32, device="cuda")
            ring = torch.zeros((NSLOT, NFIELD, NPOINT), device="cuda")
            probes = eng.history_probes(cols, src[:NFIELD], ring)
            half = kernel_bytes(ncol, nmax) // 2
            cp_src = torch.empty(half, dtype=torch.uint8, device="cuda").fill_(1)
            cp_dst = torch.empty(half, dtype=torch.uint8, device="cuda")
            stream.synchronize()
            for nent in ENTRY_COUNTS:
                ents = eng.history_entries([(src[f], acc[f], OPS[f % len(OPS)], 3600.0) for f in range(nent)])
                nbytes = kernel_bytes(ncol, nent)
                slot = [0]

                def kernel():
                    probes.slot = slot[0]
                    slot[0] += 1
                    eng.history_step(ents, blk, probes=probes, count=count, stream=sh)

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

                # faster and different is not faster: one call on fresh planes against the same float32 operations done by torch
                for t in acc[:nent]:
                    t.fill_(0.25)
                count.zero_()
                stream.synchronize()
                kernel()
                stream.synchronize()
                for f in range(nent):
                    x, a0, op = src[f], torch.full_like(src[f], 0.25), OPS[f % len(OPS)]
                    want = {"sum_dt": lambda: a0 + x * 3600.0, "sum": lambda: a0 + x, "min": lambda: torch.where(x < a0, x, a0),
                            "max": lambda: torch.where(x > a0, x, a0), "last": lambda: x}[op]()
                    if not torch.equal(acc[f].view(torch.int32), want.view(torch.int32)):
                        raise SystemExit("history_bench: entry %d (%s) of %d on %s differs from the torch restatement" % (f, op, nent, sname))
                if not bool((count == 1).all()) or not torch.equal(ring[(slot[0] - 1) % NSLOT], torch.stack([t.reshape(-1)[cols.long()] for t in src[:NFIELD]])):
                    raise SystemExit("history_bench: count plane or probe ring wrong on %s" % sname)
                for fn in (kernel, copy):                  # warm-up of this shape and case
                    window(fn, 5)
                calls = {fn: max(3, int(a.window_ms / max(window(fn, 5), 1e-3)) + 1) for fn in (kernel, copy)}
                ms = {kernel: [], copy: []}
                for rep in range(a.reps):                  # alternating, the order swapped every repetition
                    for fn in ((kernel, copy) if rep % 2 == 0 else (copy, kernel)):
                        ms[fn].append(window(fn, calls[fn]))
                k, c = _stats(ms[kernel]), _stats(ms[copy])
                results.append(dict(shape=sname, ni=ni, nj=nj, entries=nent, bytes=nbytes, kernel=k, copy=c,
                                    kernel_gbs=nbytes / k["median"] / 1e6, copy_gbs=nbytes / c["median"] / 1e6,
                                    ratio=c["median"] / k["median"], step_ms=step_ms, share=k["median"] / step_ms,
                                    calls_per_window=dict(kernel=calls[kernel], copy=calls[copy])))
                print(json.dumps(results[-1]), flush=True)
            del src, acc, cp_src, cp_dst
            torch.cuda.empty_cache()
    eng.stream_sync()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)
    lines = ["# Device-side history: what a step pays for it", "",
             "`tools/history_bench.py`: `noahmp_hip_history_step` (n two-dimensional entries + the count plane + %d probe points x %d fields, one"
             % (NPOINT, NFIELD),
             "launch) against one `hipMemcpyAsync` device-to-device with the same bytes read + written (12 B per entry-column + 24 B per column),",
             "alternating in one run on one MI355X.  Device events around windows of back-to-back calls (>= %g ms), %d repetitions after a warm-up"
             % (a.window_ms, a.reps),
             "of every case; ms per call: median (min .. max, inter-quartile range).  ratio = copy time / kernel time (1.0 = the rate of the",
             "in-run copy); share = kernel time / the step it follows (README: 3.25 ms config 3, 0.538 ms the 8-rank tile).", "",
             "| shape | entries | MB moved | kernel ms | kernel GB/s | copy ms | copy GB/s | ratio | share of the step |",
             "|---|---|---|---|---|---|---|---|---|"]
    for r in results:
        k, c = r["kernel"], r["copy"]
        lines.append("| %s %d x %d | %d | %.1f | %.4f (%.4f .. %.4f, %.4f) | %.0f | %.4f (%.4f .. %.4f, %.4f) | %.0f | %.2f | %.1f %% |" % (
            r["shape"], r["ni"], r["nj"], r["entries"], r["bytes"] / 1e6, k["median"], k["min"], k["max"], k["iqr"], r["kernel_gbs"],
            c["median"], c["min"], c["max"], c["iqr"], r["copy_gbs"], r["ratio"], 100.0 * r["share"]))
    lines.append("")
    low = min(results, key=lambda r: r["ratio"])
    lines.append("Lowest ratio: %.2f (%s, %d entries).  %s" % (
        low["ratio"], low["shape"], low["entries"],
        "Every case reaches at least 0.8 of the in-run copy's rate." if low["ratio"] >= 0.8 else
        "BELOW 0.8: look at the kernel with `rocprofv3 --kernel-trace --stats` in a run of its own and say here why."))
    lines.append("A ratio above 1 is no error: the copy writes half of its bytes, the kernel a third (8 B read per 4 B written), and a case whose")
    lines.append("planes fit the 256 MB Infinity Cache (the tile with 4 or 16 entries: 39 / 124 MB of planes) is served from it on both sides.")
    lines.append("")
    if a.note and os.path.exists(a.note):
        lines.append(open(a.note).read().rstrip())
        lines.append("")
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
