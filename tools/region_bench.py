"""What a step pays for its region series: noahmp_hip_region_step against a device-to-device copy of the same traffic, in one run.

    python tools/region_bench.py [--reps 30] [--window-ms 8] [--out profiles/region_bench.md] [--json FILE] [--note FILE] [--quick]

Shapes: the 4608 x 1536 block (config 3, 7.08 M columns) and the 1152 x 768 tile of an 8-rank run, all columns land, a weight plane.
Regions: 1 region; ~1 000 compact rectangular basins (a 32 x 32 grid of rectangles); ~100 000 small ones (squares of 8 x 8 resp. 3 x 3
cells).  Entries: n = 1, 4, 16 two-dimensional fields (ops in turn SUM, SUM, MIN, MAX).  Column order: tile order, and the order
noahmp_hip_sort_columns gives the key planes of a synthetic config-3 store (synth.config3's land-use, snow and temperature statistics:
CONUS vegetation mix, 2 % urban, 1 % glacier, 30 % snow-covered with 1-3 snow layers; keys = vegetation type, snow layers, 1 K bins of TSK
as Engine.sort_store asks for them), read through the members' positions.

Bytes of a call: per member 16 B (position, weight, XLAND, XICE) + 4 B per entry, plus 16 B per entry and chunk of 256 (the partial
written by level 1 and read by level 2).  The comparator is ONE hipMemcpyAsync
device-to-device whose bytes read plus bytes written are that figure (it copies half of it), on the same stream, ALTERNATING with the
kernel repetition by repetition.

Timing: two device events around a window of back-to-back calls on one stream (sized to --window-ms from a first estimate); every case
is warmed up first; --reps repetitions (at least 20); median, minimum, maximum and inter-quartile range in ms per call.  Before a case
is timed, one call into a fresh ring is compared value for value (float64 equal) with the numpy restatement of the contract at the full
size.  A process of its own: start it under `timeout -k 10 ...`.  Without a GPU it fails (there is nothing to measure on a CPU).
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
os.environ.setdefault("GPU_PINNED_MIN_XFER_SIZE", "1048576")

SHAPES = (("config 3 block", 4608, 1536, 3.25), ("8-rank tile", 1152, 768, 0.538))     # name, ni, nj, the step's ms (README)
ENTRY_COUNTS = (1, 4, 16)
OPS = ("sum", "sum", "min", "max")
HIP_MEMCPY_D2D = 3
HUGE = float(np.finfo(np.float32).max)
F, D = np.float32, np.float64


def call_bytes(nmember, nchunk1, nent):
    return nmember * (16 + 4 * nent) + 16 * nent * nchunk1


def region_maps(ni, nj):
    """(label, nregion, int32 map) of the three region sets."""
    j, i = np.meshgrid(np.arange(nj), np.arange(ni), indexing="ij")
    out = [("1 region", 1, np.zeros((nj, ni), np.int32))]
    out.append(("1 024 rectangular basins", 1024, ((j * 32 // nj) * 32 + i * 32 // ni).astype(np.int32)))
    b = max(1, int(round((ni * nj / 1e5) ** 0.5)))
    nbi, nbj = -(-ni // b), -(-nj // b)
    out.append(("%d squares of %d x %d cells" % (nbi * nbj, b, b), nbi * nbj, ((j // b) * nbi + i // b).astype(np.int32)))
    return out


def seg_tree(t, off, pad=0.0, comb=np.add):
    """S of the contract applied to every segment [off[r], off[r+1]) of t at once: chunks of 256, folded h = 128 .. 1, level by level."""
    nseg = off.size - 1
    while True:
        cnt = off[1:] - off[:-1]
        nch = (cnt + 255) // 256
        choff = np.concatenate([[0], np.cumsum(nch)])
        seg = np.repeat(np.arange(nseg), cnt)
        local = np.arange(t.size) - off[seg]
        m = np.full((int(choff[-1]), 256), pad, D)
        m[choff[seg] + local // 256, local % 256] = t
        h = 128
        while h:
            m = comb(m[:, :h], m[:, h:2 * h])
            h //= 2
        p = m[:, 0]
        if nch.max(initial=0) <= 1:
            res = np.full(nseg, pad, D)
            res[nch == 1] = p
            return res
        t, off = p, choff


def reference(region, nregion, weight, fields):
    """[len(fields)][nregion] float64 of the contract (every cell takes part)."""
    reg = region.ravel()
    order = np.argsort(reg, kind="stable")
    off = np.searchsorted(reg[order], np.arange(nregion + 1))
    w = weight.ravel()[order].astype(D)
    out = []
    for x, op in fields:
        xs = x.ravel()[order]
        if op == "sum":
            out.append(seg_tree(w * xs.astype(D), off))
        elif op == "min":
            out.append(seg_tree(np.where(xs < HUGE, xs, HUGE).astype(D), off, HUGE, np.minimum))
        else:
            out.append(seg_tree(np.where(xs > -HUGE, xs, -HUGE).astype(D), off, -HUGE, np.maximum))
    return np.stack(out)


def config3_keys(ni, nj, seed=3):
    """The planes the column sort reads, with synth.config3's statistics (the full store is not needed for the order)."""
    from noahmp_amd.synth import CONUS_VEG
    from noahmp_amd.state import ModelConfig
    cfg = ModelConfig()
    r = np.random.default_rng(seed)
    shp = (nj, ni)
    veg = CONUS_VEG[r.integers(0, len(CONUS_VEG), size=shp)].astype(np.int32)
    u = r.random(size=shp)
    veg[u < 0.02] = cfg.isurban
    gl = (u >= 0.02) & (u < 0.03)
    veg[gl] = cfg.isice
    tair = np.clip(r.normal(272.0, 8.0, size=shp), 245.0, 300.0).astype(F)
    has_snow = (r.random(size=shp) < 0.30) | gl
    tsk = np.where(has_snow, np.minimum(tair, F(272.0)), np.maximum(tair, F(274.5))).astype(F)
    snowh = np.where(has_snow, r.uniform(5.0, 300.0, size=shp) / r.uniform(100.0, 350.0, size=shp), 0.0)
    isnow = np.where(snowh < 0.025, 0, np.where(snowh <= 0.05, -1, np.where(snowh <= 0.20, -2, -3))).astype(np.int32)     # drv:1175-1216
    return veg, isnow, tsk, cfg


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "region_bench.md"))
    ap.add_argument("--json", default=None)
    ap.add_argument("--note", default=None)
    ap.add_argument("--quick", action="store_true", help="the 8-rank tile only (a rehearsal of the tool)")
    a = ap.parse_args()
    a.reps = max(a.reps, 20)
    import torch
    from noahmp_amd import abi
    from noahmp_amd.driver import Engine
    from noahmp_amd.tables import load_tables
    if not torch.cuda.is_available():
        raise SystemExit("region_bench: no GPU -- nothing to measure")
    eng = Engine(load_tables("usgs")[0], device=0)
    lib = eng.lib
    hip = _hip_runtime()
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    stream = torch.cuda.Stream()
    sh = stream.cuda_stream
    results = []
    nmax = max(ENTRY_COUNTS)
    with torch.cuda.stream(stream):
        for sname, ni, nj, step_ms in (SHAPES[1:] if a.quick else SHAPES):
            ncol = ni * nj
            r = np.random.default_rng(ni)
            fields_h = [(r.standard_normal(ncol) * 10.0 ** r.uniform(-3, 4, ncol)).astype(F).reshape(nj, ni) for _ in range(nmax)]
            weight_h = r.uniform(0.5, 2.0, ncol).astype(F).reshape(nj, ni)
            ops = [OPS[f % len(OPS)] for f in range(nmax)]
            # the sorted order of a synthetic config-3 store
            veg, isnow, tsk, cfg = config3_keys(ni, nj)
            xland = torch.ones((nj, ni), device="cuda")
            xice = torch.zeros((nj, ni), device="cuda")
            keys = abi.StepArgs()
            keys.ims = keys.its = keys.ids = keys.jms = keys.jts = keys.jds = 1
            keys.ime = keys.ite = keys.ide = ni
            keys.jme = keys.jte = keys.jde = nj
            kp = [torch.from_numpy(x).cuda() for x in (veg, isnow, tsk)]
            keys.xland, keys.xice, keys.xice_thres, keys.isice = xland.data_ptr(), xice.data_ptr(), 0.5, cfg.isice
            keys.ivgtyp, keys.isnowxy, keys.tsk = kp[0].data_ptr(), kp[1].data_ptr(), kp[2].data_ptr()
            perm = torch.empty(ncol, dtype=torch.int32, device="cuda")
            stream.synchronize()
            rc = lib.noahmp_hip_sort_columns(C.byref(keys), abi.SORT_VEG | abi.SORT_SNOW, 1000, perm.data_ptr(), None, None, sh)
            if rc:
                raise SystemExit("noahmp_hip_sort_columns: rc=%d %s" % (rc, lib.noahmp_hip_last_error().decode()))
            stream.synchronize()
            inv = torch.empty_like(perm)
            inv[perm.long()] = torch.arange(ncol, dtype=torch.int32, device="cuda")
            weight = torch.from_numpy(weight_h).cuda()
            tile_planes = [torch.from_numpy(x).cuda() for x in fields_h]
            sorted_planes = [t.reshape(-1)[perm.long()].reshape(nj, ni).contiguous() for t in tile_planes]
            blk = abi.StepArgs()
            blk.ims = blk.its = blk.ids = blk.jms = blk.jts = blk.jds = 1
            blk.ime = blk.ite = blk.ide = ni
            blk.jme = blk.jte = blk.jde = nj
            blk.xland, blk.xice, blk.xice_thres = xland.data_ptr(), xice.data_ptr(), 0.5       # all land: the same planes in every order
            stream.synchronize()
            for rname, nregion, reg_h in region_maps(ni, nj):
                want = reference(reg_h, nregion, weight_h, list(zip(fields_h, ops)))
                reg = torch.from_numpy(reg_h).cuda()
                stream.synchronize()
                series = torch.zeros((2, nmax, nregion), dtype=torch.float64, device="cuda")
                for order, route in (("tile order", 0), ("sorted", 1)):
                    rp = eng.region_plan(reg, nregion, weight, None if route == 0 else inv, stream=sh)
                    planes = tile_planes if route == 0 else sorted_planes
                    for nent in ENTRY_COUNTS:
                        ents = eng.region_entries([(planes[f], ops[f], None) for f in range(nent)])
                        nbytes = eng.region_scratch_bytes(rp, nent)
                        scratch = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device="cuda")
                        hdr = rp.plan[:16].cpu().numpy()
                        nmember, nchunk1 = int(hdr[4]), int(hdr[5])
                        moved = call_bytes(nmember, nchunk1, nent)
                        cp_src = torch.empty(moved // 2, dtype=torch.uint8, device="cuda").fill_(1)
                        cp_dst = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
                        slot = [0]
                        stream.synchronize()

                        def kernel():
                            rc = lib.noahmp_hip_region_step(rp.plan.data_ptr(), nent, ents, C.byref(blk), series.data_ptr(), 2, slot[0], None,
                                                            scratch.data_ptr(), sh)
                            slot[0] += 1
                            if rc:
                                raise RuntimeError("noahmp_hip_region_step: %d %s" % (rc, lib.noahmp_hip_last_error().decode()))

                        def copy():
                            rc = hip.hipMemcpyAsync(cp_dst.data_ptr(), cp_src.data_ptr(), moved // 2, HIP_MEMCPY_D2D, sh)
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

                        # faster and different is not faster: one call into a fresh ring against the restatement, at the full size
                        series.fill_(-7.0)
                        stream.synchronize()
                        kernel()
                        stream.synchronize()
                        at = ((slot[0] - 1) % 2) * nent * nregion               # the ring of this call is [2][nent][nregion]
                        got = series.reshape(-1)[at: at + nent * nregion].cpu().numpy().reshape(nent, nregion)
                        if not np.array_equal(got, want[:nent]):
                            bad = np.argwhere(got != want[:nent])[0]
                            raise SystemExit("region_bench: %s, %s, %s, n = %d: entry %d region %d is %r, the restatement gives %r"
                                             % (sname, rname, order, nent, bad[0], bad[1], got[tuple(bad)], want[tuple(bad)]))
                        for fn in (kernel, copy):
                            window(fn, 5)
                        calls = {fn: max(3, int(a.window_ms / max(window(fn, 5), 1e-3)) + 1) for fn in (kernel, copy)}
                        ms = {kernel: [], copy: []}
                        for rep in range(a.reps):          # alternating, the order swapped every repetition
                            for fn in ((kernel, copy) if rep % 2 == 0 else (copy, kernel)):
                                ms[fn].append(window(fn, calls[fn]))
                        k, c = _stats(ms[kernel]), _stats(ms[copy])
                        results.append(dict(shape=sname, ni=ni, nj=nj, regions=rname, nregion=nregion, order=order, route=route, entries=nent,
                                            bytes=moved, members=nmember, chunks=nchunk1, kernel=k, copy=c,
                                            kernel_gbs=moved / k["median"] / 1e6, copy_gbs=moved / c["median"] / 1e6,
                                            ratio=c["median"] / k["median"], step_ms=step_ms, share=k["median"] / step_ms,
                                            calls_per_window=dict(kernel=calls[kernel], copy=calls[copy])))
                        print(json.dumps(results[-1]), flush=True)
                        del scratch, cp_src, cp_dst
                del rp, series, reg
                torch.cuda.empty_cache()
            del tile_planes, sorted_planes
            torch.cuda.empty_cache()
    eng.stream_sync()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)
    lines = ["# Region series: what a step pays for them", "",
             "`tools/region_bench.py`: `noahmp_hip_region_step` (n two-dimensional entries, ops in turn SUM, SUM, MIN, MAX, a weight plane, all",
             "columns land; two or three launches) against one `hipMemcpyAsync` device-to-device with the same bytes read + written (per member",
             "16 B + 4 B per entry, plus 16 B per entry and chunk of 256), alternating in one run on one MI355X.  Device events around windows of",
             "back-to-back calls (>= %g ms), %d repetitions after a warm-up of every case; every case was first compared value for value with"
             % (a.window_ms, a.reps),
             "the numpy restatement of the contract at the full size.  ms per call: median (min .. max, inter-quartile range).  ratio = copy time /",
             "kernel time; share = kernel time / the step it follows (README: 3.25 ms config 3, 0.538 ms the 8-rank tile).  Sorted = the order",
             "`noahmp_hip_sort_columns` gives the key planes of a synthetic config-3 store; every sample is read through the member's position.", "",
             "| shape | regions | column order | n | MB | kernel ms | GB/s | copy ms | copy GB/s | ratio | share of the step |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in results:
        k, c = r["kernel"], r["copy"]
        lines.append("| %s %d x %d | %s | %s | %d | %.1f | %.4f (%.4f .. %.4f, %.4f) | %.0f | %.4f (%.4f .. %.4f, %.4f) | %.0f | %.2f | %.1f %% |" % (
            r["shape"], r["ni"], r["nj"], r["regions"], r["order"], r["entries"], r["bytes"] / 1e6, k["median"], k["min"], k["max"], k["iqr"],
            r["kernel_gbs"], c["median"], c["min"], c["max"], c["iqr"], r["copy_gbs"], r["ratio"], 100.0 * r["share"]))
    lines.append("")
    if a.note and os.path.exists(a.note):
        lines.append(open(a.note).read().rstrip())
        lines.append("")
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
