"""Cost of one ring exchange through the C-ABI (noahmp_hip_exchange_halo) on device planes: socket transport (tcp) against HIP-IPC
transport (ipc), W ranks on ONE GPU.

    python tools/halo_bench.py [--world 8] [--tile 1152 768] [--calls 200] [--warmup 20] [--rounds 3] [--planes 1 3] [--out FILE.json]

Geometry: tiles of the config-4 grid on 8 ranks (1152 x 768) on the world's rank grid (mpp_land_get_nprocsxy): at W = 8 the global grid
is the config-4 grid itself (4 x 2 tiles, 4608 x 1536), at W = 9 3 x 3 tiles, at W = 2 2 x 1.  Per round the two transports run one
after the other, their order alternating between rounds; each run of a transport is its own halo_init / finalize with `warmup` untimed calls per plane count first.  Per call: host wall time
from the call to the end of a synchronise of the stream, and the span of two device events around the call on that stream.
Reported per transport and plane count: the median over all calls of all ranks, p10 / p90, the share of calls above 1 ms and the
spread of the per-round medians.  Ranks share one GPU here, so this is the same-device path only (no xGMI), and every rank's kernels
compete with the others' for the GPU's hardware queues."""
import argparse
import json
import os
import socket
import sys
import time
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_PINNED_MIN_XFER_SIZE", "1048576")

IDX8 = ("ims", "ime", "jms", "jme", "its", "ite", "jts", "jte")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, ports, a, q):
    try:
        import ctypes as C
        import torch
        from noahmp_amd import abi
        from noahmp_amd.partition import nprocs_xy, tile_geometry
        os.environ.update(NMP_HALO_TIMEOUT_S="60", NMP_HALO_IO_TIMEOUT_S="120")
        lib = abi.load_library()
        if lib.noahmp_hip_set_device(0):
            raise RuntimeError(lib.noahmp_hip_last_error().decode())
        torch.cuda.set_device(0)
        stream = torch.cuda.Stream()
        npx, npy = nprocs_xy(world)
        geo = tile_geometry(npx * a.tile[0], npy * a.tile[1], world, rank, halo=1)
        shape = (geo["jme"] - geo["jms"] + 1, geo["ime"] - geo["ims"] + 1)
        planes = [torch.rand(shape, device="cuda") for _ in range(max(a.planes))]
        idx = (C.c_int32 * 8)(*[geo[k] for k in IDX8])
        torch.cuda.synchronize()
        out = []                                       # (round, transport, n, host_us, device_us)
        k = 0
        for rnd in range(a.rounds):
            order = ("tcp", "ipc") if rnd % 2 == 0 else ("ipc", "tcp")
            for name in order:
                rc = lib.noahmp_hip_halo_init(rank, world, b"127.0.0.1", ports[k], abi.HALO_IPC if name == "ipc" else abi.HALO_TCP)
                k += 1
                if rc:
                    raise RuntimeError("%s init: %s" % (name, lib.noahmp_hip_last_error().decode()))
                for n in a.planes:
                    ptrs = (C.c_void_p * n)(*[p.data_ptr() for p in planes[:n]])
                    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.calls)]
                    host = []
                    for i in range(a.warmup + a.calls):
                        timed = i >= a.warmup
                        if timed:
                            ev[i - a.warmup][0].record(stream)
                        t0 = time.perf_counter()
                        rc = lib.noahmp_hip_exchange_halo(n, ptrs, idx, abi.MEM_DEVICE, stream.cuda_stream)
                        if rc:
                            raise RuntimeError("%s exchange: %s" % (name, lib.noahmp_hip_last_error().decode()))
                        if timed:
                            ev[i - a.warmup][1].record(stream)
                        stream.synchronize()
                        if timed:
                            host.append((time.perf_counter() - t0) * 1e6)
                    for (e0, e1), h in zip(ev, host):
                        out.append((rnd, name, n, h, e0.elapsed_time(e1) * 1e3))
                if lib.noahmp_hip_halo_finalize():
                    raise RuntimeError("finalize: " + lib.noahmp_hip_last_error().decode())
        q.put((rank, out))
    except Exception:                                                # noqa: BLE001
        q.put((rank, traceback.format_exc()))


def _pct(v, p):
    v = sorted(v)
    return v[min(len(v) - 1, int(p / 100.0 * len(v)))]


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--world", type=int, default=8)
    ap.add_argument("--tile", type=int, nargs=2, default=[1152, 768], metavar=("NX", "NY"))
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--planes", type=int, nargs="+", default=[1, 3])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch.multiprocessing as mp
    from noahmp_amd.partition import partition, nprocs_xy
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ports = [_free_port() for _ in range(2 * a.rounds)]
    procs = [ctx.Process(target=_worker, args=(r, a.world, ports, a, q)) for r in range(a.world)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=1800) for _ in range(a.world))
    for p in procs:
        p.join(60)
    bad = {r: v for r, v in res.items() if not isinstance(v, list)}
    if bad:
        for r, v in sorted(bad.items()):
            print("rank %d:\n%s" % (r, v), file=sys.stderr)
        sys.exit(1)
    rows = [x for v in res.values() for x in v]
    npx, npy = nprocs_xy(a.world)
    t = partition(npx * a.tile[0], npy * a.tile[1], a.world)[0]
    summary = {"world": a.world, "rank_grid": [npx, npy], "tile": [t["nx"], t["ny"]], "calls": a.calls, "warmup": a.warmup,
               "rounds": a.rounds, "results": []}
    print("W=%d, rank grid %d x %d, tile %d x %d, %d timed calls x %d rounds per rank (+%d warm-up)"
          % (a.world, npx, npy, t["nx"], t["ny"], a.calls, a.rounds, a.warmup))
    print("| transport | planes | host median us | host p10 / p90 | device span median us | device p10 / p90 | calls > 1 ms | per-round host medians |")
    print("|---|---|---|---|---|---|---|---|")
    for n in a.planes:
        for name in ("tcp", "ipc"):
            sel = [x for x in rows if x[1] == name and x[2] == n]
            h, d = [x[3] for x in sel], [x[4] for x in sel]
            per_round = [_pct([x[3] for x in sel if x[0] == r], 50) for r in range(a.rounds)]
            rec = {"transport": name, "planes": n, "host_us_median": _pct(h, 50), "host_us_p10": _pct(h, 10), "host_us_p90": _pct(h, 90),
                   "device_us_median": _pct(d, 50), "device_us_p10": _pct(d, 10), "device_us_p90": _pct(d, 90),
                   "share_above_1ms": sum(x > 1000.0 for x in h) / len(h), "host_us_round_medians": per_round, "samples": len(sel)}
            summary["results"].append(rec)
            print("| %s | %d | %.1f | %.1f / %.1f | %.1f | %.1f / %.1f | %.0f %% | %s |"
                  % (name, n, rec["host_us_median"], rec["host_us_p10"], rec["host_us_p90"], rec["device_us_median"], rec["device_us_p10"],
                     rec["device_us_p90"], 100.0 * rec["share_above_1ms"], " ".join("%.1f" % x for x in per_round)))
    print(json.dumps(summary))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(summary, f, indent=1)


if __name__ == "__main__":
    main()
