"""The C-ABI ring exchange with its HIP-IPC transport (NOAHMP_HALO_IPC, noahmp_halo.hip): every rank exports one device buffer, the
neighbours read their messages from it with one pull kernel per call, the sockets carry small control tokens only.

All ranks of a test share GPU 0 (same-device IPC: what a one-GPU box can run of the multi-GPU path).  Workers are spawned; the parent
never opens the GPU, its references come from numpy or the oracle (PortLib)."""
import os
import re
import socket
import time
import traceback

import numpy as np
import pytest
import torch.multiprocessing as mp

from noahmp_amd import abi, synth
from noahmp_amd.abi import FIELD_INFO
from noahmp_amd.partition import nprocs_xy, tile_geometry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDX8 = ("ims", "ime", "jms", "jme", "its", "ite", "jts", "jte")
CFG4 = (4608, 1536)                      # the config-4 grid: 4 x 2 tiles of 1152 x 768 on 8 ranks, 3 x 3 on 9
# (geometry, planes) per call: the 3 x 3-cells-per-rank probe grid first, then the config-4 grid (buffer growth, multi-block pulls);
# seven calls, so both halves of the exported buffer are reused three times
CALLS = [("probe", 1), ("probe", 3), ("cfg4", 3), ("cfg4", 64), ("cfg4", 1), ("cfg4", 3), ("probe", 1)]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _grid(kind, world):
    npx, npy = nprocs_xy(world)
    return (3 * npx, 3 * npy) if kind == "probe" else CFG4


def _ring_mask(geo):
    ring = np.ones((geo["jme"] - geo["jms"] + 1, geo["ime"] - geo["ims"] + 1), dtype=bool)
    ring[geo["jts"] - geo["jms"]:geo["jte"] - geo["jms"] + 1, geo["its"] - geo["ims"]:geo["ite"] - geo["ims"] + 1] = False
    return ring


def _planes(geo, gx, call, n, dev):
    """n planes of the memory block whose values name their global cell, different in every call: planes p % 3 == 1 are int32,
    the others float32 (exact: cell ids < 2**24, power-of-two scales)."""
    import torch
    jj = torch.arange(geo["jms"] - 1, geo["jme"], device=dev, dtype=torch.int64)[:, None]
    ii = torch.arange(geo["ims"] - 1, geo["ime"], device=dev, dtype=torch.int64)[None, :]
    cid = jj * gx + ii
    out = []
    for p in range(n):
        if p % 3 == 1:
            h = (cid * 2654435761 + (p + 1) * 40503 + call * 1000003) % (1 << 32)
            out.append(torch.where(h >= (1 << 31), h - (1 << 32), h).to(torch.int32))
        else:
            out.append((cid + 1).to(torch.float32) * ((-1.0) ** (call + p)) * 2.0 ** -((call + p) % 4))
    return out


def _poison(planes, ring_t):
    import torch
    for p in planes:
        p[ring_t] = torch.tensor(-7 if p.dtype == torch.int32 else float("nan"), dtype=p.dtype, device=p.device)


def _digest(planes):
    """A position-weighted sum of the planes' bits (on the device): equal planes give equal digests."""
    import torch
    d = 0
    for p in planes:
        b = p.view(torch.int32).to(torch.int64).flatten()
        w = torch.arange(b.numel(), device=b.device, dtype=torch.int64) % 1009 + 1
        d = (d * 31 + int((b * w).sum().item())) % (1 << 61)
    return d


def _exchange(lib, planes, geo, stream):
    import ctypes as C
    ptrs = (C.c_void_p * len(planes))(*[p.data_ptr() for p in planes])
    idx = (C.c_int32 * 8)(*[geo[k] for k in IDX8])
    return lib.noahmp_hip_exchange_halo(len(planes), ptrs, idx, abi.MEM_DEVICE, stream.cuda_stream)


def _run_calls(lib, rank, world, stream, calls):
    """The calls on device planes; per call: rc, planes equal to the global field bit for bit (ring = neighbours' tile cells,
    interior untouched), digest."""
    import torch
    dev = torch.device("cuda", 0)
    out = []
    for c, (kind, n) in enumerate(calls):
        gx, gy = _grid(kind, world)
        geo = tile_geometry(gx, gy, world, rank, halo=1)
        want = _planes(geo, gx, c, n, dev)
        got = [w.clone() for w in want]
        _poison(got, torch.from_numpy(_ring_mask(geo)).to(dev))
        torch.cuda.synchronize()
        rc = _exchange(lib, got, geo, stream)
        msg = lib.noahmp_hip_last_error().decode() if rc else ""
        stream.synchronize()
        ok = rc == 0 and all(torch.equal(g.view(torch.int32), w.view(torch.int32)) for g, w in zip(got, want))
        out.append((rc, msg, ok, _digest(got)))
        if rc:
            break
    return out


def _gpu_env():
    os.environ.update(NMP_HALO_TIMEOUT_S="60", NMP_HALO_IO_TIMEOUT_S="120")     # a rank that dies ends the others, nobody parks


# ---- CPU: the constant, and a box without a GPU
def test_ipc_transport_constant_in_python_header_and_fortran():
    assert abi.HALO_IPC == 2 and len({abi.HALO_TCP, abi.HALO_RCCL, abi.HALO_IPC}) == 3
    hdr = open(os.path.join(ROOT, "include", "noahmp_hip.h")).read()
    assert re.search(r"^#define NOAHMP_HALO_IPC\s+2\s*$", hdr, re.M)
    f90 = open(os.path.join(ROOT, "noahmp_amd", "fortran", "module_sf_noahmpdrv_hip.F90")).read()
    assert re.search(r"integer\(c_int\), parameter ::.*\bNOAHMP_HALO_IPC = 2\b", f90)


def _no_device_worker(rank, world, port, barrier, q):
    os.environ["NMP_HALO_TIMEOUT_S"] = "4"
    lib = abi.load_library()
    if lib.noahmp_hip_device_count() > 0:
        barrier.wait(60)
        q.put((rank, "gpu", 0, 0.0, ""))
        return
    barrier.wait(60)                      # both ranks are at the call: the time below is the transport's, not a start-up's
    t0 = time.monotonic()
    rc = lib.noahmp_hip_halo_init(rank, world, b"127.0.0.1", port, abi.HALO_IPC)
    q.put((rank, "cpu", rc, time.monotonic() - t0, lib.noahmp_hip_last_error().decode()))
    lib.noahmp_hip_halo_finalize()


def test_ipc_init_without_a_device_fails_on_every_rank_in_time():
    """Two ranks ask for the IPC transport on a box without a GPU: both fail within NMP_HALO_TIMEOUT_S (the collective abort of the
    rendezvous), each saying that the IPC transport has no HIP device; nothing hangs."""
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    barrier = ctx.Barrier(world)
    p = _free_port()
    procs = [ctx.Process(target=_no_device_worker, args=(r, world, p, barrier, q)) for r in range(world)]
    for pr in procs:
        pr.start()
    res = [q.get(timeout=120) for _ in range(world)]
    for pr in procs:
        pr.join(30)
        assert pr.exitcode == 0
    if any(kind == "gpu" for _, kind, _, _, _ in res):
        pytest.skip("a GPU is visible: the no-device path is not reachable here")
    for rank, _, rc, dt, msg in res:
        assert rc != 0, (rank, msg)
        assert "IPC transport" in msg and "no HIP device" in msg, (rank, msg)
        assert dt < 4.0, (rank, dt, msg)


# ---- GPU: exchanges on device planes, TCP and IPC transports in the same worker processes
def _exchange_worker(rank, world, ports, q):
    try:
        _gpu_env()
        import torch
        lib = abi.load_library()
        assert lib.noahmp_hip_set_device(0) == 0, lib.noahmp_hip_last_error().decode()
        torch.cuda.set_device(0)
        stream = torch.cuda.Stream()
        res = {}
        for name, transport, port in (("tcp", abi.HALO_TCP, ports[0]), ("ipc", abi.HALO_IPC, ports[1])):
            rc = lib.noahmp_hip_halo_init(rank, world, b"127.0.0.1", port, transport)
            assert rc == 0, "%s init: %s" % (name, lib.noahmp_hip_last_error().decode())
            res[name] = _run_calls(lib, rank, world, stream, CALLS)
            assert lib.noahmp_hip_halo_finalize() == 0
        q.put((rank, res))
    except Exception:                                            # noqa: BLE001  (report, then leave: the peers' sockets close)
        q.put((rank, traceback.format_exc()))


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 4, 8, 9])        # 8 = the north-star 4 x 2 grid; 9 = 3 x 3: the centre rank has eight neighbours
def test_ipc_exchange_on_device_planes_equals_the_global_field(world):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ports = (_free_port(), _free_port())
    procs = [ctx.Process(target=_exchange_worker, args=(r, world, ports, q)) for r in range(world)]
    for pr in procs:
        pr.start()
    res = dict(q.get(timeout=600) for _ in range(world))
    for pr in procs:
        pr.join(60)
        assert pr.exitcode == 0
    for rank in range(world):
        r = res[rank]
        assert isinstance(r, dict), "rank %d:\n%s" % (rank, r)
        for name in ("tcp", "ipc"):
            assert len(r[name]) == len(CALLS), (rank, name, r[name][-1])
            for c, (rc, msg, ok, _) in enumerate(r[name]):
                assert rc == 0 and ok, "rank %d %s call %d %s: rc=%d %s" % (rank, name, c, CALLS[c], rc, msg)
        assert [d for *_, d in r["tcp"]] == [d for *_, d in r["ipc"]], rank


# ---- GPU: host planes are refused and leave the mover usable; init / finalize twice in the same processes
def _reinit_worker(rank, world, ports, q):
    try:
        import ctypes as C
        _gpu_env()
        import torch
        lib = abi.load_library()
        assert lib.noahmp_hip_set_device(0) == 0
        torch.cuda.set_device(0)
        stream = torch.cuda.Stream()
        out = []
        for cycle, port in enumerate(ports):
            rc = lib.noahmp_hip_halo_init(rank, world, b"127.0.0.1", port, abi.HALO_IPC)
            assert rc == 0, lib.noahmp_hip_last_error().decode()
            host = None
            if cycle == 0:                                        # host planes: refused before anything is sent or launched
                geo = tile_geometry(*_grid("probe", world), world, rank, halo=1)
                f = np.full((geo["jme"] - geo["jms"] + 1, geo["ime"] - geo["ims"] + 1), 5.0, dtype=np.float32)
                before = f.copy()
                ptrs = (C.c_void_p * 1)(f.ctypes.data)
                idx = (C.c_int32 * 8)(*[geo[k] for k in IDX8])
                hrc = lib.noahmp_hip_exchange_halo(1, ptrs, idx, abi.MEM_HOST, None)
                host = (hrc, lib.noahmp_hip_last_error().decode(), bool(np.array_equal(f, before)))
            calls = _run_calls(lib, rank, world, stream, [("probe", 2), ("cfg4", 1), ("probe", 3)])
            out.append((host, calls, lib.noahmp_hip_halo_finalize()))
        q.put((rank, out))
    except Exception:                                            # noqa: BLE001
        q.put((rank, traceback.format_exc()))


@pytest.mark.gpu
def test_ipc_host_planes_refused_and_reinit_twice():
    world = 4
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ports = (_free_port(), _free_port())
    procs = [ctx.Process(target=_reinit_worker, args=(r, world, ports, q)) for r in range(world)]
    for pr in procs:
        pr.start()
    res = dict(q.get(timeout=600) for _ in range(world))
    for pr in procs:
        pr.join(60)
        assert pr.exitcode == 0
    for rank in range(world):
        r = res[rank]
        assert isinstance(r, list) and len(r) == 2, "rank %d:\n%s" % (rank, r)
        hrc, hmsg, untouched = r[0][0]
        assert hrc == -109 and "device-resident" in hmsg and untouched, (rank, hrc, hmsg)
        for cycle, (_, calls, frc) in enumerate(r):
            assert frc == 0 and len(calls) == 3, (rank, cycle, calls)
            assert all(rc == 0 and ok for rc, _, ok, _ in calls), (rank, cycle, calls)


# ---- GPU: the config-4 chain on the HIP engine, ring moved by Comm(halo="ipc")
FORCING = ("coszin", "swdown", "glw", "t3d", "qv3d", "u_phy", "v_phy", "p8w3d", "dz8w", "rainbl")


def _cfg4_engine_worker(rank, world, port, gx, gy, nsteps, q):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    _gpu_env()
    import torch
    from noahmp_amd.driver import Engine
    from noahmp_amd.parallel import Comm
    from noahmp_amd.state import ModelConfig
    from noahmp_amd.tables import load_tables
    comm = Comm(backend="gloo", device_index=0, halo="ipc")
    try:
        T, tb = load_tables("usgs")
        eng = Engine(T, device=0)
        torch.cuda.set_device(0)
        cfg = ModelConfig(iopt_run=5)
        geo = comm.my_geometry(gx, gy)
        nx, ny = geo["ime"] - geo["ims"] + 1, geo["jme"] - geo["jms"] + 1
        s = synth.config3_tile(tb, gx, gy, geo["ims"] - 1, geo["jms"] - 1, nx, ny, cfg=cfg, groundwater=True)
        s.set_index(**{k: geo[k] for k in ("ids", "ide", "jds", "jde", "ims", "ime", "jms", "jme", "its", "ite", "jts", "jte")})
        synth.first_step_fixups(s)
        ring = _ring_mask(geo)
        for k in ("zwtxy", "fdepth", "topo"):               # only the exchange may provide the ring
            s.a[k][ring] = np.nan
        s.a["isltyp"][ring] = -7
        try:
            comm.exchange_halo([torch.from_numpy(s.a["zwtxy"])], geo)
            refused = None
        except ValueError as e:
            refused = str(e)
        sd = s.to_device("cuda:0")
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            comm.exchange_halo([sd.a[k] for k in ("fdepth", "topo", "isltyp")], geo)
            for it in range(1, nsteps + 1):
                synth.diurnal_forcing(s, (it + 5) % 24, t_offset=s.t_offset)
                st.synchronize()
                for k in FORCING:
                    sd.a[k].copy_(torch.from_numpy(np.ascontiguousarray(s.a[k])))
                assert eng.noahmplsm(sd, it, 2000, 180.0, stream=st.cuda_stream).code == 0
                comm.exchange_halo([sd.a["zwtxy"]], geo)
                eng.wtable_mmf(sd, stream=st.cuda_stream)
        st.synchronize()
        h = sd.to_host()
        j0, j1 = geo["jts"] - geo["jms"], geo["jte"] - geo["jms"] + 1
        i0, i1 = geo["its"] - geo["ims"], geo["ite"] - geo["ims"] + 1
        part = {k: v[j0:j1, ..., i0:i1].copy() for k, v in h.a.items() if k != "dzs" and (k not in FIELD_INFO or FIELD_INFO[k][2] != "in")}
        res = (geo, part, comm.probe_halo(), refused)
    except Exception:                                            # noqa: BLE001
        res = traceback.format_exc()
    parts = comm.gather_to_root(res)
    if rank == 0:
        q.put(parts)
    comm.close()


@pytest.mark.gpu
@pytest.mark.parametrize("world", [8, 9])
def test_config4_chain_on_the_engine_with_the_ipc_mover(world, port, tables):
    gx, gy, nsteps = 70, 130, 3
    from noahmp_amd.state import ModelConfig
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = _free_port()
    procs = [ctx.Process(target=_cfg4_engine_worker, args=(r, world, p, gx, gy, nsteps, q)) for r in range(world)]
    for pr in procs:
        pr.start()
    parts = q.get(timeout=600)
    for pr in procs:
        pr.join(60)
        assert pr.exitcode == 0
    for r, x in enumerate(parts):
        assert isinstance(x, tuple), "rank %d:\n%s" % (r, x)
    g = synth.config3_tile(tables[1], gx, gy, cfg=ModelConfig(iopt_run=5), groundwater=True)
    synth.first_step_fixups(g)
    for it in range(1, nsteps + 1):
        synth.diurnal_forcing(g, (it + 5) % 24, t_offset=g.t_offset)
        assert port.noahmplsm(g, it, 2000, 180.0).code == 0
        port.wtable_mmf(g)
    assert (g.a["qslat"] != 0).any()
    for geo, part, mover, refused in parts:
        assert mover == "noahmp_hip_exchange_halo (IPC transport, one phase)"
        assert refused and "device-resident" in refused
        for k, v in part.items():
            want = g.a[k][geo["jts"] - 1:geo["jte"], ..., geo["its"] - 1:geo["ite"]]
            assert np.array_equal(want, v, equal_nan=True), "%s tile its=%d jts=%d" % (k, geo["its"], geo["jts"])
