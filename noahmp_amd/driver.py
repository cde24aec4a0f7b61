"""Host-side mirror of the reference's operator interface for the hot path.

``noahmplsm(store, itimestep, yr, julian)`` has the meaning of
``module_sf_noahmpdrv :: noahmplsm`` (reference drv:11): one call advances every land column
of the tile by one timestep.  It packs the caller's arrays into the C-ABI block and calls the
HIP engine -- nothing else.  A fatal column raises :class:`NoahMPFatal` (the reference STOPs via
wrf_error_fatal, util/module_wrf_utilities.F:12-24).
"""
import ctypes as C
import os

from . import abi
from .state import DeviceColumnStore


class NoahMPFatal(RuntimeError):
    def __init__(self, code, i, j, msg):
        super().__init__("Noah-MP fatal %d (%s) at I=%d J=%d: %s" % (code, abi.error_name(code), i, j, msg))
        self.code, self.i, self.j = code, i, j


def _fill(block, keep):
    """block.<name> = the address of keep[name] (NULL for None); the tensors live as long as the block."""
    for name, t in keep.items():
        setattr(block, name, t.data_ptr() if t is not None else None)
    block._keep = keep


class Engine:
    """Thin handle on libnoahmp_hip.so (one per process == one per GPU/MPI rank)."""

    def __init__(self, tables, device=None, lib_path=None):
        self.lib = abi.load_library(lib_path)
        if self.lib.noahmp_hip_device_count() < 1:
            raise RuntimeError("Noah-MP HIP engine: no GPU visible and there is no CPU fallback")
        if device is not None:
            rc = self.lib.noahmp_hip_set_device(int(device))
            if rc:
                raise RuntimeError(self.lib.noahmp_hip_last_error().decode())
        self.tables = tables
        rc = self.lib.noahmp_hip_set_tables(C.byref(tables))
        if rc:
            raise RuntimeError("noahmp_hip_set_tables: " + self.lib.noahmp_hip_last_error().decode())
        self.last_status = abi.Status()
        if os.environ.get("NMP_JIT") in ("0", "1"):          # run-time specialisation for every option set (noahmp_jit.hip)
            self.set_option("jit_option_kernels", int(os.environ["NMP_JIT"]))

    @property
    def exact_libm(self):
        """True if the library was built with the reference libm's algorithms (bit-identical results)."""
        return self.lib.noahmp_hip_set_option(b"exact_libm", -1) == 1

    def _call(self, name, *args):
        """lib.<name>(*args); a return code other than 0 raises with the library's text."""
        rc = getattr(self.lib, name)(*args)
        if rc:
            raise RuntimeError("%s: rc=%d %s" % (name, rc, self.lib.noahmp_hip_last_error().decode()))

    def set_option(self, key, value):
        return self.lib.noahmp_hip_set_option(key.encode(), int(value))

    def _apply_ranges(self, ranges):
        """Declare (or withdraw) the class ranges of the store about to be stepped (set_option sorted_*_columns)."""
        if ranges != getattr(self.lib, "_ranges_set", None):          # the engine is one per process: remember it on the library
            n0, n1 = ranges if ranges else (-1, -1)
            self.lib.noahmp_hip_set_option(b"sorted_land_columns", int(n0))
            self.lib.noahmp_hip_set_option(b"sorted_glacier_columns", int(n1))
            self.lib._ranges_set = ranges

    def fetch(self):
        """Bring the host arrays of a resident run ("resident_state" + "lazy_download") up to date."""
        self._call("noahmp_hip_fetch", None)

    def noahmplsm(self, store, itimestep, yr, julian, stream=None, check=True):
        a = store.step_args(itimestep, yr, julian)
        mem = abi.MEM_DEVICE if isinstance(store, DeviceColumnStore) else abi.MEM_HOST
        self._apply_ranges(a._ranges if mem == abi.MEM_DEVICE else None)
        st = abi.Status()
        rc = self.lib.noahmp_hip_step(C.byref(a), mem, stream, C.byref(st))
        self.last_status = st
        if rc < 0:
            raise RuntimeError("noahmp_hip_step: " + self.lib.noahmp_hip_last_error().decode())
        if rc > 0 and check:
            raise NoahMPFatal(rc, st.i, st.j, self.lib.noahmp_hip_error_string(rc).decode())
        return st

    def noahmp_init(self, store, fndsnowh=True, stream=None, check=True):
        """Cold start on the device: NOAHMP_INIT's per-column part + SNOW_INIT (reference drv:988-1283), in place.
        ide+1 / jde+1 are passed as the reference driver does (hdrv:291; the routine loops to min(ite, ide-1))."""
        a = store.step_args(1, 2000, 1.0)
        a.ide += 1
        a.jde += 1
        mem = abi.MEM_DEVICE if isinstance(store, DeviceColumnStore) else abi.MEM_HOST
        st = abi.Status()
        rc = self.lib.noahmp_hip_init(C.byref(a), store.cfg.iswater, 1 if fndsnowh else 0, mem, stream, C.byref(st))
        self.last_status = st
        if rc < 0:
            raise RuntimeError("noahmp_hip_init: " + self.lib.noahmp_hip_last_error().decode())
        if rc > 0 and check:
            raise NoahMPFatal(rc, st.i, st.j, "lsminit: out of range value of ISLTYP (drv:1018)")
        return st

    def wtable_mmf(self, store, stream=None):
        """WTABLE_mmf_noahmp (reference gw:14): lateral groundwater flow + water-table update, in place.
        A decomposed domain must have exchanged the ZWTXY halo first (parallel.exchange_halo)."""
        w = store.wtable_args()
        mem = abi.MEM_DEVICE if isinstance(store, DeviceColumnStore) else abi.MEM_HOST
        st = abi.Status()
        rc = self.lib.noahmp_hip_wtable_mmf(C.byref(w), mem, stream, C.byref(st))
        self.last_status = st
        if rc:
            raise RuntimeError("noahmp_hip_wtable_mmf: rc=%d %s" % (rc, self.lib.noahmp_hip_last_error().decode()))
        return st

    def wtable_mmf_async(self, wargs, stream=None):
        """Enqueue one WTABLE_mmf_noahmp call described by a prepared WtableArgs block (store.wtable_args(), device pointers)."""
        self._call("noahmp_hip_wtable_mmf_async", C.byref(wargs), stream)

    def wtable_lateral_async(self, wargs, qlat, stream=None):
        """First half of WTABLE_mmf_noahmp for a sorted run: KCELL / HEAD + the QLAT stencil on the TILE-order planes of `wargs`
        (wtd, fdepth, topo, isltyp with the ring; xland, xice, ivgtyp, area) -> `qlat` (device tensor shaped like the memory block)."""
        self._call("noahmp_hip_wtable_lateral_async", C.byref(wargs), qlat.data_ptr(), stream)

    def wtable_columns_async(self, wargs, qlat, stream=None):
        """Second half: river flux, deep recharge, UPDATEWTD and the accumulators on a block whose columns are in any order, QLAT
        taken from `qlat` (same order)."""
        self._call("noahmp_hip_wtable_columns_async", C.byref(wargs), qlat.data_ptr(), stream)

    def forcing_prep(self, store, lon, rain_rate, iday, ihour, iminute=0, isecond=0, scale_vegfra=False, stream=None,
                     first_step=False, wait=True):
        """Device-resident forcing preparation (reference hdrv:336-354 + CALC_DECLIN): `lon` and `rain_rate` are
        device tensors shaped like a 2-D field; level 1 of t3d/qv3d/u_phy/v_phy/p8w3d holds the new forcing.
        first_step adds the driver's itime = 1 guesses of EAH / TAH / CH / CM (hdrv:374-384).  Returns JULIAN."""
        assert isinstance(store, DeviceColumnStore), "forcing_prep works on device-resident arrays"
        a = store.step_args(1, 2000, 1.0)
        jul = C.c_float(0)
        st = abi.Status()
        rc = self.lib.noahmp_hip_forcing_prep(C.byref(a), lon.data_ptr(), rain_rate.data_ptr(), iday, ihour, iminute,
                                              isecond, store.cfg.zlvl, (1 if scale_vegfra else 0) | (2 if first_step else 0), C.byref(jul),
                                              abi.MEM_DEVICE, stream, C.byref(st) if wait else None)
        self.last_status = st
        if rc:
            raise RuntimeError("noahmp_hip_forcing_prep: rc=%d %s" % (rc, self.lib.noahmp_hip_last_error().decode()))
        return jul.value

    def forcing_interpolate(self, store, rec_a, rec_b, idts, idts2, rain_rate, stream=None, wait=True):
        """Device-resident hrldas_input_interpolate / hrldas_input_copy (netcdf_io:1351-1403): `rec_a`, `rec_b` are
        dicts of device tensors keyed t q u v p lw sw pcp [fpar lai] (rec_b None = take rec_a as it is); `rain_rate`
        receives RAINBL_tmp.  Follow with forcing_prep(scale_vegfra=True)."""
        assert isinstance(store, DeviceColumnStore), "forcing_interpolate works on device-resident arrays"
        a = store.step_args(1, 2000, 1.0)

        def rec(d):
            r = abi.ForcingRecord()
            for n in abi.FORCING_RECORD_FIELDS:
                if d.get(n) is not None:
                    setattr(r, n, d[n].data_ptr())
            return r
        ra = rec(rec_a)
        rb = rec(rec_b) if rec_b is not None else None
        st = abi.Status()
        rc = self.lib.noahmp_hip_forcing_interpolate(C.byref(a), C.byref(ra), C.byref(rb) if rb is not None else None,
                                                     idts, idts2, rain_rate.data_ptr(), abi.MEM_DEVICE, stream,
                                                     C.byref(st) if wait else None)
        self.last_status = st
        if rc:
            raise RuntimeError("noahmp_hip_forcing_interpolate: rc=%d %s" % (rc, self.lib.noahmp_hip_last_error().decode()))
        return st

    def forcing_interpolate_prep(self, store, rec_a, rec_b, idts, idts2, rain_rate, lon, iday, ihour, iminute=0, isecond=0,
                                 scale_vegfra=False, first_step=False, stream=None, wait=True):
        """forcing_interpolate followed by forcing_prep in one launch (noahmp_hip_forcing_interpolate_prep): same arguments, same
        results.  Returns JULIAN."""
        assert isinstance(store, DeviceColumnStore), "forcing_interpolate_prep works on device-resident arrays"
        a = store.step_args(1, 2000, 1.0)

        def rec(d):
            r = abi.ForcingRecord()
            for n in abi.FORCING_RECORD_FIELDS:
                if d.get(n) is not None:
                    setattr(r, n, d[n].data_ptr())
            return r
        ra = rec(rec_a)
        rb = rec(rec_b) if rec_b is not None else None
        jul = C.c_float(0)
        st = abi.Status()
        rc = self.lib.noahmp_hip_forcing_interpolate_prep(C.byref(a), C.byref(ra), C.byref(rb) if rb is not None else None, idts, idts2,
                                                          rain_rate.data_ptr(), lon.data_ptr(), iday, ihour, iminute, isecond, store.cfg.zlvl,
                                                          (1 if scale_vegfra else 0) | (2 if first_step else 0), C.byref(jul), abi.MEM_DEVICE,
                                                          stream, C.byref(st) if wait else None)
        self.last_status = st
        if rc:
            raise RuntimeError("noahmp_hip_forcing_interpolate_prep: rc=%d %s" % (rc, self.lib.noahmp_hip_last_error().decode()))
        return jul.value

    # ---- sorted device-resident layout
    class Gather:
        """A prepared noahmp_hip_gather_fields call: dst tensors <- src tensors through a column permutation."""

        def __init__(self, lib, dst, src, perm, ni, nj):
            n = len(dst)
            self.lib, self.n, self.ni, self.nj, self.perm = lib, n, ni, nj, perm
            self.keep = (dst, src)
            self.dst = (C.c_void_p * n)(*[t.data_ptr() for t in dst])
            self.src = (C.c_void_p * n)(*[t.data_ptr() for t in src])
            self.nlev = (C.c_int * n)(*[(t.shape[1] if t.dim() == 3 else 1) for t in dst])

        def set_sources(self, src):
            for i, t in enumerate(src):
                self.src[i] = t.data_ptr()

        def set_dests(self, dst):
            """other destination tensors of the same shapes (e.g. the second of two forcing working sets)"""
            for i, t in enumerate(dst):
                self.dst[i] = t.data_ptr()

        def __call__(self, stream=None):
            rc = self.lib.noahmp_hip_gather_fields(self.n, self.dst, self.src, self.nlev, self.perm.data_ptr(), self.ni,
                                                   self.nj, stream)
            if rc:
                raise RuntimeError("noahmp_hip_gather_fields: rc=%d" % rc)

    def stream_sync(self, stream=None):
        """Wait for `stream` (None: the engine's own stream)."""
        rc = self.lib.noahmp_hip_stream_sync(stream)
        if rc:
            raise RuntimeError("noahmp_hip_stream_sync: " + self.lib.noahmp_hip_last_error().decode())

    def set_veg_order(self, first=None, ncat=64):
        """Order of the vegetation categories inside the land range of later sorts (noahmp_hip_sort_set_veg_order): `first` = categories
        in the order their columns should RUN (e.g. the expensive ones first, so that cheap waves form the tail of a launch); categories
        it does not name follow in numeric order.  None: the categories' own numbers."""
        if not first:
            rc = self.lib.noahmp_hip_sort_set_veg_order(None, 0)
        else:
            seq = [int(v) for v in first] + [v for v in range(ncat) if v not in set(int(x) for x in first)]
            rank = (C.c_int32 * ncat)()
            for place, v in enumerate(seq[:ncat]):
                rank[v] = place
            rc = self.lib.noahmp_hip_sort_set_veg_order(rank, ncat)
        if rc:
            raise RuntimeError("noahmp_hip_sort_set_veg_order: " + self.lib.noahmp_hip_last_error().decode())

    def sort_store(self, store, tsk_bin=1.0, veg=True, snow=True, snow_first=False, allow_lateral=False, tair=False, band=None, cost=False):
        """Reorder a DeviceColumnStore in place so that columns with equal (class, vegetation type, snow-layer count,
        skin-temperature bin) are adjacent, and return the permutation as an int32 device tensor: sorted position p holds the
        column that sits at linear tile index perm[p] of the ORIGINAL tile order (a second call on an already sorted
        store re-sorts it and returns the composed permutation).  Key, stable radix sort and the permutation of every
        array run on the device (noahmp_hip_sort_columns / noahmp_hip_permute_step_arrays).  Columns are independent
        (every option except the MMF lateral flow), so this only changes which lane computes which column; wavefronts
        then hold columns that take the same branches: class and vegetation type select code paths and are static, the
        snow-layer count bounds the layer loops and changes slowly (see sort_staleness), the skin temperature (`tsk_bin`
        K wide bins, 0 = off) is a cheap proxy for the stability / freezing regime a column is in.  Forcing that arrives
        in tile order goes through `scatter`.  band: name of an int32 device plane of the store (values 0..31, static; it is
        permuted with the state) used as a sub-key between the snow-layer count and the temperature bin (noahmp_hip_sort_set_band: an argument of the next sort / staleness call, consumed by it),
        e.g. the 15-degree longitude band of a lat/lon grid: a wavefront's columns then share their local solar time."""
        import numpy as np
        import torch
        assert isinstance(store, DeviceColumnStore)
        # the stencil of WTABLE_mmf_noahmp needs the (i,j) neighbourhood: a sorted OPT_RUN=5 store must return its planes to
        # tile order around every groundwater call (Engine.wtable_mmf_sorted)
        assert store.cfg.iopt_run != 5 or allow_lateral, "OPT_RUN=5 needs the (i,j) order for WTABLE_mmf_noahmp"
        n = store.ncol
        flags = ((abi.SORT_VEG if veg else 0) | (abi.SORT_SNOW if snow else 0) | (abi.SORT_SNOW_FIRST if snow_first else 0) |
                 (abi.SORT_TAIR if tair else 0) |        # tair: temperature bins from the forcing air temperature instead of TSK
                 (abi.SORT_COST if cost else 0))         # cost: bucket of the columns' own trip counts in the last step (set_option record_cost)
        a = store.step_args(1, 2000, 1.0)
        perm = torch.empty(n, dtype=torch.int32, device=store.device)
        keys = torch.empty(n, dtype=torch.int32, device=store.device)
        counts = (C.c_int64 * 3)()
        torch.cuda.current_stream().synchronize()          # tensors written by torch kernels are read on the engine's stream
        self.lib.noahmp_hip_sort_set_band(store.a[band].data_ptr() if band else None)
        self._call("noahmp_hip_sort_columns", C.byref(a), flags, int(round(tsk_bin * 1000)) if tsk_bin else 0,
                                              perm.data_ptr(), keys.data_ptr(), counts, None)
        # The sorted block's arrays are carved out of ONE allocation, packed back to back (256-byte aligned, each start one odd multiple of
        # 256 B further): separately allocated planes all start on 2 MiB boundaries, so the words of one column sit at the same offset in
        # 2 MiB-aligned regions of all 115 arrays -- the column kernel's wavefront then asks for 206 lines whose low address bits agree.
        # A/B on one box (round 6): column kernel 3.235 / 3.234 -> 3.215 / 3.212 / 3.212 ms (-0.7 %) whatever the shift (256 B .. 70 KB).
        pad = int(os.environ.get("NMP_POOL_SHIFT", "4352"))         # 17 x 256 B; 0 = separate allocations (rounds 2-5)
        if pad:
            ten = [(k, v) for k, v in store.a.items() if not isinstance(v, np.ndarray)]
            tot = sum(((v.numel() * v.element_size() + 255) // 256) * 256 + pad for k, v in ten) + 4096
            pool = torch.empty(tot, dtype=torch.uint8, device=store.device)
            new, off = {}, 0
            for k, v in ten:
                off += pad
                nb = v.numel() * v.element_size()
                new[k] = pool[off:off + nb].view(v.dtype).view(v.shape)
                off += ((nb + 255) // 256) * 256
            for k, v in store.a.items():
                if isinstance(v, np.ndarray):
                    new[k] = v
        else:
            new = {k: (v if isinstance(v, np.ndarray) else torch.empty_like(v)) for k, v in store.a.items()}
        old = store.a
        store.a = new
        b = store.step_args(1, 2000, 1.0)
        rc = self.lib.noahmp_hip_permute_step_arrays(C.byref(a), C.byref(b), perm.data_ptr(), None)
        if rc:
            store.a = old
            raise RuntimeError("noahmp_hip_permute_step_arrays: rc=%d %s" % (rc, self.lib.noahmp_hip_last_error().decode()))
        extra = [k for k in old if k not in abi.FIELD_INFO and not isinstance(old[k], np.ndarray)]    # e.g. the MMF planes
        for i in range(0, len(extra), 32):
            chunk = extra[i:i + 32]
            Engine.Gather(self.lib, [new[k] for k in chunk], [old[k] for k in chunk], perm, store.ni, store.nj)()
        prev = getattr(store, "sort_perm", None)
        if prev is not None:                                 # already sorted: compose with the earlier permutation
            total = torch.empty_like(perm)
            Engine.Gather(self.lib, [total], [prev], perm, store.ni, store.nj)()
            perm = total
        self.stream_sync()
        # classes are contiguous now: land, land ice, skipped -- each range gets its own kernel (noahmp_engine.hip, launch_any)
        store.class_ranges = (int(counts[0]), int(counts[1]))
        store.sort_perm, store.sort_keys, store.sort_flags, store.sort_band = perm, keys, flags, band
        return perm

    def sort_staleness(self, store):
        """Number of columns of a sorted store whose (class, vegetation type, snow-layer count) no longer is what they were
        sorted by -- snow layers that appeared or vanished (lsm:7044, 7110, 7177, 7294-7343).  Waits for the engine's stream."""
        a = store.step_args(1, 2000, 1.0)
        changed = C.c_int64(0)
        band = getattr(store, "sort_band", None)
        self.lib.noahmp_hip_sort_set_band(store.a[band].data_ptr() if band else None)      # the key the store was sorted by
        self._call("noahmp_hip_sort_staleness", C.byref(a), store.sort_flags, store.sort_keys.data_ptr(), C.byref(changed), None)
        return int(changed.value)

    def sort_staleness_async(self, store, stream=None):
        """sort_staleness without the wait: enqueued on `stream`, read later with sort_staleness_result (a check that drains the
        stream idles the GPU while the host refills its queue)."""
        a = store.step_args(1, 2000, 1.0)
        band = getattr(store, "sort_band", None)
        self.lib.noahmp_hip_sort_set_band(store.a[band].data_ptr() if band else None)
        self._call("noahmp_hip_sort_staleness_async", C.byref(a), store.sort_flags, store.sort_keys.data_ptr(), stream)

    def sort_staleness_result(self, wait=True):
        """The count sort_staleness_async asked for; None if it has not arrived and wait is False."""
        changed = C.c_int64(0)
        rc = self.lib.noahmp_hip_sort_staleness_result(C.byref(changed), 1 if wait else 0)
        if rc == 1:
            return None
        if rc:
            raise RuntimeError("noahmp_hip_sort_staleness_result: rc=%d %s" % (rc, self.lib.noahmp_hip_last_error().decode()))
        return int(changed.value)

    def gather(self, dst, src, perm, ni, nj):
        return Engine.Gather(self.lib, dst, src, perm, ni, nj)

    class Scatter(Gather):
        """The same permutation through noahmp_hip_scatter_fields (chunked, LDS-staged, sorted write order): the form
        to use for records that arrive every step."""

        def __init__(self, lib, dst, src, perm, ni, nj):
            Engine.Gather.__init__(self, lib, dst, src, perm, ni, nj)
            self.set_perm(perm)

        def set_perm(self, perm):
            """(Re)build the plan for `perm` on the device (noahmp_hip_scatter_plan); waits for it."""
            import torch
            n = perm.numel()
            self.perm = perm
            self.order = torch.empty(n, dtype=torch.int16, device=perm.device)
            self.dpos = torch.empty(n, dtype=torch.int32, device=perm.device)
            rc = self.lib.noahmp_hip_scatter_plan(perm.data_ptr(), self.ni, self.nj, self.order.data_ptr(), self.dpos.data_ptr(), None)
            if rc == 0:
                rc = self.lib.noahmp_hip_stream_sync(None)
            if rc:
                raise RuntimeError("noahmp_hip_scatter_plan: rc=%d" % rc)

        def __call__(self, stream=None):
            rc = self.lib.noahmp_hip_scatter_fields(self.n, self.dst, self.src, self.nlev, self.order.data_ptr(),
                                                    self.dpos.data_ptr(), self.ni, self.nj, stream)
            if rc:
                raise RuntimeError("noahmp_hip_scatter_fields: rc=%d" % rc)

        def exchange(self, sorted_planes, tile_planes, to_tile, ni_mem=None, i_off=0, j_off=0, stream=None, first_level_only=()):
            """Move planes between the sorted store and TILE-order planes (possibly the interior of a memory block that carries
            the LATERALFLOW ring: rows ni_mem long, tile origin at (i_off, j_off)) with this permutation's plan
            (noahmp_hip_sorted_exchange).  to_tile: sorted -> tile order, else tile order -> sorted.  first_level_only: as in scatter()."""
            n = len(sorted_planes)
            sp = (C.c_void_p * n)(*[t.data_ptr() for t in sorted_planes])
            tp = (C.c_void_p * n)(*[t.data_ptr() for t in tile_planes])
            nl = (C.c_int * n)(*[(t.shape[1] if t.dim() == 3 else 1) for t in sorted_planes])
            for i in first_level_only:
                if nl[i] > 1:
                    nl[i] = -nl[i]
            rc = self.lib.noahmp_hip_sorted_exchange(n, sp, tp, nl, self.order.data_ptr(), self.dpos.data_ptr(), self.ni, self.nj,
                                                     ni_mem or self.ni, i_off, j_off, 1 if to_tile else 0, stream)
            if rc:
                raise RuntimeError("noahmp_hip_sorted_exchange: rc=%d" % rc)

    def scatter(self, dst, src, perm, ni, nj, first_level_only=()):
        """first_level_only: indices of level arrays of which only the first level is moved -- T3D / QV3D / U_PHY / V_PHY / DZ8W only
        (the column kernel reads their level 1, drv:451-459; the driver's level-2 copies, hdrv:336-344, need not travel).  Never
        P8W3D: noahmplsm reads its levels 1 AND 2 (SFCPRS = (P8W3D(kts+1) + P8W3D(kts)) * 0.5, drv:463), so a P8W3D passed this way
        would keep a stale level-2 pressure."""
        sc = Engine.Scatter(self.lib, dst, src, perm, ni, nj)
        for i in first_level_only:
            if sc.nlev[i] > 1:
                sc.nlev[i] = -sc.nlev[i]
        return sc

    # ---- device-side history: interval accumulators and point probes (noahmp_history.hip; helper: noahmp_amd/history.py)
    @staticmethod
    def history_entries(entries):
        """[(src tensor, acc tensor, op, scale), ...] -> a prepared (HistoryEntry * n) array; op = a NOAHMP_HIST_* value or its lower-case
        name ("sum", "sum_dt", "min", "max", "last").  The tensors are kept alive by the returned array."""
        n = len(entries)
        arr = (abi.HistoryEntry * max(n, 1))()
        for f, (src, acc, op, scale) in enumerate(entries):
            arr[f].src = src.data_ptr() if src is not None else None
            arr[f].acc = acc.data_ptr() if acc is not None else None
            arr[f].nlev = acc.shape[1] if (acc is not None and acc.dim() == 3) else 1
            arr[f].op = abi.HIST_OP[op] if isinstance(op, str) else int(op)
            arr[f].scale = float(scale)
        arr._n, arr._keep = n, list(entries)
        return arr

    @staticmethod
    def history_probes(columns, fields, ring, slot=0):
        """A noahmp_history_probes block: `columns` int32 device tensor (linear column indices in the block's current order), `fields` 2-D
        device planes, `ring` float32 device tensor [nslot][nfield][npoint]."""
        p = abi.HistoryProbes()
        fp = (C.c_void_p * max(len(fields), 1))(*[t.data_ptr() for t in fields])
        p.npoint, p.column, p.nfield, p.field, p.ring = int(columns.numel()), columns.data_ptr(), len(fields), fp, ring.data_ptr()
        p.nslot, p.slot = int(ring.shape[0]), int(slot)
        p._keep = (columns, list(fields), ring, fp)
        return p

    def history_step(self, entries, store, probes=None, count=None, stream=None):
        """One sample of every accumulator and one ring slot of the probes after a step of `store` (a DeviceColumnStore, or a prepared
        StepArgs block with device pointers): one kernel launch, enqueued only (noahmp_hip_history_step).  entries: history_entries(...)
        or the list it takes; count: int32 device plane that counts the steps which advanced each column, or None."""
        if not isinstance(entries, C.Array):
            entries = Engine.history_entries(entries)
        a = store if isinstance(store, abi.StepArgs) else store.step_args(1, 2000, 1.0)
        self._call("noahmp_hip_history_step", entries._n, entries, C.byref(probes) if probes is not None else None, C.byref(a),
                                              count.data_ptr() if count is not None else None, stream)

    def history_finish(self, entries, dst, flags, count, store, perm=None, fill=None, mask_water=True, stream=None):
        """Output-time finish (noahmp_hip_history_finish): dst[f] (tile-order device tensors, None = reset only) <- the accumulators,
        flags[f] = "mean" / "reset" names or NOAHMP_HIST_FIN_* bits; perm = tile column -> position in the accumulators' order (the
        inverse of what sort_store returned) or None; water points get -1.E33 (IVGTYP of `store`, which is in the accumulators' order).
        Enqueued only; `count` is not cleared."""
        from .restart import UNDEFINED
        if not isinstance(entries, C.Array):
            entries = Engine.history_entries(entries)
        n = entries._n

        def bits(f):
            if isinstance(f, int):
                return f
            return sum(abi.HIST_FIN[x] for x in ((f,) if isinstance(f, str) else f))
        dp = (C.c_void_p * max(n, 1))(*[(t.data_ptr() if t is not None else None) for t in dst])
        fl = (C.c_uint32 * max(n, 1))(*[bits(f) for f in flags])
        self._call("noahmp_hip_history_finish", n, entries, dp, fl, count.data_ptr() if count is not None else None,
                                                perm.data_ptr() if perm is not None else None,
                                                store.a["ivgtyp"].data_ptr() if mask_water else None, store.cfg.iswater,
                                                float(UNDEFINED if fill is None else fill), store.ni, store.nj, stream)

    # ---- region series: per-step weighted sums / minima / maxima over labelled regions (noahmp_regions.hip; helper: history.py::Regions)
    class RegionPlan:
        """The device workspace noahmp_hip_region_plan filled, and what a step on it needs."""

        def __init__(self, plan, ni, nj, nregion):
            self.plan, self.ni, self.nj, self.nregion = plan, ni, nj, nregion
            self.scratch = None

    def region_plan(self, region_map, nregion, weight=None, inv_perm=None, stream=None):
        """Plan of the regions of a tile (noahmp_hip_region_plan): region_map = int32 device tensor (nj, ni) in TILE order, ids
        0 .. nregion-1, negative = no region; weight = float32 device tensor in tile order or None (= 1); inv_perm[tile index] = position
        of the cell in the block's current column order (int32 device tensor; None = tile order).  Built on the device; waits."""
        import torch
        nj, ni = region_map.shape
        assert region_map.dtype == torch.int32 and (weight is None or weight.dtype == torch.float32)
        words = C.c_int64(0)
        self._call("noahmp_hip_region_plan_size", ni, nj, int(nregion), C.byref(words))
        plan = torch.empty((words.value + 1) // 2, dtype=torch.int64, device=region_map.device).view(torch.int32)
        torch.cuda.current_stream().synchronize()
        self._call("noahmp_hip_region_plan", region_map.data_ptr(), weight.data_ptr() if weight is not None else None, ni, nj, int(nregion),
                                             inv_perm.data_ptr() if inv_perm is not None else None, plan.data_ptr(), plan.numel(), stream)
        return Engine.RegionPlan(plan, ni, nj, int(nregion))

    def region_follow(self, rp, inv_perm, stream=None):
        """After a re-sort: the members' positions for the new column order (noahmp_hip_region_plan_follow; enqueued only)."""
        self._call("noahmp_hip_region_plan_follow", rp.plan.data_ptr(), inv_perm.data_ptr() if inv_perm is not None else None, stream)
        rp.scratch = None

    @staticmethod
    def region_entries(entries):
        """[(src tensor or None = the constant 1, op, level or None), ...] -> a prepared (RegionEntry * n) array; op = a NOAHMP_REG_* value
        or "sum" / "min" / "max"; level: which level of a layered (nj, nlev, ni) array.  The tensors are kept alive by the array."""
        n = len(entries)
        arr = (abi.RegionEntry * max(n, 1))()
        for f, (src, op, level) in enumerate(entries):
            arr[f].src = src.data_ptr() if src is not None else None
            arr[f].nlev = src.shape[1] if (src is not None and src.dim() == 3) else 1
            arr[f].lev = int(level or 0)
            arr[f].op = abi.REG_OP[op] if isinstance(op, str) else int(op)
        arr._n, arr._keep = n, list(entries)
        return arr

    def region_scratch_bytes(self, rp, n):
        b = C.c_int64(0)
        self._call("noahmp_hip_region_scratch_size", rp.plan.data_ptr(), n, C.byref(b))
        return int(b.value)

    def region_step(self, rp, entries, store, series, slot, acc=None, stream=None):
        """One ring slot of every entry after a step of `store` (a DeviceColumnStore or a prepared StepArgs block): series = float64 device
        tensor [nslot][n][nregion], slot % nslot is written; acc = float64 [n][nregion] interval accumulators or None.  Enqueued only
        (noahmp_hip_region_step); the scratch is allocated at the first call on a plan."""
        import torch
        if not isinstance(entries, C.Array):
            entries = Engine.region_entries(entries)
        a = store if isinstance(store, abi.StepArgs) else store.step_args(1, 2000, 1.0)
        need = self.region_scratch_bytes(rp, entries._n)
        if rp.scratch is None or rp.scratch.numel() * 8 < need:
            rp.scratch = torch.empty((need + 7) // 8, dtype=torch.float64, device=rp.plan.device)
            torch.cuda.current_stream().synchronize()
        self._call("noahmp_hip_region_step", rp.plan.data_ptr(), entries._n, entries, C.byref(a), series.data_ptr(), int(series.shape[0]), int(slot),
                                             acc.data_ptr() if acc is not None else None, rp.scratch.data_ptr(), stream)

    # ---- forcing regrid: coarse records -> the model grid's planes (noahmp_regrid.hip; helper: noahmp_amd/regrid.py)
    @staticmethod
    def regrid_source(nx, ny, lon0, lat0, dlon, dlat, periodic_x=False):
        """A noahmp_regrid_source block: regular lat-lon grid, (lon0, lat0) = centre of cell (0, 0), dlat may be negative."""
        g = abi.RegridSource()
        g.nx, g.ny, g.lon0, g.lat0, g.dlon, g.dlat, g.periodic_x = int(nx), int(ny), float(lon0), float(lat0), float(dlon), float(dlat), int(bool(periodic_x))
        return g

    def regrid_plan(self, xlat, xlon, source, valid=None, search_radius=4, stream=None):
        """Plan of a tile against a source grid (noahmp_hip_regrid_plan_latlon): xlat / xlon float32 device tensors (nj, ni) in TILE order,
        valid = uint8 device tensor over the source grid or None.  Returns (plan, unfilled): the int32 workspace -- planes base, near,
        w0..w3 of ni*nj words each, then the count word -- and the number of cells without a source.  Built on the device; waits."""
        import torch
        nj, ni = xlat.shape
        assert xlat.dtype == torch.float32 and xlon.dtype == torch.float32 and xlat.is_contiguous() and xlon.is_contiguous()
        assert valid is None or (valid.dtype == torch.uint8 and valid.is_contiguous() and valid.numel() == source.nx * source.ny)
        words = C.c_int64(0)
        self._call("noahmp_hip_regrid_plan_size", ni, nj, C.byref(words))
        plan = torch.empty(words.value, dtype=torch.int32, device=xlat.device)
        torch.cuda.current_stream().synchronize()
        unfilled = C.c_int32(0)
        self._call("noahmp_hip_regrid_plan_latlon", xlat.data_ptr(), xlon.data_ptr(), ni, nj, C.byref(source),
                                                    valid.data_ptr() if valid is not None else None, int(search_radius), plan.data_ptr(),
                                                    plan.numel(), C.byref(unfilled), stream)
        return plan, int(unfilled.value)

    @staticmethod
    def regrid_entries(entries):
        """[(src tensor, dst tensor, mode, adjust tensor or None, scale, fill), ...] -> a prepared (RegridEntry * n) array; mode = a
        NOAHMP_REGRID_* value or "bilinear" / "nearest".  The tensors are kept alive by the returned array."""
        n = len(entries)
        arr = (abi.RegridEntry * max(n, 1))()
        for f, (src, dst, mode, adjust, scale, fill) in enumerate(entries):
            arr[f].src = src.data_ptr() if src is not None else None
            arr[f].dst = dst.data_ptr() if dst is not None else None
            arr[f].adjust = adjust.data_ptr() if adjust is not None else None
            arr[f].scale, arr[f].fill = float(scale), float(fill)
            arr[f].mode = abi.REGRID_MODE[mode] if isinstance(mode, str) else int(mode)
        arr._n, arr._keep = n, list(entries)
        return arr

    def forcing_regrid(self, plan, ncell, source, entries, stream=None):
        """Every entry's source plane -> its destination plane through `plan` (the workspace regrid_plan returned, or one the caller
        filled or permuted): one kernel launch, enqueued only (noahmp_hip_forcing_regrid)."""
        if not isinstance(entries, C.Array):
            entries = Engine.regrid_entries(entries)
        self._call("noahmp_hip_forcing_regrid", plan.data_ptr(), int(ncell), C.byref(source), entries._n, entries, stream)

    @staticmethod
    def regrid_met(src_t, src_p, src_q, dst_t, dst_p, dst_q, dz, src_lw=None, dst_lw=None, lapse=-0.0065, fill=float("nan")):
        """A noahmp_regrid_met block: the elevation-adjusted group of noahmp_hip_forcing_regrid_met.  src_*: coarse device planes, dst_* and
        dz (model height - regridded source height, metres): ncell values in the plan's column order.  The tensors are kept alive by the
        returned block."""
        m = abi.RegridMet()
        keep = dict(src_t=src_t, src_p=src_p, src_q=src_q, src_lw=src_lw, dst_t=dst_t, dst_p=dst_p, dst_q=dst_q, dst_lw=dst_lw, dz=dz)
        _fill(m, keep)
        m.lapse, m.fill = float(lapse), float(fill)
        return m

    def forcing_regrid_met(self, plan, ncell, source, met, entries, stream=None):
        """forcing_regrid with a met group (Engine.regrid_met): t, p, q and optionally lw regridded and moved to the model's terrain height,
        plus the 0..32 ordinary entries, in one kernel launch, enqueued only (noahmp_hip_forcing_regrid_met)."""
        if not isinstance(entries, C.Array):
            entries = Engine.regrid_entries(entries)
        self._call("noahmp_hip_forcing_regrid_met", plan.data_ptr(), int(ncell), C.byref(source), C.byref(met), entries._n, entries, stream)

    # ---- budget-preserving regrid of fluxes (noahmp_regrid_conserve.hip; helper: noahmp_amd/regrid.py)
    class RegridConservePlan:
        """The device workspace noahmp_hip_regrid_conserve_plan filled, the regrid plan it was made from, and what a record on it needs."""

        def __init__(self, cplan, regrid_plan, ni, nj, source, clipped):
            self.cplan, self.regrid_plan, self.ni, self.nj, self.source, self.clipped = cplan, regrid_plan, ni, nj, source, clipped
            self.scratch = None

    def regrid_conserve_plan(self, regrid_plan, ni, nj, source, area=None, dst_index=None, domain_edges=0b1111, stream=None):
        """Conserve plan of a window (noahmp_hip_regrid_conserve_plan) from its regrid plan in WINDOW order: area = float32 device tensor
        in window order or None (= 1); dst_index = int32 device tensor in window order (negative: a margin cell, summed but not written) or
        None (identity); domain_edges = NOAHMP_REGRID_EDGE_* bits of the window's sides that are edges of the whole model domain.
        Returns a RegridConservePlan; .clipped > 0: widen the margin.  Built on the device; waits."""
        import torch
        assert regrid_plan.dtype == torch.int32 and regrid_plan.numel() >= 6 * ni * nj
        assert area is None or (area.dtype == torch.float32 and area.is_contiguous() and area.numel() == ni * nj)
        assert dst_index is None or (dst_index.dtype == torch.int32 and dst_index.is_contiguous() and dst_index.numel() == ni * nj)
        words = C.c_int64(0)
        self._call("noahmp_hip_regrid_conserve_plan_size", ni, nj, C.byref(source), C.byref(words))
        cplan = torch.empty((words.value + 1) // 2, dtype=torch.int64, device=regrid_plan.device).view(torch.int32)
        torch.cuda.current_stream().synchronize()
        clipped = C.c_int32(0)
        self._call("noahmp_hip_regrid_conserve_plan", regrid_plan.data_ptr(), ni, nj, C.byref(source), area.data_ptr() if area is not None else None,
                                                      dst_index.data_ptr() if dst_index is not None else None, int(domain_edges),
                                                      cplan.data_ptr(), cplan.numel(), C.byref(clipped), stream)
        return Engine.RegridConservePlan(cplan, regrid_plan, ni, nj, source, int(clipped.value))

    @staticmethod
    def regrid_conserve_entries(entries):
        """[(src tensor, dst tensor, pattern tensor or None, fill), ...] -> a prepared (RegridConserveEntry * n) array.  The tensors are
        kept alive by the returned array."""
        n = len(entries)
        arr = (abi.RegridConserveEntry * max(n, 1))()
        for f, (src, dst, pattern, fill) in enumerate(entries):
            arr[f].src = src.data_ptr() if src is not None else None
            arr[f].dst = dst.data_ptr() if dst is not None else None
            arr[f].pattern = pattern.data_ptr() if pattern is not None else None
            arr[f].fill = float(fill)
        arr._n, arr._keep = n, list(entries)
        arr._ndst = min([e[1].numel() for e in entries if e[1] is not None] or [0])
        return arr

    def regrid_conserve_scratch_bytes(self, cp, n):
        b = C.c_int64(0)
        self._call("noahmp_hip_regrid_conserve_scratch_size", cp.cplan.data_ptr(), n, C.byref(b))
        return int(b.value)

    def forcing_regrid_conserve(self, cp, entries, dst_index=None, group_sum=None, stream=None):
        """1..8 entries through a RegridConservePlan (noahmp_hip_forcing_regrid_conserve): at most four launches, enqueued only; the scratch
        is allocated at the first call on a plan.  dst_index: int32 device tensor in window order (the positions of the window cells in the
        destination planes; negative = not written) or None; group_sum: float64 device tensor over the source grid that receives N_s of
        entry 0, or None."""
        import torch
        if not isinstance(entries, C.Array):
            entries = Engine.regrid_conserve_entries(entries)
        need = self.regrid_conserve_scratch_bytes(cp, entries._n)
        if cp.scratch is None or cp.scratch.numel() * 8 < need:
            cp.scratch = torch.empty((need + 7) // 8, dtype=torch.float64, device=cp.cplan.device)
            torch.cuda.current_stream().synchronize()
        self._call("noahmp_hip_forcing_regrid_conserve", cp.cplan.data_ptr(), cp.regrid_plan.data_ptr(), C.byref(cp.source),
                                                         dst_index.data_ptr() if dst_index is not None else None, int(entries._ndst),
                                                         entries._n, entries, group_sum.data_ptr() if group_sum is not None else None,
                                                         cp.scratch.data_ptr(), stream)

    # ---- shortwave forcing: zenith weighting in time, slope and aspect (noahmp_shortwave.hip; helper: noahmp_amd/shortwave.py)
    @staticmethod
    def sun_times(times):
        """[(iday, ihour, iminute, isecond), ...] -> a prepared (SunTime * n) array."""
        n = len(times)
        arr = (abi.SunTime * max(n, 1))()
        for i, (iday, ihour, iminute, isecond) in enumerate(times):
            arr[i].iday, arr[i].ihour, arr[i].iminute, arr[i].isecond = int(iday), int(ihour), int(iminute), int(isecond)
        arr._n = n
        return arr

    def cosz_mean(self, xlat, lon, times, mean, stream=None):
        """mean <- the mean of max(cos zenith, 0) over `times` = [(iday, ihour, iminute, isecond), ...] (1..64 samples of a record's
        interval) for every column of the float32 device planes xlat / lon: one kernel launch, enqueued only (noahmp_hip_forcing_cosz_mean)."""
        if not isinstance(times, C.Array):
            times = Engine.sun_times(times)
        self._call("noahmp_hip_forcing_cosz_mean", xlat.data_ptr(), lon.data_ptr(), xlat.numel(), times._n, times, mean.data_ptr(), stream)
        return mean

    @staticmethod
    def shortwave_block(sw_a, xlat, lon, swdown, sw_b=None, mean_a=None, normal=None, idts=0, idts2=0, mode="zenith", max_ratio=10.0,
                        mu_min=0.05, max_terrain_ratio=5.0, solar_constant=1361.0):
        """A noahmp_shortwave block; normal = (east, north, up) planes or None.  The tensors are kept alive by the returned block."""
        b = abi.Shortwave()
        ne, nn, nu = normal if normal is not None else (None, None, None)
        keep = dict(sw_a=sw_a, sw_b=sw_b, mean_a=mean_a, xlat=xlat, lon=lon, normal_e=ne, normal_n=nn, normal_u=nu, swdown=swdown)
        _fill(b, keep)
        b.idts, b.idts2 = int(idts), int(idts2)
        b.mode = abi.SW_MODE[mode] if isinstance(mode, str) else int(mode)
        b.max_ratio, b.mu_min, b.max_terrain_ratio, b.solar_constant = float(max_ratio), float(mu_min), float(max_terrain_ratio), float(solar_constant)
        return b

    def forcing_shortwave(self, block, ncell, now, stream=None):
        """Downward shortwave of one step from a block of Engine.shortwave_block at now = (iday, ihour, iminute, isecond): one kernel
        launch, enqueued only (noahmp_hip_forcing_shortwave).  Call it after forcing_interpolate[_prep], whose linear SWDOWN it overwrites."""
        t = Engine.sun_times([now])
        self._call("noahmp_hip_forcing_shortwave", C.byref(block), int(ncell), t, stream)

    # ---- cast shadows: terrain ray march and the lit shortwave step (noahmp_shadow.hip, noahmp_shortwave.hip; helper: noahmp_amd/shortwave.py)
    @staticmethod
    def shadow_block(height, xlat, lon, lit, dx, dy, nstep=25, cosalpha=None, sinalpha=None, dst_index=None, mu_min=0.05, height_max=None):
        """A noahmp_shadow block over the (nj, ni) WINDOW planes height / xlat / lon (float32, device): lit = the destination plane,
        dst_index = int32 plane in window order (negative: a margin cell, read but neither marched nor written) or None (identity).
        height_max defaults to the window's maximum (one device-to-host copy; a decomposed run must pass the GLOBAL maximum, the same
        number on every rank).  The tensors are kept alive by the returned block."""
        assert height.dim() == 2 and height.is_contiguous() and xlat.numel() == height.numel() and lon.numel() == height.numel()
        b = abi.Shadow()
        keep = dict(height=height, xlat=xlat, lon=lon, cosalpha=cosalpha, sinalpha=sinalpha, dst_index=dst_index, lit=lit)
        _fill(b, keep)
        b.nj, b.ni = (int(v) for v in height.shape)
        b.nstep = int(nstep)
        b.dx, b.dy, b.mu_min = float(dx), float(dy), float(mu_min)
        b.height_max = float(height_max) if height_max is not None else (float(height.max().item()) if height.numel() else 0.0)
        return b

    def forcing_shadow(self, block, ndst, now, stream=None):
        """The lit plane of a block of Engine.shadow_block at now = (iday, ihour, iminute, isecond): 1.0 where the cell sees the sun, 0.0
        in a cast shadow.  One kernel launch, enqueued only (noahmp_hip_forcing_shadow)."""
        t = Engine.sun_times([now])
        self._call("noahmp_hip_forcing_shadow", C.byref(block), int(ndst), t, stream)

    def forcing_shortwave_lit(self, block, lit, ncell, now, stream=None):
        """forcing_shortwave with the lit plane (ncell floats, the column order of the block's planes) on the direct beam: one kernel
        launch, enqueued only (noahmp_hip_forcing_shortwave_lit)."""
        t = Engine.sun_times([now])
        self._call("noahmp_hip_forcing_shortwave_lit", C.byref(block), lit.data_ptr() if lit is not None else None, int(ncell), t, stream)

    # ---- sky-view factor: horizon scan and the radiation step with it (noahmp_skyview.hip, noahmp_shortwave.hip; helper: noahmp_amd/shortwave.py)
    @staticmethod
    def skyview_directions(ndir):
        """The direction table of the horizon scan: (float32) sin / cos (2 pi q / ndir), q = 0 .. ndir-1, made in float64."""
        import numpy as np
        a = 2.0 * np.pi * np.arange(int(ndir), dtype=np.float64) / int(ndir)
        return np.sin(a).astype(np.float32), np.cos(a).astype(np.float32)

    @staticmethod
    def skyview_block(height, svf, dx, dy, nstep=25, ndir=16, dst_index=None, dir_x=None, dir_y=None):
        """A noahmp_skyview block over the (nj, ni) WINDOW plane height (float32, device): svf = the destination plane, dst_index = int32
        plane in window order (negative: a margin cell, read but neither scanned nor written) or None (identity).  dir_x / dir_y: host
        float32 arrays in grid coordinates; by default Engine.skyview_directions(ndir).  Tensors and arrays are kept alive by the block."""
        import numpy as np
        assert height.dim() == 2 and height.is_contiguous()
        if dir_x is None:
            dir_x, dir_y = Engine.skyview_directions(ndir)
        dir_x, dir_y = (np.ascontiguousarray(v, np.float32) for v in (dir_x, dir_y))
        assert dir_x.size == dir_y.size
        b = abi.Skyview()
        keep = dict(height=height, dst_index=dst_index, svf=svf)
        _fill(b, keep)
        b.dir_x, b.dir_y = dir_x.ctypes.data, dir_y.ctypes.data
        b.nj, b.ni = (int(v) for v in height.shape)
        b.nstep, b.ndir = int(nstep), int(dir_x.size)
        b.dx, b.dy = float(dx), float(dy)
        b._keep = dict(keep, dir_x=dir_x, dir_y=dir_y)
        return b

    def skyview(self, block, ndst, stream=None):
        """The sky-view factor of a block of Engine.skyview_block: 1.0 where a horizontal receiver sees the whole hemisphere.  One kernel
        launch, enqueued only, once per terrain (noahmp_hip_skyview)."""
        self._call("noahmp_hip_skyview", C.byref(block), int(ndst), stream)

    @staticmethod
    def sky_block(svf, lit=None, albedo=0.2, glw=None, tsurf=None, emiss=0.95, sigma=5.67e-8):
        """A noahmp_sky block: svf / lit / glw / tsurf are float32 device planes or None; albedo and emiss a plane or the constant of every
        column.  The tensors are kept alive by the returned block."""
        b = abi.Sky()
        planes = dict(svf=svf, lit=lit, glw=glw, tsurf=tsurf, albedo=None, emiss=None)
        b.albedo_const = b.emiss_const = 0.0
        for name, v in (("albedo", albedo), ("emiss", emiss)):
            if hasattr(v, "data_ptr"):
                planes[name] = v
            else:
                setattr(b, name + "_const", float(v))
        _fill(b, planes)
        b.sigma = float(sigma)
        return b

    def forcing_radiation_sky(self, block, sky, ncell, now, stream=None):
        """forcing_shortwave_lit plus the sky-view terms of the shortwave and the longwave of the closed part of the hemisphere, from a block
        of Engine.shortwave_block and one of Engine.sky_block: one kernel launch, enqueued only (noahmp_hip_forcing_radiation_sky)."""
        t = Engine.sun_times([now])
        self._call("noahmp_hip_forcing_radiation_sky", C.byref(block), C.byref(sky), int(ncell), t, stream)

    # ---- terrain-adjusted wind: slope and curvature of the terrain, and the wind of a record (noahmp_wind.hip; helper: noahmp_amd/wind.py)
    @staticmethod
    def wind_terrain_block(height, sx, sy, curv, dx, dy, ncurv=3, cosalpha=None, sinalpha=None, dst_index=None):
        """A noahmp_wind_terrain block over the (nj, ni) WINDOW plane height (float32, device): sx / sy / curv = the destination planes,
        dst_index = int32 plane in window order (negative: a margin cell, read and not written) or None (identity); cosalpha / sinalpha:
        WRF's rotation planes over the window, both or none.  The tensors are kept alive by the returned block."""
        assert height.dim() == 2 and height.is_contiguous()
        b = abi.WindTerrain()
        keep = dict(height=height, cosalpha=cosalpha, sinalpha=sinalpha, dst_index=dst_index, sx=sx, sy=sy, curv=curv)
        _fill(b, keep)
        b.nj, b.ni = (int(v) for v in height.shape)
        b.ncurv = int(ncurv)
        b.dx, b.dy = float(dx), float(dy)
        return b

    def wind_terrain(self, block, ndst, stream=None):
        """The slope vector (length = the slope angle, pointing uphill) and the curvature of a block of Engine.wind_terrain_block.  One
        kernel launch, enqueued only, once per terrain (noahmp_hip_wind_terrain)."""
        self._call("noahmp_hip_wind_terrain", C.byref(block), int(ndst), stream)

    @staticmethod
    def wind_block(u, v, sx, sy, curv, slope_max, curv_max, gamma_s=0.58, gamma_c=0.42, turn=True):
        """A noahmp_wind block: u / v are adjusted in place; sx / sy / curv are the planes of wind_terrain in the column order of u and v;
        slope_max / curv_max the maxima of the whole run, the same numbers on every rank.  The tensors are kept alive by the block."""
        b = abi.Wind()
        keep = dict(u=u, v=v, sx=sx, sy=sy, curv=curv)
        _fill(b, keep)
        b.slope_max, b.curv_max, b.gamma_s, b.gamma_c = float(slope_max), float(curv_max), float(gamma_s), float(gamma_c)
        b.flags = abi.WIND_FLAG["turn"] if turn else 0
        return b

    def forcing_wind(self, block, ncell, stream=None):
        """The wind of ncell columns weighted by slope and curvature and (with the TURN flag) turned around the obstacle, in place, from a
        block of Engine.wind_block: one kernel launch, enqueued only (noahmp_hip_forcing_wind)."""
        self._call("noahmp_hip_forcing_wind", C.byref(block), int(ncell), stream)

    # ---- runoff routing on a D8 network: directions, upstream bytes, upstream counts, linear reservoirs (noahmp_routing.hip; helper:
    # noahmp_amd/routing.py)
    @staticmethod
    def flow_terrain_block(height, dir, dx, dy):
        """A noahmp_flow_terrain block over the (nj, ni) WINDOW plane height (float32, device): dir = the uint8 destination plane of the
        same shape.  The tensors are kept alive by the returned block."""
        import torch
        assert height.dim() == 2 and height.is_contiguous() and height.dtype == torch.float32
        assert dir.dtype == torch.uint8 and dir.is_contiguous() and dir.numel() == height.numel()
        b = abi.FlowTerrain()
        b.height, b.dir = height.data_ptr(), dir.data_ptr()
        b.nj, b.ni = (int(v) for v in height.shape)
        b.dx, b.dy = float(dx), float(dy)
        b._keep = (height, dir)
        return b

    def flow_terrain(self, block, stream=None):
        """The direction of steepest strict descent (0 or k = 1..8) of every cell of a block of Engine.flow_terrain_block.  One kernel
        launch, enqueued only, once per terrain (noahmp_hip_flow_terrain)."""
        self._call("noahmp_hip_flow_terrain", C.byref(block), stream)

    def flow_inmask(self, dir, inmask, stream=None):
        """The byte of upstream neighbours of every cell of the (nj, ni) uint8 device plane dir, into the uint8 plane inmask.  One kernel
        launch, enqueued only (noahmp_hip_flow_inmask)."""
        import torch
        assert dir.dim() == 2 and dir.dtype == torch.uint8 and inmask.dtype == torch.uint8 and dir.is_contiguous() and inmask.is_contiguous()
        assert inmask.numel() == dir.numel()
        nj, ni = (int(v) for v in dir.shape)
        self._call("noahmp_hip_flow_inmask", dir.data_ptr(), inmask.data_ptr(), ni, nj, stream)

    def flow_accumulate(self, inmask, acc_old, acc_new, changed, stream=None):
        """One Jacobi pass of the upstream cell count over the (nj, ni) uint8 device plane inmask: acc_old -> acc_new (int32 tensors holding
        uint32 words), changed = a device word that receives 1 when a cell changed.  One kernel launch, enqueued only
        (noahmp_hip_flow_accumulate)."""
        import torch
        assert inmask.dim() == 2 and inmask.dtype == torch.uint8 and inmask.is_contiguous()
        assert all(t.dtype == torch.int32 and t.is_contiguous() and t.numel() == inmask.numel() for t in (acc_old, acc_new))
        assert changed.dtype == torch.int32 and changed.numel() >= 1
        nj, ni = (int(v) for v in inmask.shape)
        self._call("noahmp_hip_flow_accumulate", inmask.data_ptr(), acc_old.data_ptr(), acc_new.data_ptr(), changed.data_ptr(), ni, nj, stream)

    @staticmethod
    def route_block(inmask, col_index, area, release, storage, out_old, out_new, runoff_a, runoff_b, scale):
        """A noahmp_route block over the (nj, ni) WINDOW: inmask uint8, col_index int32, the others float32 device planes of the window;
        runoff_a / runoff_b (or None) in the column order of the store.  The tensors are kept alive by the returned block."""
        import torch
        assert inmask.dim() == 2 and inmask.dtype == torch.uint8 and col_index.dtype == torch.int32
        keep = dict(inmask=inmask, col_index=col_index, area=area, release=release, storage=storage, out_old=out_old, out_new=out_new,
                    runoff_a=runoff_a, runoff_b=runoff_b)
        b = abi.Route()
        for name, t in keep.items():
            if t is not None:
                assert t.is_contiguous() and (name.startswith("runoff") or t.numel() == inmask.numel()), name
                assert name in ("inmask", "col_index") or t.dtype == torch.float32, name
        _fill(b, keep)
        b.nj, b.ni = (int(v) for v in inmask.shape)
        b.scale = float(scale)
        return b

    def route_runoff(self, block, ncol, stream=None):
        """One routing step of a block of Engine.route_block: every owned cell gathers what its upstream neighbours released in the call
        before, adds its column's runoff and releases its fraction.  One kernel launch, enqueued only (noahmp_hip_route_runoff)."""
        self._call("noahmp_hip_route_runoff", C.byref(block), int(ncol), stream)

    # ---- depression filling and flat resolution for the D8 network (noahmp_flow_fill.hip; helper: noahmp_amd/routing.py DepressionFill)
    @staticmethod
    def flow_fill_block(height, fixed, w_old, w_new, changed, eps, sweeps=1, flags=0, outlet=None):
        """A noahmp_flow_fill block over the (nj, ni) WINDOW plane height (float32, device): fixed (and outlet, or None) uint8, w_old and
        w_new float32 planes of the same shape, changed an int32 device word.  flags: NOAHMP_FILL_* bits (abi.FILL_FLAG).  The tensors
        are kept alive by the returned block."""
        import torch
        assert height.dim() == 2 and height.is_contiguous() and height.dtype == torch.float32
        for t, dt in ((fixed, torch.uint8), (w_old, torch.float32), (w_new, torch.float32)) + (((outlet, torch.uint8),) if outlet is not None else ()):
            assert t.dtype == dt and t.is_contiguous() and t.numel() == height.numel()
        assert changed.dtype == torch.int32 and changed.numel() >= 1
        b = abi.FlowFill()
        b.height, b.fixed, b.w_old, b.w_new, b.changed = (t.data_ptr() for t in (height, fixed, w_old, w_new, changed))
        b.outlet = outlet.data_ptr() if outlet is not None else None
        b.nj, b.ni = (int(v) for v in height.shape)
        b.eps, b.sweeps, b.flags = float(eps), int(sweeps), int(flags)
        b._keep = (height, fixed, w_old, w_new, changed, outlet)
        return b

    def flow_fill_init(self, block, stream=None):
        """fixed and w_old of a block of Engine.flow_fill_block: outlets at their height, every other cell at +inf.  One kernel launch,
        enqueued only (noahmp_hip_flow_fill_init)."""
        self._call("noahmp_hip_flow_fill_init", C.byref(block), stream)

    def flow_fill(self, block, stream=None):
        """One call of the relaxation w_old -> w_new of a block of Engine.flow_fill_block: the pinned Jacobi pass (sweeps == 1) or the
        tiled LDS kernel; the block's changed word receives 1 when a word differs.  One kernel launch, enqueued only
        (noahmp_hip_flow_fill)."""
        self._call("noahmp_hip_flow_fill", C.byref(block), stream)

    # ---- watershed delineation on the D8 network (noahmp_basins.hip; helper: noahmp_amd/routing.py Basins)
    @staticmethod
    def flow_basin_block(dir, state_old, state_new, label, dist, changed, flags=0, seed=None, sweeps=1):
        """A noahmp_flow_basin block over the (nj, ni) WINDOW plane dir (uint8, device): state_old and state_new int64 planes (one packed
        {int32 ptr, int32 hops} word per cell), label, dist (and seed, or None) int32 planes of the same shape, changed an int32 device
        word.  flags: NOAHMP_BASIN_RING_* bits (abi.BASIN_FLAG).  sweeps: 1 = the pinned pass, more = the tiled form of the pass.  The tensors
        are kept alive by the returned block."""
        import torch
        assert dir.dim() == 2 and dir.is_contiguous() and dir.dtype == torch.uint8
        for t, dt in ((state_old, torch.int64), (state_new, torch.int64), (label, torch.int32), (dist, torch.int32)) + (((seed, torch.int32),) if seed is not None else ()):
            assert t.dtype == dt and t.is_contiguous() and t.numel() == dir.numel()
        assert changed.dtype == torch.int32 and changed.numel() >= 1
        b = abi.FlowBasin()
        b.dir, b.state_old, b.state_new, b.label, b.dist, b.changed = (t.data_ptr() for t in (dir, state_old, state_new, label, dist, changed))
        b.seed = seed.data_ptr() if seed is not None else None
        b.nj, b.ni = (int(v) for v in dir.shape)
        b.flags, b.sweeps = int(flags), int(sweeps)
        b._keep = (dir, state_old, state_new, label, dist, changed, seed)
        return b

    def flow_basin_init(self, block, stream=None):
        """state_old, label and dist of a block of Engine.flow_basin_block: every cell points at its downstream cell, roots (gauges, cells
        without a downstream cell, ring cells) at themselves.  One kernel launch, enqueued only (noahmp_hip_flow_basin_init)."""
        self._call("noahmp_hip_flow_basin_init", C.byref(block), stream)

    def flow_basin_jump(self, block, stream=None):
        """One doubling pass state_old -> state_new (the block's sweeps: the pinned pass, or the tiled form that first contracts the paths
        inside every 64 x 32 tile); the block's changed word receives 1 when a pointer moved.  One kernel launch, enqueued only
        (noahmp_hip_flow_basin_jump)."""
        self._call("noahmp_hip_flow_basin_jump", C.byref(block), stream)

    def flow_basin_resolve(self, block, stream=None):
        """label and dist of every cell from its root's, in place, on the converged state_old of the block; changed receives 1 when a
        label changed.  One kernel launch, enqueued only (noahmp_hip_flow_basin_resolve)."""
        self._call("noahmp_hip_flow_basin_resolve", C.byref(block), stream)

    # ---- upstream sums on the D8 network (noahmp_accum.hip; helper: noahmp_amd/routing.py Upstream)
    @staticmethod
    def flow_upstream_block(dir, sum, pend_in, pend_out, jump_old, jump_new, changed, flags=0, weight=None, inflow=None):
        """A noahmp_flow_upstream block over the (nj, ni) WINDOW plane dir (uint8, device): sum, pend_in and pend_out (and inflow, or
        None) int64 planes of the same shape holding uint64 words, jump_old and jump_new (and weight, or None: uint32 words) int32 planes,
        changed an int32 device word.  flags: NOAHMP_UPSTREAM_RING_* bits (abi.UPSTREAM_FLAG).  The tensors are kept alive by the
        returned block."""
        import torch
        assert dir.dim() == 2 and dir.is_contiguous() and dir.dtype == torch.uint8
        planes = ((sum, torch.int64), (pend_in, torch.int64), (pend_out, torch.int64), (jump_old, torch.int32), (jump_new, torch.int32))
        planes += ((weight, torch.int32),) if weight is not None else ()
        planes += ((inflow, torch.int64),) if inflow is not None else ()
        for t, dt in planes:
            assert t.dtype == dt and t.is_contiguous() and t.numel() == dir.numel()
        assert changed.dtype == torch.int32 and changed.numel() >= 1
        b = abi.FlowUpstream()
        b.dir, b.sum, b.pend_in, b.pend_out, b.jump_old, b.jump_new, b.changed = (
            t.data_ptr() for t in (dir, sum, pend_in, pend_out, jump_old, jump_new, changed))
        b.weight = weight.data_ptr() if weight is not None else None
        b.inflow = inflow.data_ptr() if inflow is not None else None
        b.nj, b.ni = (int(v) for v in dir.shape)
        b.flags = int(flags)
        b._keep = (dir, sum, pend_in, pend_out, jump_old, jump_new, changed, weight, inflow)
        return b

    def flow_upstream_init(self, block, stream=None):
        """sum, pend_in, pend_out and jump_old of a block of Engine.flow_upstream_block: every cell holds its weight (a ring cell its
        inflow) and jumps to its downstream cell; edges into ring cells are cut.  One kernel launch, enqueued only
        (noahmp_hip_flow_upstream_init)."""
        self._call("noahmp_hip_flow_upstream_init", C.byref(block), stream)

    def flow_upstream_pass(self, block, stream=None):
        """One doubling pass: every cell folds pend_in into sum, pushes the sum to pend_out at its jump and squares the jump into
        jump_new; the block's changed word receives 1 when a cell pushed.  The caller swaps the jump planes and the pend planes between
        passes.  One kernel launch, enqueued only (noahmp_hip_flow_upstream_pass)."""
        self._call("noahmp_hip_flow_upstream_pass", C.byref(block), stream)

    # ---- kinematic-wave routing with Manning friction on the D8 network (noahmp_channel.hip; helper: noahmp_amd/routing.py ChannelFlow)
    @staticmethod
    def flow_channel_block(dir, manning, length, conv, dx, dy, smin, height=None, slope=None):
        """A noahmp_flow_channel block over the (nj, ni) WINDOW plane dir (uint8, device): manning, length, conv and exactly one of
        height and slope are float32 planes of the same shape.  The tensors are kept alive by the returned block."""
        import torch
        assert dir.dim() == 2 and dir.is_contiguous() and dir.dtype == torch.uint8
        keep = dict(height=height, slope=slope, dir=dir, manning=manning, length=length, conv=conv)
        for name, t in keep.items():
            if t is not None and name != "dir":
                assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == dir.numel(), name
        b = abi.FlowChannel()
        _fill(b, keep)
        b.nj, b.ni = (int(v) for v in dir.shape)
        b.dx, b.dy, b.smin = float(dx), float(dy), float(smin)
        return b

    def flow_channel(self, block, stream=None):
        """The flow length along its direction and conv = sqrt(max(s, smin)) / n of every cell of a block of Engine.flow_channel_block.
        One kernel launch, enqueued only, once per terrain (noahmp_hip_flow_channel)."""
        self._call("noahmp_hip_flow_channel", C.byref(block), stream)

    @staticmethod
    def route_kinematic_block(inmask, col_index, area, width, length, conv, storage, out_old, out_new, runoff_a, runoff_b, scale, dt,
                              depth=None, diag=None):
        """A noahmp_route_kinematic block over the (nj, ni) WINDOW: inmask uint8, col_index int32, the others float32 device planes of
        the window; runoff_a / runoff_b (or None) in the column order of the store; depth a float32 plane or None; diag an int32 tensor
        of two words or None.  The tensors are kept alive by the returned block."""
        import torch
        assert inmask.dim() == 2 and inmask.dtype == torch.uint8 and col_index.dtype == torch.int32
        keep = dict(inmask=inmask, col_index=col_index, area=area, width=width, length=length, conv=conv, storage=storage, out_old=out_old,
                    out_new=out_new, runoff_a=runoff_a, runoff_b=runoff_b, depth=depth)
        for name, t in keep.items():
            if t is not None:
                assert t.is_contiguous() and (name.startswith("runoff") or t.numel() == inmask.numel()), name
                assert name in ("inmask", "col_index") or t.dtype == torch.float32, name
        if diag is not None:
            assert diag.dtype == torch.int32 and diag.is_contiguous() and diag.numel() >= 2
            keep["diag"] = diag
        b = abi.RouteKinematic()
        _fill(b, keep)
        b.nj, b.ni = (int(v) for v in inmask.shape)
        b.scale, b.dt = float(scale), float(dt)
        return b

    def route_kinematic(self, block, ncol, stream=None):
        """One kinematic-wave step of a block of Engine.route_kinematic_block: every owned cell gathers what its upstream neighbours
        released in the call before, adds its column's runoff and releases Manning's discharge of what it holds, at most all of it.
        One kernel launch, enqueued only (noahmp_hip_route_kinematic)."""
        self._call("noahmp_hip_route_kinematic", C.byref(block), int(ncol), stream)

    # ---- lakes on the D8 network: level-pool storage and outflow (noahmp_lakes.hip; helper: noahmp_amd/routing.py Lakes)
    @staticmethod
    def lake_take_block(member_cell, member_lake, storage, inflow, quantum):
        """A noahmp_lake_take block: member_cell and member_lake int32 device lists of one length (-1: a pad), storage the float32 window
        plane of the routing call, inflow an int64 device tensor of one word per lake.  The tensors are kept alive by the returned block."""
        import torch
        assert member_cell.dtype == torch.int32 and member_lake.dtype == torch.int32 and member_cell.numel() == member_lake.numel()
        assert storage.dtype == torch.float32 and inflow.dtype == torch.int64
        keep = dict(member_cell=member_cell, member_lake=member_lake, storage=storage, inflow=inflow)
        for name, t in keep.items():
            assert t.is_contiguous(), name
        b = abi.LakeTake()
        _fill(b, keep)
        b.nmember, b.nlake, b.ncell, b.quantum = int(member_cell.numel()), int(inflow.numel()), int(storage.numel()), float(quantum)
        return b

    def lake_take(self, block, stream=None):
        """The whole quanta of every listed member's storage leave the cell and are added to its lake's inflow word, an integer sum.
        One kernel launch, enqueued only (noahmp_hip_lake_take)."""
        self._call("noahmp_hip_lake_take", C.byref(block), stream)

    @staticmethod
    def lake_release_block(volume, inflow, params, outlet_cell, out_new, quantum, dt, level=None, outflow=None, diag=None):
        """A noahmp_lake_release block: volume and inflow int64 device words per lake, params a dict of the seven float64 device planes
        (area, weir_h, weir_c, weir_l, orifice_h, orifice_c, orifice_a), outlet_cell int32 per lake, out_new the float32 window plane of
        the routing call; level (float64), outflow (float32) per lake and diag (one int32 word) or None.  The tensors are kept alive by
        the returned block."""
        import torch
        nlake = int(volume.numel())
        assert volume.dtype == torch.int64 and inflow.dtype == torch.int64 and inflow.numel() == nlake
        assert outlet_cell.dtype == torch.int32 and outlet_cell.numel() == nlake and out_new.dtype == torch.float32
        keep = dict(volume=volume, inflow=inflow, outlet_cell=outlet_cell, out_new=out_new, level=level, outflow=outflow, diag=diag)
        for name in ("area", "weir_h", "weir_c", "weir_l", "orifice_h", "orifice_c", "orifice_a"):
            t = keep[name] = params[name]
            assert t.dtype == torch.float64 and t.numel() == nlake, name
        assert level is None or (level.dtype == torch.float64 and level.numel() == nlake)
        assert outflow is None or (outflow.dtype == torch.float32 and outflow.numel() == nlake)
        assert diag is None or (diag.dtype == torch.int32 and diag.numel() >= 1)
        for name, t in keep.items():
            assert t is None or t.is_contiguous(), name
        b = abi.LakeRelease()
        _fill(b, keep)
        b.nlake, b.ncell, b.quantum, b.dt = nlake, int(out_new.numel()), float(quantum), float(dt)
        return b

    def lake_release(self, block, stream=None):
        """volume += inflow, inflow = 0, the level-pool outflow of every lake (weir + orifice, at most what it holds) leaves volume and is
        written to out_new at the outlet.  One kernel launch, enqueued only (noahmp_hip_lake_release)."""
        self._call("noahmp_hip_lake_release", C.byref(block), stream)

    @staticmethod
    def lake_depth_block(member_cell, member_lake, volume, area, datum, bed, depth, quantum):
        """A noahmp_lake_depth block: the member lists of the take, volume int64 and area, datum float64 device words per lake, bed and
        depth float32 window planes (depth: the depth_new of the diffusive routing call).  The tensors are kept alive by the block."""
        import torch
        nlake = int(volume.numel())
        assert member_cell.dtype == torch.int32 and member_lake.dtype == torch.int32 and member_cell.numel() == member_lake.numel()
        assert volume.dtype == torch.int64 and area.dtype == torch.float64 and datum.dtype == torch.float64
        assert area.numel() == nlake and datum.numel() == nlake
        assert bed.dtype == torch.float32 and depth.dtype == torch.float32 and bed.numel() == depth.numel()
        keep = dict(member_cell=member_cell, member_lake=member_lake, volume=volume, area=area, datum=datum, bed=bed, depth=depth)
        for name, t in keep.items():
            assert t.is_contiguous(), name
        b = abi.LakeDepth()
        _fill(b, keep)
        b.nmember, b.nlake, b.ncell, b.quantum = int(member_cell.numel()), nlake, int(depth.numel()), float(quantum)
        return b

    def lake_depth(self, block, stream=None):
        """After lake_release: every listed member's depth becomes the lake's surface (datum + volume*quantum/area) above the member's
        bed, 0 where the bed is higher.  One kernel launch, enqueued only (noahmp_hip_lake_depth)."""
        self._call("noahmp_hip_lake_depth", C.byref(block), stream)

    # ---- diffusive-wave routing on the D8 network: backwater (noahmp_diffusive.hip; helper: noahmp_amd/routing.py DiffusiveFlow)
    @staticmethod
    def flow_drop_block(dir, drop, dx, dy, height=None, slope=None):
        """A noahmp_flow_drop block over the (nj, ni) WINDOW plane dir (uint8, device): drop and exactly one of height and slope are
        float32 planes of the same shape.  The tensors are kept alive by the returned block."""
        import torch
        assert dir.dim() == 2 and dir.is_contiguous() and dir.dtype == torch.uint8
        keep = dict(height=height, slope=slope, dir=dir, drop=drop)
        for name, t in keep.items():
            if t is not None and name != "dir":
                assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == dir.numel(), name
        b = abi.FlowDrop()
        _fill(b, keep)
        b.nj, b.ni = (int(v) for v in dir.shape)
        b.dx, b.dy = float(dx), float(dy)
        return b

    def flow_drop(self, block, stream=None):
        """The bed drop of every cell of a block of Engine.flow_drop_block to its downstream cell.  One kernel launch, enqueued only,
        once per terrain (noahmp_hip_flow_drop)."""
        self._call("noahmp_hip_flow_drop", C.byref(block), stream)

    @staticmethod
    def route_diffusive_block(inmask, col_index, dir, area, width, length, conv, manning, drop, storage, out_old, out_new, runoff_a, runoff_b,
                              depth_old, depth_new, scale, dt, limit=0.5, diag=None):
        """A noahmp_route_diffusive block over the (nj, ni) WINDOW: inmask and dir uint8, col_index int32, the others float32 device
        planes of the window; runoff_a / runoff_b (or None) in the column order of the store; diag an int32 tensor of four words or
        None.  The tensors are kept alive by the returned block."""
        import torch
        assert inmask.dim() == 2 and inmask.dtype == torch.uint8 and dir.dtype == torch.uint8 and col_index.dtype == torch.int32
        keep = dict(inmask=inmask, col_index=col_index, dir=dir, area=area, width=width, length=length, conv=conv, manning=manning, drop=drop,
                    storage=storage, out_old=out_old, out_new=out_new, runoff_a=runoff_a, runoff_b=runoff_b, depth_old=depth_old,
                    depth_new=depth_new)
        for name, t in keep.items():
            if t is not None:
                assert t.is_contiguous() and (name.startswith("runoff") or t.numel() == inmask.numel()), name
                assert name in ("inmask", "col_index", "dir") or t.dtype == torch.float32, name
        if diag is not None:
            assert diag.dtype == torch.int32 and diag.is_contiguous() and diag.numel() >= 4
            keep["diag"] = diag
        b = abi.RouteDiffusive()
        _fill(b, keep)
        b.nj, b.ni = (int(v) for v in inmask.shape)
        b.scale, b.dt, b.limit = float(scale), float(dt), float(limit)
        return b

    def route_diffusive(self, block, ncol, stream=None):
        """One diffusive-wave step of a block of Engine.route_diffusive_block: the gather and input of route_kinematic, then Manning's
        discharge at the slope of the water surface to the downstream cell, nothing where that surface is not lower, at most `limit`
        times the levelling volume.  One kernel launch, enqueued only (noahmp_hip_route_diffusive)."""
        self._call("noahmp_hip_route_diffusive", C.byref(block), int(ncol), stream)

    def groundwater_init(self, store, stream=None):
        """GROUNDWATER_INIT + EQSMOISTURE (reference drv:1286-1522): equilibrium soil moisture, deep-layer moisture
        and water-table adjustment for OPT_RUN=5, in place.  ide+1 / jde+1 as NOAHMP_INIT receives them (hdrv:291)."""
        w = store.wtable_args()
        w.ide += 1
        w.jde += 1
        mem = abi.MEM_DEVICE if isinstance(store, DeviceColumnStore) else abi.MEM_HOST
        st = abi.Status()
        rc = self.lib.noahmp_hip_groundwater_init(C.byref(w), store.cfg.iswater, mem, stream, C.byref(st))
        self.last_status = st
        if rc:
            raise RuntimeError("noahmp_hip_groundwater_init: rc=%d %s" % (rc, self.lib.noahmp_hip_last_error().decode()))
        return st

    # ---- asynchronous stepping (device-resident state only)
    def noahmplsm_async(self, args, stream=None):
        """Enqueue one step described by a prepared StepArgs block (store.step_args(...), device pointers)."""
        self._apply_ranges(getattr(args, "_ranges", None))
        self._call("noahmp_hip_step_async", C.byref(args), stream)

    def sync(self, check=True):
        """Wait for the pending asynchronous steps; returns (Status, ordinal of the failing step or -1)."""
        st = abi.Status()
        step = C.c_int(-1)
        rc = self.lib.noahmp_hip_sync(C.byref(st), C.byref(step))
        self.last_status = st
        if rc < 0:
            raise RuntimeError("noahmp_hip_sync: " + self.lib.noahmp_hip_last_error().decode())
        if rc > 0 and check:
            raise NoahMPFatal(rc, st.i, st.j, "step +%d: %s" % (step.value, self.lib.noahmp_hip_error_string(rc).decode()))
        return st, step.value

    def sync_timing(self):
        """(land-or-mixed, land-ice, skipped) kernel ms summed over the steps of the last sync(), and their number."""
        out = (C.c_float * 3)()
        n = self.lib.noahmp_hip_sync_timing(out, 3)
        return [float(x) for x in out], n

    def sync_counts(self):
        """(land, land-ice, skipped) columns summed over the steps of the last sync(), as 64-bit integers (Status carries int32)."""
        out = (C.c_int64 * 3)()
        self.lib.noahmp_hip_sync_counts(out, 3)
        return int(out[0]), int(out[1]), int(out[2])

    def sync_step_timing(self):
        """Land (or mixed) kernel ms of every step of the last sync(), in step order."""
        n = self.lib.noahmp_hip_sync_step_timing(None, 0)
        out = (C.c_float * max(n, 1))()
        self.lib.noahmp_hip_sync_step_timing(out, n)
        return [float(out[i]) for i in range(n)]

    def jit_cache_info(self):
        """(cache directory, option sets compiled by this process, loaded from the disk cache, fallen back to the generic kernel)."""
        c = (C.c_int32 * 3)()
        d = self.lib.noahmp_hip_jit_cache_info(c)
        return (d.decode() if d else ""), int(c[0]), int(c[1]), int(c[2])

    def finalize(self):
        self.lib.noahmp_hip_finalize()
