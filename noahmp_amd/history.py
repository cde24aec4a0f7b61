"""Device-side history of a device-resident run: interval accumulators and point probes (noahmp_hip_history_step / _finish).

A run that lives on the device advances millions of columns in a few milliseconds; bringing whole arrays back every step to
integrate a flux on the host would run it at PCIe speed.  `History` keeps what land-surface output is made of -- fluxes summed over
the output interval, daily minima / maxima, a per-step series at a few cells -- in device planes that take one sample per step in
one kernel launch, and returns finished tile-order planes at the output cadence.

    h = History(engine, store)
    h.add_reference_accumulators()                  # ACCPRCP, ACCECAN, ACCETRAN, ACCEDIR of the WRF_HYDRO build (drv:736-739)
    h.add("hfx_mean", "hfx", "sum", mean=True)
    h.add("t2mv_max", "t2mvxy", "max")
    h.add_probes(tower_cells, ["hfx", "lh", "t2mvxy"], nslot=24)
    for step in ...:
        engine.noahmplsm_async(args); h.step()
        if sort happened: h.follow(store)           # after Engine.sort_store(store)
    planes = h.finish()                             # {name: tile-order device tensor}, water points -1.E33; accumulators start over

The planes are torch tensors (torch is the allocator); the arithmetic runs in the engine's HIP kernels.  All calls are enqueued on the
engine's own stream unless a stream is passed.
"""
import numpy as np

from . import abi
from .restart import UNDEFINED
from .tile import inverse_perm, permute_planes, sorted_perm

HUGE = float(np.finfo(np.float32).max)
_IDENTITY = {"sum": 0.0, "sum_dt": 0.0, "min": HUGE, "max": -HUGE, "last": 0.0}

# name -> (step-block field, op, scaled by DT): the accumulators the reference keeps in its WRF_HYDRO build (drv:736-739).
# ACCPRCP = ACCPRCP + PRCP * DT: the forcing plane RAINBL already IS fl(PRCP * DT) -- the driver computes it (hdrv:343) instead of
# drv:736, the same product with the same single rounding -- so its accumulator is a plain SUM of RAINBL: the same two roundings.
REFERENCE_ACCUMULATORS = {
    "accprcp": ("rainbl", "sum", False),
    "accecan": ("ecanxy", "sum_dt", True),
    "accetran": ("etranxy", "sum_dt", True),
    "accedir": ("edirxy", "sum_dt", True),
}


class History:
    def __init__(self, engine, store):
        import torch
        self.engine, self.store, self.torch = engine, store, torch
        self.items = []                      # [name, field, op, scale, acc tensor, mean]
        self.count = torch.zeros((store.nj, store.ni), dtype=torch.int32, device=store.device)
        self.perm = getattr(store, "sort_perm", None)        # position p of the planes holds tile column perm[p]; None: tile order
        self._entries = None
        self.probe_points = None
        torch.cuda.current_stream().synchronize()

    # ------------------------------------------------------------------ set-up
    def add(self, name, field, op, scale=0.0, init=None, mean=False):
        """An accumulator of store field `field` (a 2-D plane or a layered array).  init: None = the identity of `op`, a number, or a
        tensor in the store's CURRENT column order (e.g. the SFCRUNOFF plane, to continue the reference's own accumulator)."""
        torch = self.torch
        src = self.store.a[field]
        assert src.dtype == torch.float32, "history accumulates float32 fields"
        assert len(self.items) < 32, "at most 32 accumulators per History (one launch)"
        if init is None or np.isscalar(init):
            acc = torch.full_like(src, _IDENTITY[op] if init is None else float(init))
        else:
            acc = init.detach().clone().to(src.device)
            assert acc.shape == src.shape
        self.items.append([name, field, op, float(scale), acc, bool(mean)])
        self._entries = None
        torch.cuda.current_stream().synchronize()
        return acc

    def add_reference_accumulators(self, names=("accprcp", "accecan", "accetran", "accedir")):
        """ACCPRCP / ACCECAN / ACCETRAN / ACCEDIR (drv:736-739), started from zero.  ACCPRCP is SUM of the forcing plane `rainbl`,
        which is fl(PRCP * DT) computed by the driver (hdrv:343) instead of by drv:736: the same two roundings per step."""
        for n in names:
            field, op, scaled = REFERENCE_ACCUMULATORS[n]
            self.add(n, field, op, scale=self.store.cfg.dt if scaled else 0.0, init=0.0)

    def add_probes(self, points, fields, nslot):
        """points: linear TILE indices (j * ni + i) of up to 4096 cells; fields: names of up to 32 2-D planes; a ring of `nslot` steps."""
        torch = self.torch
        self.probe_points = torch.as_tensor(np.asarray(points, dtype=np.int32), device=self.store.device)
        self.probe_fields = list(fields)
        self.ring = torch.zeros((int(nslot), len(fields), len(points)), dtype=torch.float32, device=self.store.device)
        self.slot = 0
        self._read = 0
        self._probe_columns()
        self._entries = None

    def _inverse(self, perm):
        return inverse_perm(perm)

    def _probe_columns(self):
        if self.probe_points is None:
            return
        if self.perm is None:
            self.probe_cols = self.probe_points.clone()
        else:
            self.probe_cols = self._inverse(self.perm)[self.probe_points.long()].contiguous()
        self.torch.cuda.current_stream().synchronize()

    def invalidate(self):
        """The store's planes were replaced (e.g. another forcing working set): look their addresses up again at the next step."""
        self._entries = None

    def _prepare(self):
        eng, st = self.engine, self.store
        self._entries = eng.history_entries([(st.a[f], acc, op, sc) for name, f, op, sc, acc, mean in self.items])
        self._args = st.step_args(1, 2000, 1.0)
        self._probes = None
        if self.probe_points is not None:
            self._probes = eng.history_probes(self.probe_cols, [st.a[f] for f in self.probe_fields], self.ring)

    # ------------------------------------------------------------------ per step
    def step(self, stream=None):
        """After a step of the store: one sample into every accumulator, one ring slot of the probes (one launch, enqueued only)."""
        if self._entries is None:
            self._prepare()
        if self._probes is not None:
            self._probes.slot = self.slot
            self.slot += 1
        self.engine.history_step(self._entries, self._args, probes=self._probes, count=self.count, stream=stream)

    def follow(self, store=None):
        """After Engine.sort_store(store): bring the accumulators, the count and the probe columns into the store's new column order
        (noahmp_hip_gather_fields).  Waits for the engine's stream."""
        if store is not None:
            self.store = store
        new = sorted_perm(self.store, self.store.ni, self.store.nj)
        g = new if self.perm is None else self._inverse(self.perm)[new.long()].contiguous()   # new position p <- old position g[p]
        fresh = permute_planes(self.engine, [it[4] for it in self.items] + [self.count], g, self.store.ni, self.store.nj)
        for it, t in zip(self.items, fresh):
            it[4] = t
        self.count = fresh[-1]
        self.perm = new
        self._probe_columns()
        self._entries = None

    # ------------------------------------------------------------------ output time
    def finish(self, reset=True, fill=None, mask_water=True, stream=None):
        """{name: tile-order device tensor}: the accumulators (means divided by the number of steps that advanced the column; `fill`,
        default undefined_real -1.E20, where none did), water points -1.E33 as in the reference's output files.  reset: accumulators
        return to the identity of their op (LAST keeps its value) and the count to zero -- the next interval starts.  Waits."""
        torch = self.torch
        if self._entries is None:
            self._prepare()
        inv = self._inverse(self.perm) if self.perm is not None else None
        dst = [torch.empty_like(it[4]) for it in self.items]
        torch.cuda.current_stream().synchronize()
        flags = [(abi.HIST_FIN["mean"] if it[5] else 0) | (abi.HIST_FIN["reset"] if reset else 0) for it in self.items]
        self.engine.history_finish(self._entries, dst, flags, self.count, self.store, perm=inv,
                                   fill=float(UNDEFINED) if fill is None else fill, mask_water=mask_water, stream=stream)
        self.engine.stream_sync(stream)
        if reset:
            self.count.zero_()
            torch.cuda.current_stream().synchronize()
        return {it[0]: d for it, d in zip(self.items, dst)}

    def read_probes(self):
        """The records written since the last read (at most the ring's slots), oldest first: numpy [record][field][point].  Waits."""
        self.engine.stream_sync()
        nslot = self.ring.shape[0]
        first = max(self._read, self.slot - nslot)
        ring = self.ring.cpu().numpy()
        out = np.stack([ring[s % nslot] for s in range(first, self.slot)]) if self.slot > first else ring[:0]
        self._read = self.slot
        return out


class Regions:
    """Per-step series of fields of the store over labelled regions -- basins, counties, land-use zones (noahmp_hip_region_step).

        rg = Regions(engine, store, basin_map, nbasin, weight=cell_area, nslot=24)
        rg.add("runoff", "runsfxy")                     # area-weighted sum per basin and step
        rg.add("sm_top", "smois", level=0)
        rg.add("t2_max", "t2mvxy", op="max")
        for step in ...:
            engine.noahmplsm_async(args); rg.step()
            if sort happened: rg.follow(store)          # after Engine.sort_store(store)
        series = rg.read()                              # {name: float64 [steps since the last read][nregion]}
        means = rg.means()                              # the SUM series divided by the series of the summed weights

    region_map: int32 (nj, ni) in TILE order whatever order the store is in (numpy or device tensor), ids 0 .. nregion-1, negative = no
    region; weight: float32 (nj, ni) in tile order or None (= 1).  The result is a function of the tile-order values alone: the same bits in
    tile order, in any sorted layout, before and after a re-sort.  Cells that the step does not advance (open water, sea ice) contribute
    nothing.  A region that spans the tiles of several ranks: each rank returns its own sums and weight sums.  At most 31 series (one more,
    the summed weights, is kept for means()); a ring of `nslot` steps between two read() calls."""

    WEIGHT = "__weight__"

    def __init__(self, engine, store, region_map, nregion, weight=None, nslot=24):
        import torch
        self.engine, self.store, self.torch = engine, store, torch
        dev = store.device
        self.region_map = torch.as_tensor(np.ascontiguousarray(region_map, dtype=np.int32) if isinstance(region_map, np.ndarray) else region_map,
                                          device=dev).to(torch.int32).contiguous()
        self.weight = None if weight is None else torch.as_tensor(
            np.ascontiguousarray(weight, dtype=np.float32) if isinstance(weight, np.ndarray) else weight, device=dev).to(torch.float32).contiguous()
        assert tuple(self.region_map.shape) == (store.nj, store.ni)
        self.nregion, self.nslot = int(nregion), int(nslot)
        self.items = [(self.WEIGHT, None, "sum", None)]          # [name, field, op, level]; entry 0: the summed weights of the cells that took part
        self.slot = self._read = 0
        self.series = self.acc = self._entries = None
        torch.cuda.current_stream().synchronize()
        self.plan = engine.region_plan(self.region_map, self.nregion, self.weight, self._inverse(getattr(store, "sort_perm", None)))

    def _inverse(self, perm):
        """inverse_perm(perm), complete before the engine's stream reads it; None for None."""
        if perm is None:
            return None
        inv = inverse_perm(perm)
        self.torch.cuda.current_stream().synchronize()
        return inv

    def add(self, name, field, op="sum", level=None):
        """A series of store field `field` (a 2-D plane, or level `level` of a layered array); op: "sum" (weighted), "min", "max"."""
        assert self.slot == 0, "add series before the first step"
        assert len(self.items) < 32, "at most 31 series per Regions (one launch)"
        src = self.store.a[field]
        assert src.dtype == self.torch.float32 and (src.dim() == 2 or level is not None)
        self.items.append((name, field, op, level))
        self._entries = None

    def invalidate(self):
        """The store's planes were replaced: look their addresses up again at the next step."""
        self._entries = None

    def _prepare(self):
        torch, st = self.torch, self.store
        n = len(self.items)
        if self.series is None:
            self.series = torch.zeros((self.nslot, n, self.nregion), dtype=torch.float64, device=st.device)
            self.acc = torch.zeros((n, self.nregion), dtype=torch.float64, device=st.device)
            self.reset_acc()
        self._entries = self.engine.region_entries([(st.a[f] if f is not None else None, op, lev) for name, f, op, lev in self.items])
        self._args = st.step_args(1, 2000, 1.0)
        torch.cuda.current_stream().synchronize()

    def reset_acc(self):
        """Start the next interval: the accumulators (`acc`: sums of the series' sums, minima of minima, maxima of maxima) to their identities."""
        for f, (name, field, op, lev) in enumerate(self.items):
            self.acc[f].fill_({"sum": 0.0, "min": HUGE, "max": -HUGE}[op])
        self.torch.cuda.current_stream().synchronize()

    def step(self, stream=None):
        """After a step of the store: one ring slot of every series (enqueued only)."""
        if self._entries is None:
            self._prepare()
        self.engine.region_step(self.plan, self._entries, self._args, self.series, self.slot, acc=self.acc, stream=stream)
        self.slot += 1

    def follow(self, store=None):
        """After Engine.sort_store(store): the members' positions in the store's new column order."""
        if store is not None:
            self.store = store
        perm = sorted_perm(self.store, self.store.ni, self.store.nj)
        self.engine.region_follow(self.plan, self._inverse(perm))
        self.engine.stream_sync()
        self._entries = None

    def read(self):
        """{name: float64 numpy [steps][nregion]}: the steps since the last read (at most the ring's slots), oldest first.  Waits."""
        self.engine.stream_sync()
        first = max(self._read, self.slot - self.nslot)
        n = len(self.items)
        ring = self.series.cpu().numpy() if self.series is not None else np.zeros((self.nslot, n, self.nregion))
        rec = np.stack([ring[s % self.nslot] for s in range(first, self.slot)]) if self.slot > first else ring[:0]
        self._read = self.slot
        self._last = {name: rec[:, f, :].copy() for f, (name, field, op, lev) in enumerate(self.items)}
        return {k: v for k, v in self._last.items() if k != self.WEIGHT}

    def means(self, series=None):
        """The SUM series of the last read() (or of `series`, as read() returned it) divided by the summed weights of the cells that took
        part: area-weighted means, NaN where no cell of the region took part."""
        w = self._last[self.WEIGHT]
        src = series if series is not None else self._last
        out = {}
        with np.errstate(all="ignore"):
            for name, field, op, lev in self.items[1:]:
                if op == "sum" and name in src:
                    out[name] = src[name] / w
        return out
