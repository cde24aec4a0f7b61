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
        torch = self.torch
        inv = torch.empty_like(perm)
        inv[perm.long()] = torch.arange(perm.numel(), dtype=perm.dtype, device=perm.device)
        return inv

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
        torch = self.torch
        if store is not None:
            self.store = store
        new = getattr(self.store, "sort_perm", None)
        assert new is not None, "follow() is for a store that Engine.sort_store has sorted"
        g = new if self.perm is None else self._inverse(self.perm)[new.long()].contiguous()   # new position p <- old position g[p]
        torch.cuda.current_stream().synchronize()
        old = [it[4] for it in self.items] + [self.count]
        fresh = [torch.empty_like(t) for t in old]
        torch.cuda.current_stream().synchronize()
        self.engine.stream_sync()
        for i in range(0, len(old), 32):
            self.engine.gather(fresh[i:i + 32], old[i:i + 32], g, self.store.ni, self.store.nj)()
        self.engine.stream_sync()
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
