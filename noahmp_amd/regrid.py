"""Forcing records on their own coarse grid -> the model grid's planes, on the device (noahmp_hip_forcing_regrid).

    src = Engine.regrid_source(nx, ny, lon0, lat0, dlon, dlat, periodic_x=False)
    rg = ForcingRegrid(engine, xlat, xlon, src, valid=None, search_radius=4)      # builds the plan; rg.unfilled
    rg.set_adjust("t", z_model - rg.regrid_plane(z_source), scale=-0.0065)       # optional: lapse-rate correction of one plane, or
    rg.set_elevation(z_model, z_source, lapse=-0.0065)                           # optional: t, p, q, lw moved to the model's terrain height
    rec = rg.record({"t": t_c, "q": q_c, ..., "pcp": p_c}, modes={"pcp": "nearest"})
    rg.follow(store)          # after Engine.sort_store: plan and adjust planes go into the store's column order

``record()`` returns what ``Engine.forcing_interpolate[_prep]`` takes as ``rec_a`` / ``rec_b``: a dict of (nj, ni) device planes.  Two
sets of output planes are used alternately, so a bracketing pair of records stays alive.  The coarse planes are device tensors of the
source grid's shape (ny, nx): uploading them is the caller's (they are 50-150 times smaller than what is made of them).

The contract -- every rounding of the plan and of the value -- is the text in include/noahmp_hip.h.  Each rank plans its own tile
against the one global source.
"""


class ForcingRegrid:
    def __init__(self, engine, xlat, xlon, source, valid=None, search_radius=4, fill=float("nan")):
        import torch
        self.engine, self.torch, self.source = engine, torch, source
        self.nj, self.ni = xlat.shape
        self.ncell = self.ni * self.nj
        self.device = xlat.device
        self.fill = float(fill)
        self.plan_tile, self.unfilled = engine.regrid_plan(xlat.contiguous(), xlon.contiguous(), source, valid=valid, search_radius=search_radius)
        self.plan = self.plan_tile               # the plan in the column order the records are made in
        self.perm = None                         # position p of that order holds tile column perm[p]; None: tile order
        self.adjust_tile, self.adjust = {}, {}   # name -> (plane, scale)
        self.sets = [{}, {}]                     # two sets of output planes, used alternately
        self.turn = 0
        self.dz_tile = self.dz = None            # set_elevation: model height - regridded source height, tile order / current order
        self.lapse = 0.0

    def _check_source_plane(self, t, name):
        assert t.dtype == self.torch.float32 and t.is_contiguous() and t.numel() == self.source.nx * self.source.ny, \
            "%s: a contiguous float32 device plane of the source grid (%d x %d) is required" % (name, self.source.ny, self.source.nx)

    def regrid_plane(self, plane, mode="bilinear", out=None):
        """One source plane in the current column order, without adjustment (e.g. the source's terrain height).  Waits."""
        torch = self.torch
        self._check_source_plane(plane, "regrid_plane")
        if out is None:
            out = torch.empty((self.nj, self.ni), dtype=torch.float32, device=self.device)
        torch.cuda.current_stream().synchronize()
        self.engine.forcing_regrid(self.plan, self.ncell, self.source, [(plane, out, mode, None, 0.0, self.fill)])
        self.engine.stream_sync()
        return out

    def set_adjust(self, name, plane, scale):
        """Records' plane `name` receives + scale * plane: `plane` is an (nj, ni) device tensor in the CURRENT column order (what
        regrid_plane returns), e.g. model height - regridded source height with scale = -0.0065 K/m for the air temperature."""
        torch = self.torch
        if name == "t" and self.dz is not None:
            raise ValueError("set_adjust('t', ...) and set_elevation exclude each other: the met group makes the lapse-rate correction itself")
        plane = plane.to(torch.float32).contiguous()
        assert plane.numel() == self.ncell
        self.adjust[name] = (plane, float(scale))
        self.adjust_tile[name] = (self._tile_order(plane), float(scale))
        torch.cuda.current_stream().synchronize()      # the plane is complete before a record() reads it on the engine's stream

    def _tile_order(self, plane):
        """A tile-order copy of a plane in the current column order: follow() always starts from tile order."""
        torch = self.torch
        if self.perm is None:
            return plane
        inv = torch.empty_like(self.perm)
        inv[self.perm.long()] = torch.arange(self.ncell, dtype=torch.int32, device=self.device)
        tile = torch.empty_like(plane)
        torch.cuda.current_stream().synchronize()
        self.engine.gather([tile], [plane], inv, self.ni, self.nj)()
        self.engine.stream_sync()
        return tile

    MET_NAMES = ("t", "p", "q", "lw")

    def set_elevation(self, z_model, z_source, lapse=-0.0065):
        """From now on record() moves t, p, q and, if the record has it, lw from the source's terrain height to the model's
        (noahmp_hip_forcing_regrid_met, in the same launch as the other names).  z_model: (nj, ni) device plane of the model's height in the
        CURRENT column order; z_source: the source's height on its own grid.  dz = z_model - regrid_plane(z_source) is made once."""
        torch = self.torch
        if "t" in self.adjust:
            raise ValueError("set_elevation and set_adjust('t', ...) exclude each other: the met group makes the lapse-rate correction itself")
        z_model = z_model.to(torch.float32).contiguous()
        assert z_model.numel() == self.ncell
        self.dz = (z_model.reshape(self.nj, self.ni) - self.regrid_plane(z_source)).contiguous()
        self.dz_tile = self._tile_order(self.dz)
        self.lapse = float(lapse)
        torch.cuda.current_stream().synchronize()      # dz is complete before a record() reads it on the engine's stream

    def record(self, planes, modes=None, stream=None):
        """{name: coarse device plane} -> {name: (nj, ni) device plane} in ONE launch, enqueued only on the engine's stream (or
        `stream`); modes: {name: "bilinear" | "nearest"}, default bilinear.  The coarse planes must be complete on the device before
        the call (the engine's stream does not wait for torch's)."""
        torch = self.torch
        modes = modes or {}
        met_names = ()
        if self.dz is not None:
            missing = [nm for nm in ("t", "p", "q") if planes.get(nm) is None]
            if missing:
                raise ValueError("with set_elevation a record needs t, p and q; missing: %s" % ", ".join(missing))
            met_names = tuple(nm for nm in self.MET_NAMES if planes.get(nm) is not None)
            for nm in met_names:
                if modes.get(nm, "bilinear") != "bilinear":
                    raise ValueError("with set_elevation %s is regridded bilinearly (mode %r asked)" % (nm, modes[nm]))
        out = self.sets[self.turn]
        self.turn ^= 1
        fresh = False
        entries = []
        for name, src in planes.items():
            if src is None:
                continue
            self._check_source_plane(src, name)
            if name not in out:
                out[name] = torch.empty((self.nj, self.ni), dtype=torch.float32, device=self.device)
                fresh = True
            if name in met_names:
                continue
            adj, scale = self.adjust.get(name, (None, 0.0))
            entries.append((src, out[name], modes.get(name, "bilinear"), adj, scale, self.fill))
        if fresh:
            torch.cuda.current_stream().synchronize()
        if met_names:
            met = self.engine.regrid_met(planes["t"], planes["p"], planes["q"], out["t"], out["p"], out["q"], self.dz,
                                         src_lw=planes.get("lw"), dst_lw=out.get("lw") if "lw" in met_names else None,
                                         lapse=self.lapse, fill=self.fill)
            self.engine.forcing_regrid_met(self.plan, self.ncell, self.source, met, entries[:32], stream=stream)
            entries = entries[32:]
        for i in range(0, len(entries), 32):
            self.engine.forcing_regrid(self.plan, self.ncell, self.source, entries[i:i + 32], stream=stream)
        return {name: out[name] for name, src in planes.items() if src is not None}

    def follow(self, store):
        """After Engine.sort_store(store): the six plan planes, the adjust planes and dz, permuted into the store's column order with
        noahmp_hip_gather_fields.  Waits for the engine's stream.  Records made before the call keep the old order."""
        torch = self.torch
        perm = getattr(store, "sort_perm", None)
        assert perm is not None, "follow() is for a store that Engine.sort_store has sorted"
        assert store.ni == self.ni and store.nj == self.nj
        n = self.ncell
        new = torch.empty_like(self.plan_tile)
        names = list(self.adjust_tile)
        fresh = [torch.empty_like(self.adjust_tile[k][0]) for k in names]
        new_dz = torch.empty_like(self.dz_tile) if self.dz_tile is not None else None
        torch.cuda.current_stream().synchronize()
        self.engine.stream_sync()
        dst = [new[k * n:(k + 1) * n] for k in range(6)] + fresh
        src = [self.plan_tile[k * n:(k + 1) * n] for k in range(6)] + [self.adjust_tile[k][0] for k in names]
        if new_dz is not None:
            dst.append(new_dz)
            src.append(self.dz_tile)
        for i in range(0, len(dst), 32):
            self.engine.gather(dst[i:i + 32], src[i:i + 32], perm, self.ni, self.nj)()
        self.engine.stream_sync()
        self.plan, self.perm = new, perm
        self.adjust = {k: (t, self.adjust_tile[k][1]) for k, t in zip(names, fresh)}
        self.dz = new_dz
        self.sets = [{}, {}]
