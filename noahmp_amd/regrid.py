"""Forcing records on their own coarse grid -> the model grid's planes, on the device (noahmp_hip_forcing_regrid).

    src = Engine.regrid_source(nx, ny, lon0, lat0, dlon, dlat, periodic_x=False)
    rg = ForcingRegrid(engine, xlat, xlon, src, valid=None, search_radius=4)      # builds the plan; rg.unfilled
    rg.set_adjust("t", z_model - rg.regrid_plane(z_source), scale=-0.0065)       # optional: lapse-rate correction of one plane, or
    rg.set_elevation(z_model, z_source, lapse=-0.0065)                           # optional: t, p, q, lw moved to the model's terrain height
    rg.set_conserve(area=cell_area)                                              # optional: budget-preserving regrid of fluxes; rg.clipped
    rg.set_pattern("pcp", prism_ratio)                                           # optional: a fine climatology pattern of one conserve plane
    rec = rg.record({"t": t_c, "q": q_c, ..., "pcp": p_c}, modes={"pcp": "conserve"})      # or "nearest" / "bilinear"
    rg.follow(store)          # after Engine.sort_store: plan and adjust planes go into the store's column order

``record()`` returns what ``Engine.forcing_interpolate[_prep]`` takes as ``rec_a`` / ``rec_b``: a dict of (nj, ni) device planes.  Two
sets of output planes are used alternately, so a bracketing pair of records stays alive.  The coarse planes are device tensors of the
source grid's shape (ny, nx): uploading them is the caller's (they are 50-150 times smaller than what is made of them).

The contract -- every rounding of the plan and of the value -- is the text in include/noahmp_hip.h.  Each rank plans its own tile
against the one global source.
"""


from .tile import inverse_perm, permute_planes, sorted_perm, to_tile_order, window_index


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
        self.valid, self.search_radius = valid, search_radius
        self.conserve = None                     # set_conserve: the Engine.RegridConservePlan of the window
        self.clipped = 0                         # groups the window cuts (set_conserve); > 0: widen the margin
        self.window = None                       # set_conserve: ((nj_w, ni_w), (i0, j0)) of the window
        self.window_tile = self.dst_index = None # per window cell: its tile index or -1 / its position in the current column order or -1
        self.patterns = {}                       # name -> plane in window order

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
        return to_tile_order(self.engine, plane, self.perm, self.ni, self.nj)

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

    def set_conserve(self, area=None, window=None, domain_edges=0b1111):
        """From now on record() serves the names whose mode is "conserve" with noahmp_hip_forcing_regrid_conserve: bilinear, optionally
        shaped by a pattern, rescaled so that the area-weighted mean over the model cells of each source cell is the source cell's value.
        area: float32 device plane of the window's shape in WINDOW order (TILE order without a window), or None = 1.  window =
        (xlat_w, xlon_w, i0, j0): a wider rectangle of model cells that holds the tile at column i0, row j0 -- the margin of a
        decomposed run, wide enough to hold every model cell of every source cell that owns a tile cell; None: the tile itself.
        domain_edges: NOAHMP_REGRID_EDGE_* bits of the window's sides that are edges of the whole model domain.  Sets rg.clipped: the
        number of source cells that own a tile cell and reach a side of the window that is no domain edge; > 0: widen the margin.  Waits."""
        torch = self.torch
        if window is None:
            plan_w, nj_w, ni_w, i0, j0 = self.plan_tile, self.nj, self.ni, 0, 0
        else:
            xlat_w, xlon_w, i0, j0 = window
            nj_w, ni_w = xlat_w.shape
            assert 0 <= i0 and i0 + self.ni <= ni_w and 0 <= j0 and j0 + self.nj <= nj_w, "the window must hold the tile"
            plan_w, _ = self.engine.regrid_plan(xlat_w.contiguous(), xlon_w.contiguous(), self.source, valid=self.valid, search_radius=self.search_radius)
        self.window = ((nj_w, ni_w), (i0, j0))
        self.window_tile = window_index(*self.window, self.ni, self.nj, device=self.device)
        if area is not None:
            area = area.to(torch.float32).contiguous()
            assert area.numel() == nj_w * ni_w, "area has the window's shape"
        self._refresh_dst_index()
        torch.cuda.current_stream().synchronize()
        self.conserve = self.engine.regrid_conserve_plan(plan_w, ni_w, nj_w, self.source, area=area, dst_index=self.dst_index, domain_edges=domain_edges)
        self.clipped = self.conserve.clipped
        self.patterns = {}

    def _refresh_dst_index(self):
        """dst_index of the window cells for the current column order: only this changes after a re-sort."""
        if self.perm is None:
            self.dst_index = self.window_tile
        else:
            self.dst_index = window_index(*self.window, self.ni, self.nj, pos=inverse_perm(self.perm), device=self.device)

    def set_pattern(self, name, plane):
        """Conserve plane `name` is shaped by `plane` before it is rescaled (a fine climatology, PRISM-style): a float32 device plane of
        the window's shape in WINDOW order; None removes it."""
        torch = self.torch
        assert self.conserve is not None, "set_pattern follows set_conserve"
        if plane is None:
            self.patterns.pop(name, None)
            return
        plane = plane.to(torch.float32).contiguous()
        assert plane.numel() == self.conserve.ni * self.conserve.nj, "a pattern has the window's shape"
        self.patterns[name] = plane
        torch.cuda.current_stream().synchronize()

    def record(self, planes, modes=None, stream=None):
        """{name: coarse device plane} -> {name: (nj, ni) device plane} in ONE launch, enqueued only on the engine's stream (or
        `stream`); modes: {name: "bilinear" | "nearest" | "conserve"}, default bilinear.  The names in mode "conserve" (after
        set_conserve) go through noahmp_hip_forcing_regrid_conserve, at most four more launches per eight names; everything else through
        the one launch, unchanged.  The coarse planes must be complete on the device before the call (the engine's stream does not wait
        for torch's)."""
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
        entries, conserve = [], []
        for name, src in planes.items():
            if src is None:
                continue
            self._check_source_plane(src, name)
            if name not in out:
                out[name] = torch.empty((self.nj, self.ni), dtype=torch.float32, device=self.device)
                fresh = True
            if name in met_names:
                continue
            if modes.get(name) == "conserve":
                if self.conserve is None:
                    raise ValueError("mode 'conserve' (%s) needs set_conserve first" % name)
                if name in self.adjust:
                    raise ValueError("%s: a conserve plane takes no adjust" % name)
                conserve.append((src, out[name], self.patterns.get(name), self.fill))
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
        for i in range(0, len(conserve), 8):
            self.engine.forcing_regrid_conserve(self.conserve, conserve[i:i + 8], dst_index=self.dst_index, stream=stream)
        return {name: out[name] for name, src in planes.items() if src is not None}

    def follow(self, store):
        """After Engine.sort_store(store): the six plan planes, the adjust planes and dz, permuted into the store's column order with
        noahmp_hip_gather_fields; the conserve plan keeps its window order and only dst_index is made anew.  Waits for the engine's stream.
        Records made before the call keep the old order."""
        torch = self.torch
        perm = sorted_perm(store, self.ni, self.nj)
        n = self.ncell
        new = torch.empty_like(self.plan_tile)
        names = list(self.adjust_tile)
        fresh = [torch.empty_like(self.adjust_tile[k][0]) for k in names]
        new_dz = torch.empty_like(self.dz_tile) if self.dz_tile is not None else None
        dst = [new[k * n:(k + 1) * n] for k in range(6)] + fresh
        src = [self.plan_tile[k * n:(k + 1) * n] for k in range(6)] + [self.adjust_tile[k][0] for k in names]
        if new_dz is not None:
            dst.append(new_dz)
            src.append(self.dz_tile)
        permute_planes(self.engine, src, perm, self.ni, self.nj, out=dst)
        self.plan, self.perm = new, perm
        self.adjust = {k: (t, self.adjust_tile[k][1]) for k, t in zip(names, fresh)}
        self.dz = new_dz
        self.sets = [{}, {}]
        if self.conserve is not None:            # the conserve plan stays as it is: only the positions of the window cells change
            self._refresh_dst_index()
            torch.cuda.current_stream().synchronize()
