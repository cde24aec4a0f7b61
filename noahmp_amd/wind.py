"""Wind of a device-resident run on complex terrain: the MicroMet wind model (Liston and Elder 2006, J. Hydrometeorol. 7, 217-234, section
2e) on the forcing records (noahmp_hip_wind_terrain / noahmp_hip_forcing_wind).

    wt = WindTerrain(engine, ni, nj)                               # the tile of the store
    wt.set_terrain(height, dx, dy, ncurv=3, origin=(i0, j0))       # once: height is a WINDOW = tile + margin of max(1, ncurv) cells
    wt.follow(store)                                               # after Engine.sort_store: the three planes go into the store's order
    wt.record(rec_a); wt.record(rec_b)                             # per record: rec["u"], rec["v"] adjusted IN PLACE, one launch each
    engine.forcing_interpolate_prep(store, rec_a, rec_b, ...)      # unchanged: it interpolates the adjusted records

The speed of a column is weighted by the terrain slope in the direction of the wind and by the terrain curvature, W' = W (1 + 0.58 Os +
0.42 Oc), and the direction is turned around the obstacle; flat terrain changes no bit.  Not represented: a mass-consistent flow solver,
any dependence on stability, any dependence of the speed on elevation.  The contract -- every rounding -- is the text in
include/noahmp_hip.h.
"""
import math

from .tile import permute_planes, sorted_perm, window_index


class WindTerrain:
    def __init__(self, engine, ni, nj, gamma_s=0.58, gamma_c=0.42):
        import torch
        self.engine, self.torch = engine, torch
        self.ni, self.nj = int(ni), int(nj)
        self.ncell = self.ni * self.nj
        self.gamma_s, self.gamma_c = float(gamma_s), float(gamma_c)
        self.planes_tile = self.planes = None                        # (sx, sy, curv) in tile order / the column order the records are in
        self.slope_max = self.curv_max = None
        self.perm = None

    def set_terrain(self, height, dx, dy, ncurv=3, origin=(0, 0), cosalpha=None, sinalpha=None, slope_max=None, curv_max=None):
        """height: the terrain height [m] of an (nj_w, ni_w) WINDOW that contains the tile with its cell (0, 0) at window cell origin =
        (i0, j0); a margin of max(1, ncurv) cells on every side that is not an edge of the whole domain gives the bits of the undecomposed
        run.  dx, dy: grid spacing [m]; ncurv: the curvature length in cells (about half the distance from ridge to valley); cosalpha /
        sinalpha: WRF's rotation planes over the window, or None (grid y is true north; the wind is then taken in grid coordinates).
        The terrain is scanned ONCE, here, into three tile-order planes (slope vector east / north, curvature) that are kept; follow()
        permutes them.  slope_max defaults to the maximum of sqrt(sx^2 + sy^2) and curv_max to the maximum of |curv| over the WINDOW
        (one more launch over every window cell and two torch reductions, made once; a maximum of zero -- flat terrain, where no column
        is changed -- becomes 1).  A DECOMPOSED RUN MUST PASS THE GLOBAL VALUES, the same numbers on every rank, or the ranks scale the
        same slope differently.  Works before or after follow()."""
        torch = self.torch
        assert height.dim() == 2 and (cosalpha is None) == (sinalpha is None)
        dev = height.device
        index = window_index(height.shape, origin, self.ni, self.nj, device=dev)
        h = height.to(torch.float32).contiguous()
        rot = (None, None)
        if cosalpha is not None:
            rot = tuple(t.to(torch.float32).contiguous() for t in (cosalpha, sinalpha))
            assert all(t.shape == h.shape for t in rot)
        tile = tuple(torch.empty((self.nj, self.ni), dtype=torch.float32, device=dev) for _ in range(3))
        need_max = slope_max is None or curv_max is None
        win = tuple(torch.empty_like(h) for _ in range(3)) if need_max else None
        torch.cuda.current_stream().synchronize()
        self.engine.wind_terrain(self.engine.wind_terrain_block(h, *tile, dx, dy, ncurv=ncurv, cosalpha=rot[0], sinalpha=rot[1], dst_index=index),
                                 self.ncell)
        if need_max:
            self.engine.wind_terrain(self.engine.wind_terrain_block(h, *win, dx, dy, ncurv=ncurv, cosalpha=rot[0], sinalpha=rot[1]), h.numel())
        self.engine.stream_sync()
        if slope_max is None:
            slope_max = float(torch.sqrt(win[0] * win[0] + win[1] * win[1]).max().item()) or 1.0
        if curv_max is None:
            curv_max = float(win[2].abs().max().item()) or 1.0
        if not (math.isfinite(slope_max) and slope_max > 0 and math.isfinite(curv_max) and curv_max > 0):
            raise ValueError("slope_max %r / curv_max %r: the terrain holds NaN or Inf; pass both maxima" % (slope_max, curv_max))
        self.slope_max, self.curv_max = float(slope_max), float(curv_max)
        self.planes_tile = self.planes = tile
        if self.perm is not None:
            self._permute()

    def _permute(self):
        self.planes = tuple(permute_planes(self.engine, self.planes_tile, self.perm, self.ni, self.nj))

    def follow(self, store):
        """After Engine.sort_store(store): the three planes, permuted into the store's column order with noahmp_hip_gather_fields.  Waits for
        the engine's stream."""
        self.perm = sorted_perm(store, self.ni, self.nj)
        if self.planes_tile is not None:
            self._permute()

    def record(self, rec, turn=True, stream=None):
        """rec["u"] and rec["v"] (float32 device planes of the tile's columns, in the column order the planes are in) adjusted IN PLACE: one
        launch, enqueued only.  Call it once per record, before the record goes into forcing_interpolate[_prep]; a record adjusted twice
        is adjusted twice."""
        if self.planes is None:
            raise ValueError("call set_terrain() first")
        u, v = rec["u"], rec["v"]
        assert u.dtype == self.torch.float32 and v.dtype == self.torch.float32 and u.is_contiguous() and v.is_contiguous()
        assert u.numel() == self.ncell and v.numel() == self.ncell
        sx, sy, curv = self.planes
        block = self.engine.wind_block(u, v, sx, sy, curv, self.slope_max, self.curv_max, gamma_s=self.gamma_s, gamma_c=self.gamma_c, turn=turn)
        self.engine.forcing_wind(block, self.ncell, stream=stream)
