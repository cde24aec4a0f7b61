"""Downward shortwave of a device-resident run: weighted in time by the cosine of the solar zenith angle, moved to the sloping surface
(noahmp_hip_forcing_cosz_mean / noahmp_hip_forcing_shortwave).

    sw = Shortwave(engine, xlat, xlon, mode="zenith")            # (nj, ni) float32 device planes, degrees, TILE order
    sw.set_terrain(slope, aspect)                                 # optional; or set_normal(e, n, u), or terrain_from_height(z, dx, dy)
    sw.set_shadow(height, dx, dy, nstep=25)                        # optional: cast shadows by a ray march over the terrain (window = tile + margin)
    sw.set_skyview(height, dx, dy, nstep=25, ndir=16)              # optional: sky-view factor by a horizon scan (the same window), once
    sw.follow(store)                                              # after Engine.sort_store: lat, lon and the normals go into the store's order
    mean_a = sw.interval((2000, 171, 18, 0, 0), 10800, 36)        # per record: mean of max(cos zenith, 0) over [a, b), 36 samples
    engine.forcing_interpolate_prep(store, rec_a, rec_b, idts, idts2, rain, lon, iday, ihour, iminute, isecond, ...)
    sw.apply(store, rec_a, rec_b, idts, idts2, (iday, ihour, iminute, isecond))      # per step: overwrites the store's linear SWDOWN

The interpolation calls keep writing the reference's linear SWDOWN (netcdf_io:1369-1403); ``apply`` replaces it.  In mode "zenith" record
a's value holds over [a, b) and is multiplied by cos(zenith now) / its interval mean, which keeps the interval's energy, follows the sun
and writes exact zeros where the sun is down; mode "linear" keeps the reference's bits and only adds the terrain step.  The contract --
every rounding -- is the text in include/noahmp_hip.h.
"""
import math

from .tile import check_window, inverse_perm, permute_planes, sorted_perm, to_tile_order, window_index


def days_in_year(year):
    return 366 if (year % 4 == 0 and (year % 100 != 0 or year % 400 == 0)) else 365


def time_after(start, seconds):
    """(year, iday, ihour, iminute, isecond) + whole seconds -> the same form; iday is the day of the year as noahmp_hip_forcing_prep takes
    it (0 = 1 January) and rolls over into the next year."""
    year, iday, ihour, iminute, isecond = (int(x) for x in start)
    t = ((iday * 24 + ihour) * 60 + iminute) * 60 + isecond + int(seconds)
    assert t >= 0, "a time before the start of the year"
    iday, rest = divmod(t, 86400)
    while iday >= days_in_year(year):
        iday -= days_in_year(year)
        year += 1
    ihour, rest = divmod(rest, 3600)
    iminute, isecond = divmod(rest, 60)
    return year, iday, ihour, iminute, isecond


def sample_times(start, seconds, nsample, at="start"):
    """The nsample times of the interval [start, start + seconds): at="start" k * seconds / nsample (the step times of a model that makes
    nsample steps per record, for which the zenith weighting conserves the record's energy exactly), at="mid" the midpoints; whole seconds."""
    assert at in ("start", "mid") and nsample >= 1
    if at == "start":
        off = [k * int(seconds) // nsample for k in range(nsample)]
    else:
        off = [(2 * k + 1) * int(seconds) // (2 * nsample) for k in range(nsample)]
    return [time_after(start, o) for o in off]


def normal_from_height(z, dx, dy, cosalpha=None, sinalpha=None):
    """The upward unit normal (east, north, up), the slope and the aspect [radians; downslope azimuth clockwise from true north] of a
    terrain height z, an (nj, ni) torch plane, on a grid of spacing dx (along i) and dy (along j) [the unit of z]: central differences,
    one-sided at the tile's edge.  cosalpha / sinalpha (WRF's COSALPHA / SINALPHA: the local rotation of the grid's y axis against true
    north) turn the gradient from grid to earth coordinates."""
    import torch
    z = z.to(torch.float32)
    gx, gy = torch.zeros_like(z), torch.zeros_like(z)
    if z.shape[1] > 1:
        gx[:, 1:-1] = (z[:, 2:] - z[:, :-2]) / (2.0 * dx)
        gx[:, 0] = (z[:, 1] - z[:, 0]) / dx
        gx[:, -1] = (z[:, -1] - z[:, -2]) / dx
    if z.shape[0] > 1:
        gy[1:-1, :] = (z[2:, :] - z[:-2, :]) / (2.0 * dy)
        gy[0, :] = (z[1, :] - z[0, :]) / dy
        gy[-1, :] = (z[-1, :] - z[-2, :]) / dy
    if cosalpha is not None:                       # grid (x, y) -> earth (east, north), the rotation WRF applies to its winds
        ge = gx * cosalpha - gy * sinalpha
        gn = gx * sinalpha + gy * cosalpha
    else:
        ge, gn = gx, gy
    g2 = ge * ge + gn * gn
    norm = torch.sqrt(g2 + 1.0)
    slope = torch.atan(torch.sqrt(g2))
    aspect = torch.remainder(torch.atan2(-ge, -gn), 2.0 * math.pi)
    return -ge / norm, -gn / norm, 1.0 / norm, slope, aspect      # the upward normal of z(x, y) is (-dz/dx, -dz/dy, 1) / |.|


class Shortwave:
    def __init__(self, engine, xlat, xlon, mode="zenith", max_ratio=10.0, mu_min=0.05, max_terrain_ratio=5.0, solar_constant=1361.0):
        import torch
        assert xlat.dtype == torch.float32 and xlon.dtype == torch.float32 and xlat.shape == xlon.shape and xlat.dim() == 2
        assert mode in ("linear", "zenith")
        self.engine, self.torch, self.mode = engine, torch, mode
        self.nj, self.ni = xlat.shape
        self.ncell = self.ni * self.nj
        self.device = xlat.device
        self.par = dict(max_ratio=max_ratio, mu_min=mu_min, max_terrain_ratio=max_terrain_ratio, solar_constant=solar_constant)
        self.lat_tile, self.lon_tile = xlat.contiguous(), xlon.contiguous()
        self.lat, self.lon = self.lat_tile, self.lon_tile          # in the column order the records are in
        self.normal_tile = self.normal = None                        # (east, north, up) planes
        self.perm = None
        self.means = [None, None]                                    # two interval-mean planes, used alternately
        self.turn = 0
        self.mean_a = None                                           # the plane the last interval() filled
        self.shadow = None                                           # set_shadow: the window planes and the noahmp_shadow block
        self.lit = None                                              # the lit plane, in the column order the records are in
        self.shadow_calls = 0
        self.sky = None                                              # set_skyview: the sources of the per-step planes and the constants
        self.svf_tile = self.svf = None                              # the sky-view plane in tile order / the column order the records are in
        torch.cuda.current_stream().synchronize()

    # ---- terrain
    def set_normal(self, e, n, u):
        """Unit surface normals in east / north / up components: (nj, ni) planes in the CURRENT column order."""
        torch = self.torch
        planes = tuple(t.to(torch.float32).contiguous() for t in (e, n, u))
        assert all(t.numel() == self.ncell for t in planes)
        self.normal = planes
        self.normal_tile = tuple(self._tile_order(t) for t in planes)
        torch.cuda.current_stream().synchronize()      # complete before an apply() reads them on the engine's stream

    def set_terrain(self, slope, aspect):
        """slope [radians] and aspect [radians, the downslope azimuth clockwise from true north]: the normal is
        (sin s * sin a, sin s * cos a, cos s)."""
        torch = self.torch
        s, a = slope.to(torch.float32), aspect.to(torch.float32)
        self.set_normal(torch.sin(s) * torch.sin(a), torch.sin(s) * torch.cos(a), torch.cos(s))

    def terrain_from_height(self, z, dx, dy, cosalpha=None, sinalpha=None):
        """set_normal(normal_from_height(...)) for the model's terrain height z, an (nj, ni) plane in TILE order.  Returns (slope, aspect)."""
        assert self.perm is None, "terrain_from_height takes tile order: call it before follow(), follow() permutes the normals"
        e, n, u, slope, aspect = normal_from_height(z, dx, dy, cosalpha, sinalpha)
        self.set_normal(e, n, u)
        return slope, aspect

    # ---- cast shadows
    def set_shadow(self, height, dx, dy, nstep=25, origin=(0, 0), cosalpha=None, sinalpha=None, height_max=None, every=1):
        """Cast shadows on the direct beam (noahmp_hip_forcing_shadow + noahmp_hip_forcing_shortwave_lit).  height: the terrain height
        [m] of an (nj_w, ni_w) WINDOW that contains the tile with its cell (0, 0) at window cell origin = (i0, j0); the cells around the
        tile are the margin that lets a ray cross the tile's edge: at least nstep cells on every side that is not an edge of the whole
        domain give the bits of the undecomposed run.  dx, dy: grid spacing [m]; nstep: cells marched (25 at 1 km = WRF's shadlen);
        cosalpha / sinalpha: WRF's rotation planes over the window, or None (grid y is true north).  height_max defaults to the
        WINDOW's maximum: a decomposed run must pass the GLOBAL maximum, the same number on every rank, or ranks disagree on where a
        ray is above all terrain.  every: the lit plane is made again at every `every`-th apply() and reused in between (the sun moves
        0.25 degrees per minute).  apply() then enqueues the shadow launch and the lit shortwave call in place of the unshaded one;
        terrain normals are optional.  Works before or after follow()."""
        torch = self.torch
        assert height.dim() == 2 and (cosalpha is None) == (sinalpha is None) and int(every) >= 1
        i0, j0 = check_window(height.shape, origin, self.ni, self.nj)
        h = height.to(torch.float32).contiguous()
        lat, lon = torch.zeros_like(h), torch.zeros_like(h)      # only tile cells are marched, so only they need a sun
        lat[j0:j0 + self.nj, i0:i0 + self.ni] = self.lat_tile
        lon[j0:j0 + self.nj, i0:i0 + self.ni] = self.lon_tile
        rot = None
        if cosalpha is not None:
            rot = tuple(t.to(torch.float32).contiguous() for t in (cosalpha, sinalpha))
            assert all(t.shape == h.shape for t in rot)
        hmax = float(height_max) if height_max is not None else float(h.max().item())
        self.shadow = dict(height=h, lat=lat, lon=lon, rot=rot, dx=float(dx), dy=float(dy), nstep=int(nstep), origin=(i0, j0), height_max=hmax,
                           every=int(every))
        self.lit = torch.empty((self.nj, self.ni), dtype=torch.float32, device=self.device)
        self.shadow_calls = 0
        self._shadow_index()

    def _shadow_index(self):
        """dst_index of the shadow window: the position of every tile cell in the current column order, -1 in the margin."""
        torch = self.torch
        sh = self.shadow
        pos = inverse_perm(self.perm) if self.perm is not None else None
        rot = sh["rot"] or (None, None)
        sh["index"] = window_index(sh["height"].shape, sh["origin"], self.ni, self.nj, pos=pos, device=self.device)
        sh["block"] = self.engine.shadow_block(sh["height"], sh["lat"], sh["lon"], self.lit, sh["dx"], sh["dy"], nstep=sh["nstep"], cosalpha=rot[0],
                                               sinalpha=rot[1], dst_index=sh["index"], mu_min=self.par["mu_min"], height_max=sh["height_max"])
        self.shadow_calls = 0
        torch.cuda.current_stream().synchronize()      # complete before an apply() reads them on the engine's stream

    # ---- sky-view factor
    def set_skyview(self, height, dx, dy, nstep=25, ndir=16, origin=(0, 0), albedo="store", longwave=True, emiss="store", tsurf="tsk",
                    sigma=5.67e-8):
        """Sky-view factor in the radiation (noahmp_hip_skyview + noahmp_hip_forcing_radiation_sky).  height, dx, dy, origin: the WINDOW of
        set_shadow (a caller that uses both passes the same window); a margin of at least nstep cells on every side that is not an edge of
        the whole domain gives the bits of the undecomposed run.  The terrain is scanned ONCE, here, along ndir directions (grid
        coordinates, (float32) sin / cos (2 pi q / ndir)) for nstep cells each, into a tile-order plane that is kept; follow() permutes it.
        apply() then enqueues the shadow launch as before (if set_shadow was called) and the radiation call in place of the shortwave
        call: the diffuse shortwave is narrowed to the visible sky, the closed part of the hemisphere reflects with `albedo`, and -- with
        longwave=True -- the store's GLW becomes svf*GLW + (1 - svf)*emiss*sigma*tsurf^4.  albedo / emiss: "store" = the plane of that name
        of the store passed to apply(), or a float = the constant of every column; tsurf: the name of the store's temperature plane.
        ALBEDO and EMISS are OUTPUTS of the step: before the first step the caller gives constants here or initialised planes in the
        store.  Works before or after follow()."""
        torch = self.torch
        assert height.dim() == 2
        index = window_index(height.shape, origin, self.ni, self.nj, device=self.device)
        h = height.to(torch.float32).contiguous()
        self.svf_tile = torch.empty((self.nj, self.ni), dtype=torch.float32, device=self.device)
        torch.cuda.current_stream().synchronize()
        self.engine.skyview(self.engine.skyview_block(h, self.svf_tile, dx, dy, nstep=nstep, ndir=ndir, dst_index=index), self.ncell)
        self.engine.stream_sync()
        self.sky = dict(albedo=albedo, emiss=emiss, tsurf=tsurf, longwave=bool(longwave), sigma=float(sigma))
        self.svf = self.svf_tile
        if self.perm is not None:
            self.svf = permute_planes(self.engine, [self.svf_tile], self.perm, self.ni, self.nj)[0]

    def _sky_block(self, store):
        sky = self.sky
        plane = lambda v: store.a[v] if isinstance(v, str) else v      # noqa: E731  "store" names the plane of the store, a float is the constant
        albedo = plane("albedo" if sky["albedo"] == "store" else sky["albedo"])
        emiss = plane("emiss" if sky["emiss"] == "store" else sky["emiss"])
        glw = store.a["glw"] if sky["longwave"] else None
        tsurf = store.a[sky["tsurf"]] if sky["longwave"] else None
        return self.engine.sky_block(self.svf, lit=self.lit if self.shadow is not None else None, albedo=albedo, glw=glw, tsurf=tsurf,
                                     emiss=emiss, sigma=sky["sigma"])

    def _tile_order(self, plane):
        return to_tile_order(self.engine, plane, self.perm, self.ni, self.nj)

    def follow(self, store):
        """After Engine.sort_store(store): lat, lon and the normals, permuted into the store's column order with noahmp_hip_gather_fields.
        Waits for the engine's stream.  Interval means made before the call keep the old order: make them again."""
        perm = sorted_perm(store, self.ni, self.nj)
        src = [self.lat_tile, self.lon_tile] + list(self.normal_tile or ()) + ([self.svf_tile] if self.svf_tile is not None else [])
        dst = permute_planes(self.engine, src, perm, self.ni, self.nj)
        self.lat, self.lon, self.perm = dst[0], dst[1], perm
        self.normal = tuple(dst[2:5]) if self.normal_tile is not None else None
        if self.svf_tile is not None:
            self.svf = dst[-1]
        self.means = [None, None]
        self.mean_a = None
        if self.shadow is not None:
            self._shadow_index()

    # ---- per record
    def interval(self, start, seconds, nsample, at="start", stream=None):
        """The mean of max(cos zenith, 0) over nsample times of [start, start + seconds), start = (year, iday, ihour, iminute, isecond):
        one launch, enqueued only.  Returns the plane (and keeps it as mean_a for apply); two planes are used alternately."""
        torch = self.torch
        times = [t[1:] for t in sample_times(start, seconds, nsample, at)]
        if self.means[self.turn] is None:
            self.means[self.turn] = torch.empty((self.nj, self.ni), dtype=torch.float32, device=self.device)
            torch.cuda.current_stream().synchronize()
        out = self.means[self.turn]
        self.turn ^= 1
        self.engine.cosz_mean(self.lat, self.lon, times, out, stream=stream)
        self.mean_a = out
        return out

    # ---- per step
    def apply(self, store, rec_a, rec_b, idts, idts2, now, mean_a=None, stream=None):
        """The store's SWDOWN at now = (iday, ihour, iminute, isecond) from the records' "sw" planes: one launch, enqueued only.  Call it
        after forcing_interpolate[_prep] on the same stream.  rec_b may be None; it is read in mode "linear" only."""
        mean_a = mean_a if mean_a is not None else self.mean_a
        if self.mode == "zenith" and mean_a is None:
            raise ValueError("mode 'zenith' needs the interval mean of record a: call interval() first")
        sw_b = rec_b["sw"] if (rec_b is not None and self.mode == "linear") else None
        block = self.engine.shortwave_block(rec_a["sw"], self.lat, self.lon, store.a["swdown"], sw_b=sw_b,
                                            mean_a=mean_a if self.mode == "zenith" else None, normal=self.normal, idts=idts, idts2=idts2,
                                            mode=self.mode, **self.par)
        if self.shadow is None and self.sky is None:
            self.engine.forcing_shortwave(block, self.ncell, now, stream=stream)
            return
        if self.shadow is not None:
            if self.shadow_calls % self.shadow["every"] == 0:
                self.engine.forcing_shadow(self.shadow["block"], self.ncell, now, stream=stream)
            self.shadow_calls += 1
        if self.sky is None:
            self.engine.forcing_shortwave_lit(block, self.lit, self.ncell, now, stream=stream)
        else:
            self.engine.forcing_radiation_sky(block, self._sky_block(store), self.ncell, now, stream=stream)
