"""Discharge of a device-resident run: cell-to-cell linear reservoirs on a D8 network (noahmp_hip_flow_terrain / _flow_inmask /
_flow_accumulate / noahmp_hip_route_runoff), on raw terrain or on terrain conditioned on the device (noahmp_hip_flow_fill_init /
noahmp_hip_flow_fill), the basins of gauge cells on that network (noahmp_hip_flow_basin_init / _jump / _resolve; class Basins below)
and the weighted upstream sums (noahmp_hip_flow_upstream_init / _pass; class Upstream below), and a kinematic wave with Manning
friction in place of the linear reservoirs (noahmp_hip_flow_channel / noahmp_hip_route_kinematic; class ChannelFlow below).

    net = FlowNetwork(engine, ni, nj)                              # the tile of the store
    net.set_terrain(height, dx, dy, origin=(i0, j0))               # once: height is a WINDOW = tile + 2 cells where there is a neighbour
    #   or: net.set_terrain(height, dx, dy, fill=1e-3)             single tile: depressions filled, flats resolved first (net.filled)
    #   or: net.set_terrain_filled(height_block, dx, dy, 1e-3, origin=(i0, j0), comm=comm, geom=geom)      the decomposed recipe
    #   or: net.set_directions(FlowNetwork.from_esri(codes), origin=(i0, j0), dx=dx, dy=dy)      codes: a window = tile + 1-cell ring
    net.set_area(area); net.set_velocity(0.5, dt)                  # m2 per cell; release = 1 - exp(-dt*v/length)
    net.follow(store)                                              # after Engine.sort_store: only col_index is rewritten
    engine.noahmplsm(store, ...); net.step(store, dt)              # per step: one launch (nsub launches), enqueued only
    q = net.discharge()                                            # m3/s leaving every cell of the block in the last step

Every cell gathers what its upstream neighbours released in the call before, adds (RUNSFXY + RUNSBXY) * dt * 1e-3 * area of its column
and releases the fraction `release` of its storage; water leaves the network at the cells without a direction (outlets, pits, the coast).
The window planes (the BLOCK: the tile plus a 1-cell ring where the window given has room for one) never move; a sorted store is followed
through col_index alone.  Not represented by the reservoirs: a celerity that depends on the water held (ChannelFlow does that), a
celerity above one cell per call (nsub sub-steps); by neither: diffusive wave, backwater and losses.  Lakes with storage: class Lakes below.

Conditioning a raw DEM (DepressionFill; set_terrain(fill=eps); set_terrain_filled): the surface W* of priority-flood + epsilon, made on the
device as the fixed point of a monotone relaxation, the same bits in every schedule and every decomposition.  Built: every cell that can
reach an outlet drains; flats and filled depressions become ramps of one lift (eps, or one float32 step where eps is below it) per cell
away from their outlet.  Not built: carving / breaching, a combined-gradient flat resolution (Garbrecht-Martz).
Without fill, set_terrain takes the terrain as it is: water leaves the network at every pit.  The contract -- every rounding -- is the
text in include/noahmp_hip.h.
"""
import math

import numpy as np

from .tile import check_window, inverse_perm, sorted_perm, window_index

ESRI_CODES = {1: 1, 128: 2, 64: 3, 32: 4, 16: 5, 8: 6, 4: 7, 2: 8}      # ESRI / WRF-Hydro FLOWDIRECTION (E = 1, clockwise) -> k, with j towards north
NOT_OWNED = -2                                                           # col_index of a ring cell
# in-tile sweeps per call of noahmp_hip_flow_fill, from profiles/flow_fill_bench.md (tools/flow_fill_bench.py, one MI355X, device time
# to the fixed point): 16 is the fastest setting at 7 077 888 cells (3.13 ms; 4: 3.41, 64: 3.31, pinned: 46.4) and second at 884 736 cells
# (1.03 ms; 4: 0.85, 64: 1.15, pinned: 5.21).  No setting is fastest at both sizes; 16 has the smallest sum over the two.
FILL_SWEEPS = 16


class DepressionFill:
    """The filled surface W* of a height window (noahmp_hip_flow_fill_init / noahmp_hip_flow_fill).

        fill = DepressionFill(engine)
        fill.begin(height, eps)                  # every window edge an outlet side
        w = fill.run()                           # calls until one changes nothing; fill.calls counts them
    """

    def __init__(self, engine):
        import torch
        self.engine, self.torch = engine, torch
        self.height = self.fixed = self.outlet = None
        self.w, self.cur = None, 0
        self.flags = self.eps = None
        self.changed = None                                              # two device words: [0] the calls before the last of a relax(), [1] the last
        self.free_cells = self.calls = 0
        self._blocks = {}

    @staticmethod
    def _side_flags(outlet_sides, ring_sides):
        from . import abi
        f = 0
        for kind, sides in (("outlet", outlet_sides), ("ring", ring_sides)):
            for s in sides.lower():
                if s not in "wesn":
                    raise ValueError("sides are letters of 'wesn', not %r" % s)
                f |= abi.FILL_FLAG["%s_%s" % (kind, s)]
        return f

    def begin(self, height_window, eps, outlet=None, outlet_sides="wesn", ring_sides=""):
        """height_window: (nj, ni) float32 device plane [m].  eps: the lift increment [m].  outlet: uint8 plane, non-zero = a caller
        outlet, or None.  outlet_sides / ring_sides: letters of "wesn"; a side in neither is a closed wall.  One launch; w is z at the
        outlets and +inf elsewhere, a ring waits for the caller's exchange."""
        torch = self.torch
        assert height_window.dim() == 2
        self.height = height_window.to(torch.float32).contiguous()
        dev = self.height.device
        self.outlet = None if outlet is None else (outlet != 0).to(torch.uint8).contiguous()
        self.fixed = torch.empty(self.height.shape, dtype=torch.uint8, device=dev)
        self.w, self.cur = [torch.empty_like(self.height), torch.empty_like(self.height)], 0
        self.changed = torch.zeros(2, dtype=torch.int32, device=dev)
        self.flags, self.eps = self._side_flags(outlet_sides, ring_sides), float(eps)
        self._blocks = {}
        torch.cuda.current_stream().synchronize()
        self.engine.flow_fill_init(self._block(0, 0, 1))
        self.engine.stream_sync()
        self.free_cells = int((self.fixed == 0).sum().item())
        self.calls = 0

    def _block(self, cur, word, sweeps):
        key = (cur, word, sweeps)
        b = self._blocks.get(key)
        if b is None:
            b = self._blocks[key] = self.engine.flow_fill_block(self.height, self.fixed, self.w[cur], self.w[1 - cur], self.changed[word:word + 1],
                                                                self.eps, sweeps=sweeps, flags=self.flags, outlet=self.outlet)
        return b

    @property
    def surface(self):
        """The current plane w (W* once a call has changed nothing)."""
        return self.w[self.cur]

    def relax(self, ncall=1, sweeps=None):
        """ncall calls of noahmp_hip_flow_fill, enqueued in a row, ping-ponging the two planes; returns the LAST call's flag (0: it changed
        nothing, the surface is W*).  The last call stores into a flag word of its own, zeroed with the other before the batch, so there
        is one host wait per relax(), not one per call."""
        torch = self.torch
        sweeps = FILL_SWEEPS if sweeps is None else int(sweeps)
        assert ncall >= 1 and self.w is not None
        self.changed.zero_()
        torch.cuda.current_stream().synchronize()
        for n in range(int(ncall)):
            self.engine.flow_fill(self._block(self.cur, 1 if n == ncall - 1 else 0, sweeps))
            self.cur = 1 - self.cur
        self.engine.stream_sync()
        self.calls += int(ncall)
        return int(self.changed[1].item())

    def run(self, max_call=None, check=8, sweeps=None, comm=None, geom=None):
        """Calls until one changes nothing; returns the surface W*.  The flag is read every `check` calls.  max_call defaults to the number
        of free cells + 1 (every call lowers at least the cells a Jacobi pass lowers, and a Jacobi pass that lowers anything brings at
        least one more cell to its final value); exceeding it raises.
        With a comm (the window is the block: the tile plus the ring sides given to begin()), EVERY call is preceded by
        comm.exchange_halo([w], geom) and followed by comm.agree_any(flag): the loop ends when no rank changed anything in a call that
        followed an exchange.  max_call is then the caller's, the same number on every rank (None: no limit; the loop ends by the
        argument in DESIGN.md section 6).  THE STREAM RULE of FlowNetwork.step holds: the exchange runs on torch's current stream, the
        launches on the engine's; each waits for the other."""
        torch = self.torch
        if comm is None:
            max_call = self.free_cells + 1 if max_call is None else int(max_call)
            while self.calls < max_call:
                if self.relax(min(int(check), max_call - self.calls), sweeps) == 0:
                    return self.surface
            raise RuntimeError("DepressionFill.run: still changing after %d calls" % self.calls)
        while max_call is None or self.calls < int(max_call):
            self.engine.stream_sync()                                    # w is written before it travels
            comm.exchange_halo([self.surface], geom)
            torch.cuda.current_stream().synchronize()                    # ... and its ring has arrived before the call reads it
            if not comm.agree_any(self.relax(1, sweeps) != 0):
                return self.surface
        raise RuntimeError("DepressionFill.run: still changing on some rank after %d calls" % self.calls)


class FlowNetwork:
    def __init__(self, engine, ni, nj):
        import torch
        self.engine, self.torch = engine, torch
        self.ni, self.nj = int(ni), int(nj)
        self.ncell = self.ni * self.nj
        self.dir = self.inmask = None                                    # uint8, the block
        self.i0 = self.j0 = 0                                            # the tile's cell (0, 0) inside the block
        self.dx = self.dy = None
        self.area = self.release = self.storage = None
        self.out = None                                                  # the two out planes; out[cur] holds the last call's
        self.cur = 0
        self.col_index = None
        self.has_input = None                                            # bool, tile order: None = every column
        self._input_known = False                                        # False: step() derives has_input from its store
        self.perm = None
        self.last_dt = None
        self.passes = 0                                                  # passes the last upstream_cells() made
        self._area_default = True                                        # area is dx*dy of the last set_directions, not the caller's
        self.filled = None                                               # the filled height plane of set_terrain(fill=...) / set_terrain_filled
        self.fill_calls = 0                                              # calls of noahmp_hip_flow_fill it took
        self.window_shape = self.window_block = None                     # the window of the last set_directions and the block's slices in it
        self.after_launch = []                                           # f(out_new, dt_sub, comm, stream) after every launch of a step (Lakes.attach)
        self.held = None                                                 # bool plane of the block: cells that hold their water (Lakes.set_lakes)

    # ---- the network
    @staticmethod
    def from_esri(codes):
        """The 1 / 2 / 4 / ... / 128 codes of an ESRI / WRF-Hydro FLOWDIRECTION grid (rows from south to north, as the model's j) as
        directions 0..8 (uint8, numpy or torch in, the same out).  Every other code (0, 255, nodata) becomes 0."""
        lut = np.zeros(256, np.uint8)
        for code, k in ESRI_CODES.items():
            lut[code] = k
        if isinstance(codes, np.ndarray):
            c = codes.astype(np.int64)
            return np.where((c >= 0) & (c < 256), lut[np.clip(c, 0, 255)], 0).astype(np.uint8)
        import torch
        c = codes.to(torch.int64)
        t = torch.from_numpy(lut).to(codes.device)
        return torch.where((c >= 0) & (c < 256), t[c.clamp(0, 255)], torch.zeros((), dtype=torch.uint8, device=codes.device))

    def _block_of(self, shape, origin):
        i0, j0 = check_window(shape, origin, self.ni, self.nj)
        nj_w, ni_w = shape
        w, s = min(1, i0), min(1, j0)
        e, n = min(1, ni_w - i0 - self.ni), min(1, nj_w - j0 - self.nj)
        return (slice(j0 - s, j0 + self.nj + n), slice(i0 - w, i0 + self.ni + e)), (w, s)

    def set_terrain(self, height, dx, dy, origin=(0, 0), fill=None, outlet=None):
        """height: the terrain height [m] of an (nj_w, ni_w) float32 device WINDOW that contains the tile with its cell (0, 0) at window
        cell origin = (i0, j0): the tile plus 2 cells on every side that is not an edge of the whole domain gives, on the block, the
        directions of the undecomposed run.  Two launches, once.
        fill = eps [m]: SINGLE-TILE conditioning.  The window is filled first (DepressionFill, every window edge an outlet side, `outlet`
        an optional uint8 plane of caller outlets) and the directions are those of the filled plane, kept as self.filled.  A filled
        surface is global: a decomposed caller uses set_terrain_filled."""
        torch = self.torch
        assert height.dim() == 2
        h = height.to(torch.float32).contiguous()
        self.filled = None
        if fill is not None:
            f = DepressionFill(self.engine)
            f.begin(h, fill, outlet=outlet)
            h = self.filled = f.run()
            self.fill_calls = f.calls
        d = torch.empty(h.shape, dtype=torch.uint8, device=h.device)
        torch.cuda.current_stream().synchronize()
        self.engine.flow_terrain(self.engine.flow_terrain_block(h, d, dx, dy))
        self.engine.stream_sync()
        self.set_directions(d, origin=origin, dx=dx, dy=dy)

    def set_terrain_filled(self, height_block, dx, dy, eps, origin=(0, 0), outlet=None, comm=None, geom=None):
        """The decomposed recipe.  height_block: the terrain height [m] of the BLOCK, the tile plus a 1-cell
        ring on every side where a neighbour rank exists, the tile's cell (0, 0) at block cell origin = (i0, j0).  Sides with a ring are
        RING sides of the fill, the others OUTLET sides.  (1) fill on the block, (2) the ring of w exchanged before every call
        (DepressionFill.run), (3) noahmp_hip_flow_terrain on the filled block -- right on the tile's cells, (4) the ring's directions
        through the same exchange as a float32 plane (0..8 are exact), (5) set_directions.  The filled block is kept as self.filled."""
        torch = self.torch
        assert height_block.dim() == 2
        i0, j0 = check_window(tuple(height_block.shape), origin, self.ni, self.nj)
        nj_b, ni_b = height_block.shape
        room = dict(w=i0, e=ni_b - i0 - self.ni, s=j0, n=nj_b - j0 - self.nj)
        if any(v not in (0, 1) for v in room.values()):
            raise ValueError("set_terrain_filled takes the block: the tile plus a ring of ONE cell where there is a neighbour")
        ring = "".join(k for k, v in room.items() if v == 1)
        if ring and comm is None:
            raise ValueError("a block with a ring needs the comm that fills it")
        f = DepressionFill(self.engine)
        f.begin(height_block, eps, outlet=outlet, outlet_sides="".join(k for k in "wesn" if k not in ring), ring_sides=ring)
        self.filled = f.run(comm=comm, geom=geom) if ring else f.run()
        self.fill_calls = f.calls
        d = torch.empty(self.filled.shape, dtype=torch.uint8, device=self.filled.device)
        torch.cuda.current_stream().synchronize()
        self.engine.flow_terrain(self.engine.flow_terrain_block(self.filled, d, dx, dy))
        self.engine.stream_sync()
        if ring:
            df = d.to(torch.float32)
            comm.exchange_halo([df], geom)
            torch.cuda.current_stream().synchronize()
            d = df.to(torch.uint8)
        self.set_directions(d, origin=origin, dx=dx, dy=dy)

    def set_directions(self, dir_window, origin=(0, 0), dx=None, dy=None):
        """dir_window: directions 0..8 (uint8 device plane, e.g. from_esri of a FLOWDIRECTION grid) of a window that contains the tile
        at origin; the block is the tile plus the 1-cell ring the window has room for.  Raises on a value outside 0..8.  dx, dy [m]: for
        set_velocity and the default area dx*dy; without them the caller gives set_area and set_release.  One launch."""
        torch = self.torch
        assert dir_window.dim() == 2 and dir_window.dtype == torch.uint8
        if int(dir_window.max().item()) > 8:
            raise ValueError("directions are 0 (none) or 1..8 (E, NE, N, NW, W, SW, S, SE); FlowNetwork.from_esri converts ESRI codes")
        block, (self.i0, self.j0) = self._block_of(tuple(dir_window.shape), origin)
        self.window_shape, self.window_block = tuple(dir_window.shape), block      # for ChannelFlow: cutting a plane of the same window
        self.dir = dir_window[block].contiguous()
        self.inmask = torch.empty_like(self.dir)
        self.dx, self.dy = (float(dx), float(dy)) if dx is not None and dy is not None else (None, None)
        torch.cuda.current_stream().synchronize()
        self.engine.flow_inmask(self.dir, self.inmask)
        self.engine.stream_sync()
        dev = self.dir.device
        zeros = lambda: torch.zeros(self.dir.shape, dtype=torch.float32, device=dev)      # noqa: E731
        self.storage, self.out, self.cur = zeros(), [zeros(), zeros()], 0
        if self._area_default or self.area is None or self.area.shape != self.dir.shape:      # the caller's area is kept, a default is remade
            self.area = torch.full(self.dir.shape, self.dx * self.dy, dtype=torch.float32, device=dev) if self.dx is not None else None
            self._area_default = True
        if self.release is None or self.release.shape != self.dir.shape:
            self.release = torch.ones(self.dir.shape, dtype=torch.float32, device=dev)
        self._index()

    @property
    def block_shape(self):
        return tuple(self.dir.shape)

    def tile_view(self, plane):
        """The tile's cells of a block plane."""
        return plane[self.j0:self.j0 + self.nj, self.i0:self.i0 + self.ni]

    def _index(self):
        torch = self.torch
        dev = self.dir.device
        if self.perm is not None:                                        # sorted position p holds tile column perm[p]
            pos = inverse_perm(self.perm)
        else:
            pos = torch.arange(self.ncell, dtype=torch.int32, device=dev)
        if self.has_input is not None:
            pos = torch.where(self.has_input.reshape(-1), pos, torch.full_like(pos, -1))
        self.col_index = window_index(self.dir.shape, (self.i0, self.j0), self.ni, self.nj, pos=pos, fill=NOT_OWNED, device=dev)
        torch.cuda.current_stream().synchronize()

    def set_input_columns(self, has_input):
        """has_input: bool plane of the tile in TILE order, False where a column has no local input (water and skipped columns, whose
        RUNSFXY / RUNSBXY the step never writes), or None = every column."""
        self.has_input = None if has_input is None else has_input.to(self.torch.bool).reshape(self.nj, self.ni)
        self._input_known = True
        if self.dir is not None:
            self._index()

    def follow(self, store):
        """After Engine.sort_store(store): only col_index is rewritten, from the inverse permutation.  The window planes never move."""
        self.perm = sorted_perm(store, self.ni, self.nj)
        if self.dir is not None:
            self._index()

    def upstream_cells(self, max_pass=None):
        """The number of cells that drain through every cell of the block, itself included (uint32 words in an int32 device plane):
        noahmp_hip_flow_accumulate until nothing changes, the flag read every 64 passes.  SINGLE-TILE: the block's edge counts as the
        domain's; a decomposed caller exchanges acc after every pass and agrees on `changed` itself.  max_pass defaults to 4*(ni + nj).
        It needs one pass per cell of the longest flow path: Basins(net).run() gives that length (hops.max() + 1) in a logarithmic number
        of launches."""
        torch = self.torch
        nj, ni = self.block_shape
        max_pass = 4 * (ni + nj) if max_pass is None else int(max_pass)
        a = torch.ones((nj, ni), dtype=torch.int32, device=self.dir.device)
        b = torch.empty_like(a)
        changed = torch.zeros(1, dtype=torch.int32, device=self.dir.device)
        torch.cuda.current_stream().synchronize()
        done = 0
        while done < max_pass:
            n = min(64, max_pass - done)
            for _ in range(n - 1):
                self.engine.flow_accumulate(self.inmask, a, b, changed)
                a, b = b, a
            self.engine.stream_sync()
            changed.zero_()                                              # the flag of the LAST pass of the batch decides
            torch.cuda.current_stream().synchronize()
            self.engine.flow_accumulate(self.inmask, a, b, changed)
            a, b = b, a
            self.engine.stream_sync()
            done += n
            self.passes = done
            if int(changed.item()) == 0:
                return a
        raise RuntimeError("upstream_cells: still changing after %d passes: the flow paths are longer than that, or caller-given "
                           "directions hold a cycle" % max_pass)

    # ---- the reservoirs
    def _plane(self, plane, name):
        torch = self.torch
        if not torch.is_tensor(plane):
            plane = torch.full(self.block_shape, float(plane), dtype=torch.float32, device=self.dir.device)
        plane = plane.to(torch.float32)
        if tuple(plane.shape) == (self.nj, self.ni) and self.block_shape != (self.nj, self.ni):
            full = torch.zeros(self.block_shape, dtype=torch.float32, device=self.dir.device)
            self.tile_view(full).copy_(plane)
            plane = full
        assert tuple(plane.shape) == self.block_shape, "%s: a plane of the block %s or of the tile" % (name, self.block_shape)
        return plane.contiguous()

    def set_area(self, plane):
        """Cell area [m2]: a number, or a float32 device plane of the block or of the tile."""
        self.area = self._plane(plane, "area")
        self._area_default = False

    def set_release(self, plane):
        """The fraction of its storage every cell releases per call, in [0, 1] (not checked; 0 holds the water)."""
        self.release = self._plane(plane, "release")
        self._hold()

    def set_velocity(self, velocity, dt):
        """release = 1 - exp(-dt*velocity/length), made in float64 on the host and rounded once; length = dx, dy or the diagonal by the
        cell's direction (dx where it has none).  velocity [m/s]: a number or a plane of the block or the tile."""
        assert self.dx is not None, "set_velocity needs the dx, dy of set_terrain / set_directions"
        v = self._plane(velocity, "velocity").cpu().numpy().astype(np.float64)
        d = self.dir.cpu().numpy()
        diag = math.sqrt(self.dx * self.dx + self.dy * self.dy)
        length = np.where(d == 0, self.dx, np.where(d % 2 == 0, diag, np.where((d == 3) | (d == 7), self.dy, self.dx)))
        r = (1.0 - np.exp(-float(dt) * v / length)).astype(np.float32)
        self.release = self.torch.from_numpy(r).to(self.dir.device).contiguous()
        self._hold()

    def _hold(self):
        """release = 0 at the held cells (the members of Lakes.set_lakes), whatever the caller's plane says there."""
        if self.held is not None and self.release is not None and self.release.shape == self.held.shape:
            self.release.masked_fill_(self.held, 0.0)
            self.torch.cuda.current_stream().synchronize()

    def step(self, store, dt, fields=("runsfxy", "runsbxy"), nsub=1, comm=None, geom=None, stream=None):
        """One model step of routing after Engine.noahmplsm: nsub launches with scale = dt*1e-3/nsub, ping-ponging the two out planes;
        with a comm, comm.exchange_halo([out], geom) refreshes the ring after every launch.  fields: one or two planes of the store in
        mm/s.  Without a comm the launches are enqueued only, on `stream` (None: the engine's own).
        THE STREAM RULE with a comm: the exchange is enqueued on torch's CURRENT stream (the RCCL and IPC transports return before their
        copies are done), which is in general not the stream the launch runs on.  So after every launch step() waits for `stream`, runs
        the exchange, and waits for torch's current stream: the next launch -- the next sub-step, or the next step's -- reads a ring that
        has arrived, whatever the two streams are."""
        ra, rb = self._runoff_planes(store, fields, nsub)
        scale = float(np.float32(dt) * np.float32(1e-3)) / nsub

        def launch(out_old, out_new):
            b = self.engine.route_block(self.inmask, self.col_index, self.area, self.release, self.storage, out_old, out_new, ra, rb, scale)
            self.engine.route_runoff(b, self.ncell, stream=stream)

        self._sub_steps(launch, dt, nsub, comm, geom, stream)

    def _runoff_planes(self, store, fields, nsub):
        """What every per-step call checks first; returns the one or two runoff planes of the store."""
        if self.dir is None:
            raise ValueError("call set_terrain() or set_directions() first")
        if self.area is None:
            raise ValueError("directions were given without dx, dy: call set_area() first")
        assert store.ni == self.ni and store.nj == self.nj and 1 <= len(fields) <= 2 and nsub >= 1
        if not self._input_known:
            self._auto_input(store)                                      # once: the columns the step advances
        return store.a[fields[0]], (store.a[fields[1]] if len(fields) > 1 else None)

    def _sub_steps(self, launch, dt, nsub, comm, geom, stream, also=None):
        """The loop of step(), ChannelFlow.step() and DiffusiveFlow.step(): nsub times launch(out_old, out_new), ping-ponging the two
        out planes, with the exchange of the new plane under THE STREAM RULE of step().  also: None, or a function of the new index
        that returns further planes written by that launch (DiffusiveFlow: the new depth plane); they travel with out[new] in the same
        exchange_halo call, so their ring has arrived before the next launch as well."""
        for _ in range(int(nsub)):
            new = 1 - self.cur
            launch(self.out[self.cur], self.out[new])
            self.cur = new
            for f in self.after_launch:                                  # e.g. the lakes: take and release, before out[new] travels
                f(self.out[new], float(dt) / nsub, comm, stream)
            if comm is not None:
                self.engine.stream_sync(stream)                          # out[new] is written before it travels
                comm.exchange_halo([self.out[new]] + (list(also(new)) if also is not None else []), geom)
                self.torch.cuda.current_stream().synchronize()           # ... and its ring has arrived before anybody reads it
        self.last_dt = float(dt) / nsub

    def _auto_input(self, store):
        """Columns with XLAND >= 1.5 (water) or XICE >= XICE_THRES (sea ice) are skipped by the step (drv:426-441): no local input."""
        xland, xice = store.a["xland"].reshape(-1), store.a["xice"].reshape(-1)
        has = ((xland - 1.5) < 0) & ~(xice >= float(store.cfg.xice_thres))
        if self.perm is not None:                                        # the store is sorted: back to tile order
            has = has[inverse_perm(self.perm).long()]
        self.set_input_columns(has.reshape(self.nj, self.ni))

    def discharge(self):
        """out / dt of the last call [m3/s], a plane of the block: at the cells without a direction it is the water leaving the network."""
        assert self.last_dt, "no step yet"
        return self.out[self.cur] / self.last_dt

    def state_dict(self):
        """The restart state: storage and the current out plane (copies)."""
        return dict(storage=self.storage.clone(), out=self.out[self.cur].clone())

    def load_state_dict(self, state):
        self.torch.cuda.current_stream().synchronize()
        self.engine.stream_sync()
        self.storage.copy_(state["storage"])
        self.out[self.cur].copy_(state["out"])
        self.torch.cuda.current_stream().synchronize()


BASIN_CHECK = 4                                                          # jump passes enqueued between two host waits
# in-tile iterations of the FIRST call of noahmp_hip_flow_basin_jump, which is then the tiled form; the calls after it are pinned passes.
# From profiles/basins_bench.md (tools/basins_bench.py, one MI355X, device time of the calls to the fixed point): on the filled terrain 9
# calls in 0.261 ms against 12 pinned passes in 0.359 ms at 7 077 888 cells and 8 in 0.052 against 11 in 0.076 ms at 884 736; on the raw
# terrain 4 against 5 calls, 0.155 / 0.164 and 0.037 / 0.038 ms.  The tiled form in EVERY call saves no further call and costs more per
# call (0.387 and 0.080 ms on the filled terrain).  12 = the 11 doublings a path inside a 64 x 32 tile can need and the one that moves nothing.
BASIN_SWEEPS = 12


class Basins:
    """Which gauge every cell of a FlowNetwork drains to, and how many cells away it is (noahmp_hip_flow_basin_init / _jump / _resolve):
    pointer doubling over the directions, ceil(log2 L) + 1 passes for a longest flow path of L cells.

        b = Basins(net)                          # a FlowNetwork with directions set; works on its block
        b.set_gauges([(i, j), ...])              # tile cells -> ids 0..n-1; or a block-shaped int32 seed plane (>= 0: a gauge's id)
        #   or: b.set_outlet_gauges()            single tile: every tile cell without a downstream cell, row-major ids
        b.run()                                  # decomposed: b.run(comm=comm, geom=geom)
        b.label, b.hops                          # int32 block planes; b.passes, b.rounds
        rg = Regions(engine, store, b.region_map(), b.ngauge)

    A gauge cell is the root of its INCREMENTAL area: cells above another gauge belong to that one.  downstream_gauge() and nested() turn
    incremental sums into whole-basin sums on the host.  label is the gauge's id, or NOAHMP_BASIN_NONE (-1: the path ends at a cell without
    a downstream cell that is no gauge), _PENDING (-2: it ends in a ring nobody answered for, or on a cycle across ranks), _CYCLE (-3: it
    ends on a cycle of caller-given directions).  hops counts the cells to the gauge or outlet, -1 where there is none.  Integer words and
    a unique fixed point: the same planes in every schedule and every decomposition.  Not represented: weighted or metric flow length."""

    def __init__(self, net):
        if net.dir is None:
            raise ValueError("the FlowNetwork has no directions: call set_terrain() or set_directions() first")
        self.net, self.engine, self.torch = net, net.engine, net.torch
        self.seed, self.ngauge = None, 0
        self.label = self.hops = self.state = self.changed = None
        self.cur = self.passes = self.rounds = 0
        self.cap = (max(net.dir.numel(), 1) - 1).bit_length() + 1          # ceil(log2(ni*nj)) + 1
        self._blocks = {}
        self._moved = None

    # ---- gauges
    def _block_dir(self):
        return self.net.dir.cpu().numpy()

    def set_gauges(self, points):
        """points: [(i, j)] in TILE cells, ids 0..n-1 in the order given; or an int32 plane of the block (numpy or device), >= 0 = the id
        of the gauge at that cell (a decomposed caller gives ids that mean the same on every rank), negative = none."""
        torch, net = self.torch, self.net
        dev = net.dir.device
        if torch.is_tensor(points) or (isinstance(points, np.ndarray) and points.ndim == 2 and tuple(points.shape) == net.block_shape):
            seed = torch.as_tensor(points, device=dev).to(torch.int32).contiguous()
            assert tuple(seed.shape) == net.block_shape, "a seed plane has the shape of the block %s" % (net.block_shape,)
            self.ngauge = max(0, int(seed.max().item()) + 1) if seed.numel() else 0
        else:
            pts = [(int(i), int(j)) for i, j in points]
            if len(set(pts)) != len(pts):
                raise ValueError("two gauges at one cell")
            plane = np.full(net.block_shape, -1, np.int32)
            for n, (i, j) in enumerate(pts):
                if not (0 <= i < net.ni and 0 <= j < net.nj):
                    raise ValueError("gauge %d at (%d, %d) lies outside the tile %d x %d" % (n, i, j, net.ni, net.nj))
                plane[net.j0 + j, net.i0 + i] = n
            seed = torch.from_numpy(plane).to(dev)
            self.ngauge = len(pts)
        self.seed = seed if self.ngauge else None
        self._blocks = {}

    def set_outlet_gauges(self):
        """SINGLE TILE: every tile cell without a downstream cell (no direction, or one that leaves the block) becomes a gauge; ids in
        row-major order of the tile.  Returns their (i, j)."""
        net = self.net
        down = _np_down(self._block_dir())
        tile = down[net.j0:net.j0 + net.nj, net.i0:net.i0 + net.ni]
        jj, ii = np.nonzero(tile < 0)
        pts = list(zip(ii.tolist(), jj.tolist()))
        self.set_gauges(pts)
        return pts

    # ---- the calls
    def ring_sides(self):
        """The sides of the block that are a ring: letters of "wesn"."""
        net = self.net
        nj, ni = net.block_shape
        room = dict(w=net.i0, e=ni - net.i0 - net.ni, s=net.j0, n=nj - net.j0 - net.nj)
        return "".join(k for k, v in room.items() if v == 1)

    def _block(self, cur, word, sweeps=1):
        key = (cur, word, sweeps)
        b = self._blocks.get(key)
        if b is None:
            from . import abi
            flags = sum(abi.BASIN_FLAG["ring_" + s] for s in self.ring_sides())
            b = self._blocks[key] = self.engine.flow_basin_block(self.net.dir, self.state[cur], self.state[1 - cur], self.label, self.hops,
                                                                 self.changed[word:word + 1], flags=flags, seed=self.seed, sweeps=sweeps)
        return b

    def begin(self):
        """The planes and noahmp_hip_flow_basin_init: one launch."""
        torch = self.torch
        shape, dev = self.net.block_shape, self.net.dir.device
        self.state = [torch.empty(shape, dtype=torch.int64, device=dev), torch.empty(shape, dtype=torch.int64, device=dev)]
        self.label = torch.empty(shape, dtype=torch.int32, device=dev)
        self.hops = torch.empty(shape, dtype=torch.int32, device=dev)
        self.changed = torch.zeros(self.cap + 1, dtype=torch.int32, device=dev)      # a word per pass, the last for resolve
        self.cur = self.passes = self.rounds = 0
        self._blocks = {}
        torch.cuda.current_stream().synchronize()
        self.engine.flow_basin_init(self._block(0, 0))
        self.engine.stream_sync()

    def contract(self, check=BASIN_CHECK, sweeps=None, tiled_calls=1):
        """noahmp_hip_flow_basin_jump until a pass moves no pointer or the cap of ceil(log2(ni*nj)) + 1 passes: `check` passes are enqueued in
        a row, each with a flag word of its own, and the host waits once per batch.  self.passes: the passes up to and including the first
        that changed nothing (a batch may have made up to check - 1 more: they change nothing either).  Returns True when it converged,
        False at the cap: caller-given directions hold a cycle, which resolve() marks.
        sweeps > 1: the first `tiled_calls` calls (None: all of them) are the tiled form with that many in-tile iterations; it moves every
        pointer at least as far as the pinned pass, so the cap holds."""
        torch = self.torch
        sweeps = BASIN_SWEEPS if sweeps is None else int(sweeps)
        self.changed.zero_()
        torch.cuda.current_stream().synchronize()
        done = 0
        while done < self.cap:
            n = min(int(check), self.cap - done)
            for k in range(done, done + n):
                self.engine.flow_basin_jump(self._block(self.cur, k, sweeps if tiled_calls is None or k < tiled_calls else 1))
                self.cur = 1 - self.cur
            self.engine.stream_sync()
            flags = self.changed[done:done + n].cpu().numpy()
            done += n
            still = np.nonzero(flags == 0)[0]
            if still.size:
                self.passes = done - n + int(still[0]) + 1
                return True
        self.passes = done
        return False

    def resolve(self):
        """One noahmp_hip_flow_basin_resolve on the contracted state; returns its flag (0: no label changed)."""
        torch = self.torch
        self.changed[self.cap:].zero_()
        torch.cuda.current_stream().synchronize()
        self.engine.flow_basin_resolve(self._block(self.cur, self.cap))
        self.engine.stream_sync()
        self.rounds += 1
        return int(self.changed[self.cap].item())

    def unresolved(self):
        """(cells of the tile labelled CYCLE, cells of the tile labelled PENDING)."""
        from . import abi
        t = self.net.tile_view(self.label)
        return int((t == abi.BASIN_CYCLE).sum().item()), int((t == abi.BASIN_PENDING).sum().item())

    def run(self, comm=None, geom=None, strict=True, check=BASIN_CHECK, sweeps=None, tiled_calls=1):
        """init, the doubling passes, and the resolve rounds: one without a comm; with a comm (the block's ring sides are owned by
        neighbour ranks) { comm.exchange_halo of label and hops, resolve, comm.agree_any(changed) } until no rank changed anything -- the
        largest number of ownership changes along a flow path, plus 2, rounds.  The passes stay local: ring cells are roots.  The int32
        planes travel as float32 views of the same words (every mover copies words).
        THE STREAM RULE of FlowNetwork.step holds: the exchange runs on torch's current stream, the launches on the engine's; each waits
        for the other.
        strict: a tile cell that ends as CYCLE or PENDING raises RuntimeError with the counts; strict=False leaves them marked.
        check, sweeps, tiled_calls: those of contract()."""
        torch = self.torch
        ring = self.ring_sides()
        if ring and comm is None:
            raise ValueError("a block with a ring needs the comm that fills it")
        self.begin()
        self.contract(check, sweeps, tiled_calls)
        if comm is None:
            self.resolve()
        else:
            views = [self.label.view(torch.float32), self.hops.view(torch.float32)]
            while True:
                self.engine.stream_sync()                                # label and hops are written before they travel
                comm.exchange_halo(views, geom)
                torch.cuda.current_stream().synchronize()                # ... and their ring has arrived before resolve reads it
                if not comm.agree_any(self.resolve() != 0):
                    break
        if strict:
            ncycle, npending = self.unresolved()
            if ncycle or npending:
                raise RuntimeError("Basins.run: %d cells of the tile end on a cycle of the directions and %d are pending (a ring nobody "
                                   "answered for, or a cycle across ranks)" % (ncycle, npending))
        return self.label

    # ---- what comes out
    def region_map(self):
        """int32 (nj, ni) in TILE order, the gauge's id or a negative word: the region_map of Regions (nregion = self.ngauge)."""
        return self.net.tile_view(self.label).contiguous().clone()

    def gauge_cells(self):
        """Block cell (j, i) of every gauge, int64 [ngauge, 2]; every id must mark exactly one cell."""
        out = np.full((self.ngauge, 2), -1, np.int64)
        if self.ngauge:
            seed = self.seed.cpu().numpy()
            jj, ii = np.nonzero(seed >= 0)
            ids = seed[jj, ii]
            if len(np.unique(ids)) != len(ids) or len(ids) != self.ngauge:
                raise ValueError("downstream_gauge needs ids 0..n-1 with one cell each")
            out[ids, 0], out[ids, 1] = jj, ii
        return out

    def downstream_gauge(self):
        """Per gauge the label of the cell below it: the next gauge downstream, or -1 (none: it drains to an outlet that is no gauge, has
        no downstream cell, or the cell below is unresolved).  int32 [ngauge], after run()."""
        cells = self.gauge_cells()
        down = _np_down(self._block_dir())
        label = self.label.cpu().numpy().ravel()
        out = np.full(self.ngauge, -1, np.int32)
        for g, (j, i) in enumerate(cells):
            d = down[j, i]
            if d >= 0 and label[d] >= 0:
                out[g] = label[d]
        return out

    def nested(self, series):
        """series[..., g]: sums over the INCREMENTAL area of gauge g (what Regions gives for region_map()).  Returns the sums over the whole
        basin above every gauge: every gauge's own value added to every gauge downstream of it."""
        dg = self.downstream_gauge()
        inc = np.array(series)
        assert inc.shape[-1] == self.ngauge
        out = inc.copy()
        for g in range(self.ngauge):
            d, n = dg[g], 0
            while d >= 0:
                out[..., d] += inc[..., g]
                d, n = dg[d], n + 1
                assert n <= self.ngauge, "downstream_gauge holds a cycle"
        return out


def _np_down(d):
    """down(c) of the header text over a block of directions: the flat index of the downstream cell, -1 where there is none."""
    nj, ni = d.shape
    k = np.where(d <= 8, d, 0).astype(np.int64)
    di = np.array((0, 1, 1, 0, -1, -1, -1, 0, 1))[k]
    dj = np.array((0, 0, 1, 1, 1, 0, -1, -1, -1))[k]
    jj, ii = np.meshgrid(np.arange(nj), np.arange(ni), indexing="ij")
    jn, i_n = jj + dj, ii + di
    ok = (k > 0) & (jn >= 0) & (jn < nj) & (i_n >= 0) & (i_n < ni)
    return np.where(ok, jn * ni + i_n, -1)


UPSTREAM_CHECK = 4                                                       # passes enqueued between two host waits


class Upstream:
    """The sum of a weight over the cells that drain through every cell of a FlowNetwork, itself included (noahmp_hip_flow_upstream_init /
    _pass): the drained cell count, or the contributing area, by doubling -- bit_length(L) + 1 passes for a longest flow path of L hops.

        u = Upstream(net)                        # a FlowNetwork with directions set; works on its block
        u.set_weight(Upstream.quantise(area, 100.0))     # uint32 words (here: units of 100 m2), block-shaped; None = 1 everywhere
        s = u.run()                              # decomposed: u.run(comm=comm, geom=geom); u.sum is the same plane
        u.channel_mask(5000)                     # bool: sum >= threshold
        u.passes, u.rounds, u.converged

    Words are uint64, kept in an int64 plane: a legal sum is below 2^63.  The adds are integer adds, so every schedule and every
    decomposition gives the same words; a real-valued weight is quantised ONCE, on the host side (quantise).  Not represented: float
    accumulation, metric flow length, Strahler order.
    A cycle of caller-given directions keeps the passes pushing up to the cap of ceil(log2(ni*nj)) + 1: run(strict=True) raises;
    strict=False sets converged = False and leaves the sums, exact wherever the cell is not on a cycle, for the caller to mask with the
    CYCLE labels of Basins."""

    def __init__(self, net):
        if net.dir is None:
            raise ValueError("the FlowNetwork has no directions: call set_terrain() or set_directions() first")
        self.net, self.engine, self.torch = net, net.engine, net.torch
        self.weight = None
        self._sum = self.pend = self.jump = self.changed = self.inflow = None
        self._ring = self._feeds = self._halo = None
        self.cur = self.passes = self.rounds = 0
        self.converged = False
        self.cap = (max(net.dir.numel(), 1) - 1).bit_length() + 1          # ceil(log2(ni*nj)) + 1
        self._blocks = {}

    # ---- the weight
    def set_weight(self, plane=None):
        """plane: uint32 words of the block -- an int32 device plane read as uint32, or a numpy uint32 / int32 array -- or None for 1
        at every cell.  Weights of ring cells are not read (their owner counts them)."""
        torch = self.torch
        if plane is not None:
            if isinstance(plane, np.ndarray):
                assert plane.dtype in (np.uint32, np.int32), "weights are uint32 words: Upstream.quantise makes them"
                plane = torch.from_numpy(np.ascontiguousarray(plane).view(np.int32))
            assert plane.dtype == torch.int32 and tuple(plane.shape) == self.net.block_shape, \
                "a weight plane is int32 (uint32 words) and has the shape of the block %s" % (self.net.block_shape,)
            plane = plane.to(self.net.dir.device).contiguous()
        self.weight = plane
        self._blocks = {}

    @staticmethod
    def quantise(field, step):
        """round(field / step) as uint32 words, made in float64, ties to even: a numpy array gives a numpy uint32 array, a tensor an int32
        tensor holding the same words.  Raises ValueError on a NaN, a negative value or a quotient above 2^32 - 1."""
        is_np = isinstance(field, np.ndarray) or not hasattr(field, "cpu")
        q = np.rint(np.asarray(field if is_np else field.cpu().numpy(), np.float64) / float(step))
        if np.isnan(q).any():
            raise ValueError("Upstream.quantise: the field holds a NaN (or step is 0 or NaN)")
        if (q < 0).any():
            raise ValueError("Upstream.quantise: negative values cannot be weights")
        if (q > 4294967295.0).any():
            raise ValueError("Upstream.quantise: a value above (2^32 - 1) * step; choose a larger step")
        w = q.astype(np.uint32)
        if is_np:
            return w
        import torch
        return torch.from_numpy(w.view(np.int32)).to(field.device)

    # ---- the calls
    def ring_sides(self):
        """The sides of the block that are a ring: letters of "wesn"."""
        net = self.net
        nj, ni = net.block_shape
        room = dict(w=net.i0, e=ni - net.i0 - net.ni, s=net.j0, n=nj - net.j0 - net.nj)
        return "".join(k for k, v in room.items() if v == 1)

    def _block(self, cur, word):
        key = (cur, word)
        b = self._blocks.get(key)
        if b is None:
            from . import abi
            flags = sum(abi.UPSTREAM_FLAG["ring_" + s] for s in self.ring_sides())
            b = self._blocks[key] = self.engine.flow_upstream_block(self.net.dir, self._sum, self.pend[cur], self.pend[1 - cur], self.jump[cur],
                                                                    self.jump[1 - cur], self.changed[word:word + 1], flags=flags,
                                                                    weight=self.weight, inflow=self.inflow)
        return b

    def _planes(self):
        torch = self.torch
        shape, dev = self.net.block_shape, self.net.dir.device
        i64 = lambda: torch.empty(shape, dtype=torch.int64, device=dev)      # noqa: E731
        i32 = lambda: torch.empty(shape, dtype=torch.int32, device=dev)      # noqa: E731
        self._sum, self.pend, self.jump = i64(), [i64(), i64()], [i32(), i32()]
        self.changed = torch.zeros(self.cap, dtype=torch.int32, device=dev)      # a word per pass
        sides = self.ring_sides()
        self.inflow = self._ring = self._feeds = None
        if sides:
            ring = np.zeros(shape, bool)
            for s, sl in (("w", np.s_[:, 0]), ("e", np.s_[:, -1]), ("s", np.s_[0, :]), ("n", np.s_[-1, :])):
                if s in sides:
                    ring[sl] = True
            self._ring = torch.from_numpy(ring).to(dev)
            self.inflow = torch.zeros(shape, dtype=torch.int64, device=dev)
        self._blocks = {}

    def begin(self):
        """The planes (made once, kept with the inflow they hold) and noahmp_hip_flow_upstream_init: one launch."""
        torch = self.torch
        if self._sum is None or tuple(self._sum.shape) != self.net.block_shape:
            self._planes()
        self.cur = self.passes = 0
        self.converged = False
        torch.cuda.current_stream().synchronize()
        self.engine.flow_upstream_init(self._block(0, 0))
        self.engine.stream_sync()
        if self._ring is not None and self._feeds is None:               # the ring cells that push into the tile: a function of dir alone
            self._feeds = self._ring & (self.jump[0] >= 0)

    def accumulate(self, check=UPSTREAM_CHECK):
        """noahmp_hip_flow_upstream_pass until a pass pushes nothing or the cap of ceil(log2(ni*nj)) + 1 passes: `check` passes are
        enqueued in a row, each with a flag word of its own, and the host waits once per batch.  self.passes: the passes up to and
        including the first in which nobody pushed (a batch may have made up to check - 1 more: they change no word of sum).  Returns
        self.converged: True, or False at the cap -- caller-given directions hold a cycle."""
        torch = self.torch
        self.changed.zero_()
        torch.cuda.current_stream().synchronize()
        done = 0
        while done < self.cap:
            n = min(int(check), self.cap - done)
            for k in range(done, done + n):
                self.engine.flow_upstream_pass(self._block(self.cur, k))
                self.cur = 1 - self.cur
            self.engine.stream_sync()
            flags = self.changed[done:done + n].cpu().numpy()
            done += n
            still = np.nonzero(flags == 0)[0]
            if still.size:
                self.passes = done - n + int(still[0]) + 1
                self.converged = True
                return True
        self.passes = done
        self.converged = False
        return False

    def halo_planes(self):
        """sum as two float32 views of int32 planes, the low and the high words: what travels in a ring exchange (every mover copies
        words).  The same two planes every time."""
        torch = self.torch
        words = self._sum.view(torch.int32).view(self._sum.shape + (2,))
        if self._halo is None:
            self._halo = [torch.empty(self._sum.shape, dtype=torch.int32, device=self._sum.device) for _ in range(2)]
        for k in range(2):
            self._halo[k].copy_(words[..., k])
        return [h.view(torch.float32) for h in self._halo]

    def absorb_ring(self):
        """After the exchange of halo_planes(): the ring cells' words become inflow.  Returns True when a ring cell that pushes into the
        tile holds another word than before (the others change nothing here)."""
        torch = self.torch
        got = torch.stack(self._halo, dim=-1).contiguous().view(torch.int64)[..., 0]
        new = torch.where(self._ring, got, torch.zeros_like(got))
        moved = bool(((new != self.inflow) & self._feeds).any().item())
        self.inflow.copy_(new)
        return moved

    def run(self, comm=None, geom=None, strict=True, check=UPSTREAM_CHECK, max_rounds=None):
        """init and the passes; returns sum.  With a comm (the block's ring sides are owned by neighbour ranks) ROUNDS: round 0 with
        inflow = 0, then { comm.exchange_halo of the low and the high words of sum; inflow = the ring; init and the passes again where the
        ring changed; comm.agree_any(ring changed) } until no rank's ring changed.  The ring values only grow; a flow path that changes
        its owner k times is summed after round k, so the loop makes at most (the largest k) + 2 rounds, the last of which only finds the
        rings unchanged.  A cycle ACROSS ranks grows for ever: max_rounds (the same on every rank; None = no limit) raises when reached --
        Basins.run marks such cells PENDING beforehand.
        THE STREAM RULE of FlowNetwork.step holds: the exchange runs on torch's current stream, the launches on the engine's; each waits
        for the other.
        strict: passes that still push at the cap (a cycle of the directions inside the block) raise RuntimeError; strict=False leaves
        converged = False and the sums as they are."""
        torch = self.torch
        if self.ring_sides() and comm is None:
            raise ValueError("a block with a ring needs the comm that fills it")
        if self.inflow is not None:
            self.inflow.zero_()
        self.begin()
        ok = self.accumulate(check)
        self.rounds = 1
        while comm is not None:
            if max_rounds is not None and self.rounds >= int(max_rounds):
                raise RuntimeError("Upstream.run: the ring still changes on some rank after %d rounds: a cycle across ranks?" % self.rounds)
            self.engine.stream_sync()                                    # sum is written before it travels
            planes = self.halo_planes()
            comm.exchange_halo(planes, geom)
            torch.cuda.current_stream().synchronize()                    # ... and its ring has arrived before init reads it
            moved = self.absorb_ring()
            if moved:
                self.begin()
                ok = self.accumulate(check) and ok
            self.rounds += 1
            if not comm.agree_any(moved):
                break
        if self.inflow is not None:                                      # ring cells show their owner's latest word
            self._sum.copy_(torch.where(self._ring, self.inflow, self._sum))
            torch.cuda.current_stream().synchronize()
        self.converged = ok
        if strict and not ok:
            raise RuntimeError("Upstream.run: cells still push after the cap of %d passes: the directions hold a cycle (strict=False keeps "
                               "the sums; Basins marks the cells)" % self.cap)
        return self._sum

    # ---- what comes out
    @property
    def sum(self):
        """int64 block plane of uint64 words: the sum over every cell's upstream area, itself included; ring cells hold their inflow."""
        return self._sum

    def cells(self, **kw):
        """run() with unit weights: the number of cells that drain through every cell (FlowNetwork.upstream_cells in 64 bits)."""
        self.set_weight(None)
        return self.run(**kw)

    def channel_mask(self, threshold):
        """bool block plane: sum >= threshold (a channel begins where enough area drains through a cell)."""
        return self._sum >= int(threshold)

    @staticmethod
    def mean_of(field_sum, weight_sum):
        """The upstream mean of a field: the sums of Upstream runs with weights quantise(field * w, .) and quantise(w, .), divided in
        float64 (times the ratio of the two steps, which is the caller's); NaN where weight_sum is 0."""
        import torch
        f, w = field_sum.to(torch.float64), weight_sum.to(torch.float64)
        return f / w.masked_fill(w == 0, float("nan"))


class ChannelFlow:
    """Kinematic-wave routing with Manning friction on a FlowNetwork (noahmp_hip_flow_channel / noahmp_hip_route_kinematic): where
    FlowNetwork.step releases a constant fraction, a cell releases Manning's discharge of a rectangular section whose depth follows from
    what the cell holds, at most all of it.

        ch = ChannelFlow(net)                                    # a FlowNetwork with directions set; works on net.storage, net.out, net.cur
        area = up.sum.double() * step                            # Upstream: the contributing area [m2]
        w = ChannelFlow.width_from_area(area, 2.0, 0.4, 5e6, net.dir, dx, dy)
        ch.set_geometry(w, 0.05)                                 # once: bed slopes from net.filled, one launch
        engine.noahmplsm(store, ...); ch.step(store, dt, nsub=2) # per step, INSTEAD of net.step
        ch.courant(), ch.capped(); ch.reset_diag()               # 5/3 * the largest vel*dt/length since the reset; keep it near or below 1
        net.discharge(), net.state_dict(), Regions / probes over net.out: as with net.step

    Not represented: diffusive wave and backwater, trapezoidal sections, losses, an implicit solve (lakes: class Lakes); nsub is the
    caller's choice, read from courant()."""

    def __init__(self, net):
        if net.dir is None:
            raise ValueError("the FlowNetwork has no directions: call set_terrain() or set_directions() first")
        self.net, self.engine, self.torch = net, net.engine, net.torch
        self.width = self.manning = self.length = self.conv = None
        self.smin = None
        self._depth = None
        self.diag = None                                                 # two device words: the bits of the largest cr, the capped cells

    def _plane(self, plane, name, ring):
        """A number, a plane of the block or a plane of the tile (its ring cells, which no call computes, get `ring`)."""
        torch, net = self.torch, self.net
        dev = net.dir.device
        if not torch.is_tensor(plane):
            return torch.full(net.block_shape, float(plane), dtype=torch.float32, device=dev)
        plane = plane.to(torch.float32)
        if tuple(plane.shape) == (net.nj, net.ni) and net.block_shape != (net.nj, net.ni):
            full = torch.full(net.block_shape, float(ring), dtype=torch.float32, device=dev)
            net.tile_view(full).copy_(plane)
            plane = full
        assert tuple(plane.shape) == net.block_shape, "%s: a number, a plane of the block %s or of the tile" % (name, net.block_shape)
        return plane.contiguous()

    def _cut(self, plane, name):
        """A plane of the block as it is; a plane of the window given to set_terrain / set_directions (same origin) cut to the block."""
        net = self.net
        plane = plane.to(self.torch.float32)
        if tuple(plane.shape) == net.block_shape:
            return plane.contiguous()
        if net.window_shape is not None and tuple(plane.shape) == net.window_shape:
            return plane[net.window_block].contiguous()
        raise ValueError("%s: a plane of the block %s or of the window %s" % (name, net.block_shape, net.window_shape))

    def set_geometry(self, width, manning, smin=1e-4, height=None, slope=None):
        """width [m] and manning [s m^-1/3]: numbers, or float32 device planes of the block or the tile.  The bed slope comes from
        `slope` (a plane), else from `height`, else from net.filled: the drop to the downstream cell over the distance, at least smin.
        A height or slope plane is one of the block, or one of the window given to set_terrain with the same origin.  One launch; length
        and conv are kept.  A cell with manning not > 0 holds its water."""
        torch, net = self.torch, self.net
        if net.dx is None:
            raise ValueError("set_geometry needs the dx, dy of set_terrain / set_directions")
        if slope is None and height is None:
            height = net.filled
        if slope is None and height is None:
            raise ValueError("no bed slope: the network has no filled surface (set_terrain(fill=...) / set_terrain_filled); give height= or slope=")
        self.width = self._plane(width, "width", 1.0)
        assert bool((self.width > 0).all().item()), "width must be > 0 everywhere"
        self.manning = self._plane(manning, "manning", 0.0)
        h = s = None
        if slope is not None:
            s = self._cut(slope, "slope")
        else:
            h = self._cut(height, "height")
        dev = net.dir.device
        self.length = torch.empty(net.block_shape, dtype=torch.float32, device=dev)
        self.conv = torch.empty(net.block_shape, dtype=torch.float32, device=dev)
        self._depth = torch.zeros(net.block_shape, dtype=torch.float32, device=dev)
        self.diag = torch.zeros(2, dtype=torch.int32, device=dev)
        self.smin = float(smin)
        torch.cuda.current_stream().synchronize()
        self.engine.flow_channel(self.engine.flow_channel_block(net.dir, self.manning, self.length, self.conv, net.dx, net.dy, self.smin,
                                                                height=h, slope=s))
        self.engine.stream_sync()
        if net.held is not None:                                         # the members of Lakes.set_lakes hold their water
            self.conv.masked_fill_(net.held, 0.0)
            torch.cuda.current_stream().synchronize()

    @staticmethod
    def width_from_area(area_m2, a, b, threshold_m2, dir, dx, dy):
        """The width of every cell's rectangular section [m], float32, numpy in numpy out, tensor in tensor out.  Where area_m2 >=
        threshold_m2 (a channel cell) the hydraulic-geometry width a * area^b, made in float64 on the host and rounded once; elsewhere
        (a hillslope cell: sheet flow) the cell's width ACROSS its direction: dy for E / W, dx for N / S, dx*dy/diagonal for the diagonals,
        dx where there is no direction.  area_m2: Upstream.sum() times the quantisation step.  dir: the directions of the same cells."""
        is_np = isinstance(area_m2, np.ndarray)
        area = np.asarray(area_m2 if is_np else area_m2.cpu().numpy(), np.float64)
        d = np.asarray(dir if isinstance(dir, np.ndarray) else dir.cpu().numpy())
        assert d.shape == area.shape
        dx, dy = float(dx), float(dy)
        diag = math.sqrt(dx * dx + dy * dy)
        across = np.where((d == 0) | (d > 8), dx, np.where(d % 2 == 0, dx * dy / diag, np.where((d == 3) | (d == 7), dx, dy)))
        with np.errstate(all="ignore"):
            w = np.where(area >= float(threshold_m2), float(a) * np.power(area, float(b)), across).astype(np.float32)
        if is_np:
            return w
        import torch
        return torch.from_numpy(w).to(area_m2.device)

    def step(self, store, dt, fields=("runsfxy", "runsbxy"), nsub=1, comm=None, geom=None, stream=None):
        """One model step of routing after Engine.noahmplsm, INSTEAD of FlowNetwork.step: nsub launches with dt/nsub and scale =
        dt*1e-3/nsub on the network's storage and out planes; the stream rule and the exchange of out are those of FlowNetwork.step.
        depth and the two diag words are written by every launch; diag accumulates until reset_diag()."""
        net = self.net
        if self.conv is None:
            raise ValueError("call set_geometry() first")
        ra, rb = net._runoff_planes(store, fields, nsub)
        scale = float(np.float32(dt) * np.float32(1e-3)) / nsub
        dts = float(dt) / nsub

        def launch(out_old, out_new):
            b = self.engine.route_kinematic_block(net.inmask, net.col_index, net.area, self.width, self.length, self.conv, net.storage,
                                                  out_old, out_new, ra, rb, scale, dts, depth=self._depth, diag=self.diag)
            self.engine.route_kinematic(b, net.ncell, stream=stream)

        net._sub_steps(launch, dt, nsub, comm, geom, stream)

    def follow(self, store):
        """After Engine.sort_store(store): FlowNetwork.follow -- only col_index is rewritten."""
        self.net.follow(store)

    def depth(self):
        """The water depth h [m] of the last launch, a plane of the block (0 where a cell held no water or has no conveyance)."""
        return self._depth

    def reset_diag(self):
        """Zero the two diag words (the calls never do)."""
        self.torch.cuda.current_stream().synchronize()
        self.engine.stream_sync()
        self.diag.zero_()
        self.torch.cuda.current_stream().synchronize()

    def _diag_words(self):
        self.engine.stream_sync()                                        # the one host wait
        w = self.diag.cpu().numpy().view(np.uint32)
        return int(w[0]), int(w[1])

    def courant(self, comm=None):
        """5/3 * the largest vel*dt/length of any owned cell in any launch since reset_diag(): the Courant number of the kinematic
        celerity on a wide section.  NaN when a cell's was NaN.  With a comm the maximum over the ranks.  One host wait."""
        bits = self._diag_words()[0]
        if comm is not None:
            bits = int(comm.reduce_max(bits))                            # uint32 bits are exact in float64 and monotone like the floats
        return 5.0 / 3.0 * float(np.array([bits], np.uint32).view(np.float32)[0])

    def capped(self, comm=None):
        """The number of (cell, launch) pairs since reset_diag() in which a cell released all it held (mod 2^32 per rank); with a comm
        the sum over the ranks.  One host wait."""
        n = self._diag_words()[1]
        return int(comm.reduce_sum(n)) if comm is not None else n


class DiffusiveFlow(ChannelFlow):
    """Diffusive-wave routing on a FlowNetwork: backwater (noahmp_hip_flow_drop / noahmp_hip_route_diffusive).  Where ChannelFlow
    releases Manning's discharge at the bed slope, the friction slope here is the slope of the water surface to the downstream cell: a
    cell whose surface is not above its downstream cell's releases nothing, so water pools behind an adverse bed, crosses flats and
    filled depressions by its own surface slope, and backs up in front of a lake (Lakes.set_datum).

        df = DiffusiveFlow(net)
        df.set_geometry(w, 0.05, limit=0.5)                      # once: ChannelFlow's launch, then the bed drops; two depth planes
        engine.noahmplsm(store, ...); df.step(store, dt, nsub=4) # per step, INSTEAD of net.step / ch.step
        df.courant(), df.capped(), df.limited(), df.blocked(); df.reset_diag()
        df.depth(); df.state_dict() / df.load_state_dict()       # the depth plane is read by the next call: restart state

    Choosing nsub: keep courant() near or below 1 as for ChannelFlow; limited() counts the (cell, launch) pairs in which the limiter
    cut a release -- a few near level pools are the scheme at work, many on a slope say that nsub is too small.
    df.report = False runs the launches without the diag words: where most workgroups hold a blocked cell their atomics to one word cost
    more than the launch itself (profiles/diffusive_bench.md); the planes have the same bits either way.
    Not represented: reverse flow against the fixed directions, dynamic directions, an inertial or implicit formulation, trapezoidal
    sections, losses; nsub is the caller's choice."""

    def __init__(self, net):
        super().__init__(net)
        self.drop = self.bed = None
        self.limit = 0.5
        self.report = True                                               # False: the launches get no diag (every workgroup that reports sends atomics)
        self._d = None                                                   # two depth planes, ping-ponged in step with net.out

    def set_geometry(self, width, manning, smin=1e-4, height=None, slope=None, limit=0.5):
        """ChannelFlow.set_geometry (length and conv: the outlets release at normal depth), then the bed drop of every cell from the
        same height or slope plane (one more launch).  With heights (given, or net.filled) the bed is kept as `bed`: Lakes.set_datum
        needs it.  limit: the flow limiter, finite and > 0."""
        torch, net = self.torch, self.net
        if not (math.isfinite(float(limit)) and float(limit) > 0):
            raise ValueError("limit must be finite and > 0")
        if slope is None and height is None:
            height = net.filled
        super().set_geometry(width, manning, smin=smin, height=height, slope=slope)
        h = s = None
        if slope is not None:
            s = self._cut(slope, "slope")
        else:
            h = self._cut(height, "height")
        dev = net.dir.device
        self.limit = float(limit)
        self.bed = h
        self.drop = torch.empty(net.block_shape, dtype=torch.float32, device=dev)
        self._d = [torch.zeros(net.block_shape, dtype=torch.float32, device=dev) for _ in range(2)]
        self._depth = None
        self.diag = torch.zeros(4, dtype=torch.int32, device=dev)        # the bits of the largest cr; capped, limited, blocked cells
        torch.cuda.current_stream().synchronize()
        self.engine.flow_drop(self.engine.flow_drop_block(net.dir, self.drop, net.dx, net.dy, height=h, slope=s))
        self.engine.stream_sync()

    def step(self, store, dt, fields=("runsfxy", "runsbxy"), nsub=1, comm=None, geom=None, stream=None):
        """One model step of routing after Engine.noahmplsm, INSTEAD of FlowNetwork.step / ChannelFlow.step: nsub launches with dt/nsub
        and scale = dt*1e-3/nsub.  The two depth planes ping-pong in step with the network's out planes, and with a comm the new depth
        plane travels with out in the same exchange: its ring has arrived before the next launch (the stream rule of
        FlowNetwork.step).  The four diag words accumulate until reset_diag()."""
        net = self.net
        if self.drop is None:
            raise ValueError("call set_geometry() first")
        ra, rb = net._runoff_planes(store, fields, nsub)
        scale = float(np.float32(dt) * np.float32(1e-3)) / nsub
        dts = float(dt) / nsub

        def launch(out_old, out_new):
            b = self.engine.route_diffusive_block(net.inmask, net.col_index, net.dir, net.area, self.width, self.length, self.conv,
                                                  self.manning, self.drop, net.storage, out_old, out_new, ra, rb, self._d[net.cur],
                                                  self._d[1 - net.cur], scale, dts, limit=self.limit, diag=self.diag if self.report else None)
            self.engine.route_diffusive(b, net.ncell, stream=stream)    # net.cur flips after the launch: _d[net.cur] is then the new plane

        net._sub_steps(launch, dt, nsub, comm, geom, stream, also=lambda new: [self._d[new]])

    def depth(self):
        """The water depth [m] at the end of the last launch, a plane of the block: what the next launch reads as its neighbours'."""
        return self._d[self.net.cur]

    def _diag_words(self):
        self.engine.stream_sync()                                        # the one host wait
        return tuple(int(v) for v in self.diag.cpu().numpy().view(np.uint32))

    def capped(self, comm=None):
        """The (cell, launch) pairs since reset_diag() in which a cell released all it held and the limiter did not cut it."""
        return super().capped(comm)

    def limited(self, comm=None):
        """The (cell, launch) pairs since reset_diag() in which the limiter cut a release (mod 2^32 per rank; with a comm the sum)."""
        n = self._diag_words()[2]
        return int(comm.reduce_sum(n)) if comm is not None else n

    def blocked(self, comm=None):
        """The (cell, launch) pairs since reset_diag() in which a cell with water released nothing because its surface did not stand
        above its downstream cell's (mod 2^32 per rank; with a comm the sum)."""
        n = self._diag_words()[3]
        return int(comm.reduce_sum(n)) if comm is not None else n

    def state_dict(self):
        """The restart state: the network's (storage, the current out plane) and the current depth plane (copies)."""
        return dict(self.net.state_dict(), depth=self.depth().clone())

    def load_state_dict(self, state):
        self.net.load_state_dict(state)
        self.depth().copy_(state["depth"])
        self.torch.cuda.current_stream().synchronize()


LAKE_PARAMS = ("area", "weir_h", "weir_c", "weir_l", "orifice_h", "orifice_c", "orifice_a")
LAKE_WAVE = 64                                                           # every lake's entries are padded to whole waves


class Lakes:
    """Lakes on a FlowNetwork or a ChannelFlow: level-pool storage and outflow (noahmp_hip_lake_take / noahmp_hip_lake_release).

        lakes = Lakes(ch)                                        # or Lakes(net); quantum = 2**-10 m3
        lake_id, outlet_ij, area = Lakes.from_fill(raw, filled, upstream_sum, 0.5, cell_area=dx * dy)      # once, host, global planes
        lakes.set_lakes(lake_id_tile, params, outlet_ij, tile_origin=(i0, j0))
        lakes.attach()                                           # after every launch of net.step / ch.step: take, (sum over ranks,) release
        ch.step(store, dt, nsub=2)
        lakes.level(), lakes.outflow(), lakes.volume_m3(), lakes.emptied()
        lakes.set_datum(Lakes.datum_from_fill(raw, filled, lake_id))     # on a DiffusiveFlow: the lake's stage backs up its inflowing channels

    The members of a lake hold everything that reaches them (release and conv are zeroed there, also when set_release, set_velocity or
    set_geometry is called later); after each launch the whole quanta of their storage move to the lake's volume word and the level-pool
    outflow of a weir and an orifice is written to out at the outlet, where the next launch's gather picks it up.  Water is conserved
    exactly.  Not built: evaporation and precipitation on the lake surface, hypsometric (level-dependent) area, an implicit or
    Runge-Kutta level-pool solve, reservoir operating rules, backwater into inflowing channels."""

    def __init__(self, flow, quantum=2.0 ** -10):
        self.ch = flow if isinstance(flow, ChannelFlow) else None
        self.net = flow.net if self.ch is not None else flow
        if self.net.dir is None:
            raise ValueError("the FlowNetwork has no directions: call set_terrain() or set_directions() first")
        self.engine, self.torch = self.net.engine, self.net.torch
        self.quantum = float(quantum)
        m, e = math.frexp(self.quantum)
        if m != 0.5 or not -40 <= e - 1 <= 20:
            raise ValueError("quantum must be an exact power of two in [2^-40, 2^20]")
        self.nlake = 0
        self.member_cell = self.member_lake = self.outlet_cell = None
        self.volume = self.inflow = self.params = None
        self._level = self._outflow = self.diag = None
        self._blocks = {}
        self.datum = None                                                # float64 per lake: the height of level 0 in the bed's datum
        self._dblocks = {}

    # ---- the host helper
    @staticmethod
    def datum_from_fill(raw, filled, lake_id):
        """The datum of every lake of Lakes.from_fill, float64 numpy on the host, on GLOBAL planes: min(filled over the members) -
        mean(filled - raw over the members).  With it a lake holding area * its mean depth has its surface at the spill level."""
        raw, filled, lid = np.asarray(raw, np.float64), np.asarray(filled, np.float64), np.asarray(lake_id)
        assert raw.shape == filled.shape == lid.shape
        nlake = int(lid.max()) if lid.size else 0
        m = lid > 0
        l = lid[m].astype(np.int64) - 1
        count = np.bincount(l, minlength=nlake).astype(np.float64)
        spill = np.full(nlake, np.inf)
        np.minimum.at(spill, l, filled[m])
        mean = np.bincount(l, weights=(filled - raw)[m], minlength=nlake) / np.maximum(count, 1.0)
        return np.where(count > 0, spill - mean, 0.0)

    def set_datum(self, datum):
        """The height of every lake's level 0 [m, in the datum of the bed heights]: a number or nlake values.  With a DiffusiveFlow that
        has a bed, every launch is then followed by noahmp_hip_lake_depth after the release: the members' depth becomes the lake's
        surface above their bed, and a channel that drains into the lake backs up until its own surface is higher.  None: off."""
        self._wait()
        self._dblocks = {}
        if datum is None:
            self.datum = None
            return
        d = np.ascontiguousarray(np.broadcast_to(np.asarray(datum, np.float64), (self.nlake,)))
        self.datum = self.torch.from_numpy(d.copy()).to(self.net.dir.device)
        self.torch.cuda.current_stream().synchronize()

    @staticmethod
    def from_fill(raw, filled, upstream_sum, min_depth, min_cells=1, cell_area=1.0):
        """Lakes of a filled terrain, numpy, once per terrain on GLOBAL (nj, ni) planes: the 8-connected components of
        filled - raw >= min_depth with at least min_cells cells, numbered 1.. by their smallest cell index ascending.  The outlet of a
        lake is its member with the largest upstream_sum (ties: the smallest cell index); area = cells * cell_area.
        Returns (lake_id int32 plane, outlet_ij int64 (nlake, 2) of global (i, j), area float64 (nlake,))."""
        raw, filled, up = np.asarray(raw, np.float64), np.asarray(filled, np.float64), np.asarray(upstream_sum)
        assert raw.ndim == 2 and raw.shape == filled.shape == up.shape
        nj, ni = raw.shape
        with np.errstate(invalid="ignore"):
            mask = (filled - raw) >= float(min_depth)
        big = nj * ni
        cell = np.arange(big, dtype=np.int64).reshape(nj, ni)
        label = np.where(mask, cell, big)
        pad = np.full((nj + 2, ni + 2), big, np.int64)
        while True:                                                      # the smallest cell index of every component: min over the
            pad[1:-1, 1:-1] = label                                      # neighbours, then pointer jumping through the labels
            new = label
            for dj in (0, 1, 2):
                for di in (0, 1, 2):
                    new = np.minimum(new, pad[dj:dj + nj, di:di + ni])
            new = np.where(mask, new, big)
            flat = np.append(new.ravel(), big)
            for _ in range(64):
                nxt = flat[flat]
                if (nxt == flat).all():
                    break
                flat = nxt
            new = flat[:-1].reshape(nj, ni)
            if (new == label).all():
                break
            label = new
        roots, inverse, counts = np.unique(label[mask], return_inverse=True, return_counts=True)
        keep = counts >= int(min_cells)
        number = np.zeros(roots.size, np.int32)
        number[keep] = np.arange(1, int(keep.sum()) + 1, dtype=np.int32)
        lake_id = np.zeros((nj, ni), np.int32)
        lake_id[mask] = number[inverse]
        nlake = int(keep.sum())
        member = lake_id > 0
        mc, ml = cell[member], lake_id[member].astype(np.int64) - 1
        mu = up[member].astype(np.int64) if up.dtype.kind in "iu" else up[member].astype(np.float64)
        order = np.lexsort((-mc, mu, ml))                               # the last entry of every lake: the largest sum, then the smallest cell
        last = np.r_[np.nonzero(np.diff(ml[order]))[0], order.size - 1] if order.size else np.zeros(0, np.int64)
        oc = mc[order][last]
        outlet_ij = np.stack([oc % ni, oc // ni], axis=1).astype(np.int64).reshape(nlake, 2)
        area = counts[keep].astype(np.float64) * float(cell_area)
        return lake_id, outlet_ij, area

    # ---- the lakes of this tile
    def set_lakes(self, lake_id, params, outlet_ij, tile_origin=(0, 0)):
        """lake_id: int32 plane of the TILE, 0 = none, 1..nlake = global ids, the same on all ranks.  params: a dict of the seven float64
        arrays of length nlake (LAKE_PARAMS).  outlet_ij: the global (i, j) of every lake's outlet.  tile_origin: the global (i, j) of the
        tile's cell (0, 0).  Builds the member list of the owned members, sorted by lake, every lake padded to whole waves with -1; the
        outlet_cell of a lake whose outlet is not on this tile is -1.  Zeroes release (and conv) at the members."""
        torch, net = self.torch, self.net
        dev = net.dir.device
        lid = np.asarray(lake_id.cpu().numpy() if torch.is_tensor(lake_id) else lake_id).astype(np.int64)
        if lid.shape != (net.nj, net.ni):
            raise ValueError("lake_id is a plane of the tile (%d, %d)" % (net.nj, net.ni))
        par = {k: np.ascontiguousarray(params[k], np.float64).ravel() for k in LAKE_PARAMS}
        nlake = par["area"].size
        out_ij = np.asarray(outlet_ij, np.int64)
        if any(v.size != nlake for v in par.values()) or out_ij.size != 2 * nlake or lid.min() < 0 or lid.max() > nlake:
            raise ValueError("params and outlet_ij have one entry per lake, lake_id holds 0 .. nlake")
        out_ij = out_ij.reshape(nlake, 2)
        nj_b, ni_b = net.block_shape
        d = net.dir.cpu().numpy()
        from . import abi
        outlet_cell = np.full(nlake, -1, np.int32)
        for l in range(nlake):
            i, j = int(out_ij[l, 0]) - int(tile_origin[0]), int(out_ij[l, 1]) - int(tile_origin[1])
            if not (0 <= i < net.ni and 0 <= j < net.nj):
                continue                                                 # another rank owns it
            if lid[j, i] != l + 1:
                raise ValueError("the outlet (%d, %d) of lake %d is not a member of it" % (out_ij[l, 0], out_ij[l, 1], l + 1))
            k = int(d[j + net.j0, i + net.i0])
            if 1 <= k <= 8:
                i2, j2 = i + abi.FLOW_DI[k - 1], j + abi.FLOW_DJ[k - 1]
                if 0 <= i2 < net.ni and 0 <= j2 < net.nj and lid[j2, i2] == l + 1:
                    raise ValueError("the outlet (%d, %d) of lake %d drains into a member of the same lake" % (out_ij[l, 0], out_ij[l, 1], l + 1))
            outlet_cell[l] = (j + net.j0) * ni_b + (i + net.i0)
        jj, ii = np.nonzero(lid > 0)
        lake = lid[jj, ii] - 1
        cellb = (jj + net.j0) * ni_b + (ii + net.i0)
        order = np.lexsort((cellb, lake))
        lake, cellb = lake[order], cellb[order]
        counts = np.bincount(lake, minlength=nlake) if lake.size else np.zeros(nlake, np.int64)
        padded = (counts + LAKE_WAVE - 1) // LAKE_WAVE * LAKE_WAVE
        start = np.concatenate([[0], np.cumsum(padded)])[:-1] if nlake else np.zeros(0, np.int64)
        mcell = np.full(int(padded.sum()), -1, np.int32)
        mlake = np.full(int(padded.sum()), -1, np.int32)
        if lake.size:
            first = np.concatenate([[0], np.cumsum(counts)])[:-1]
            pos = start[lake] + (np.arange(lake.size) - first[lake])
            mcell[pos], mlake[pos] = cellb, lake
        held = np.zeros((nj_b, ni_b), bool)
        held[jj + net.j0, ii + net.i0] = True
        self.nlake = nlake
        self.member_cell, self.member_lake = torch.from_numpy(mcell).to(dev), torch.from_numpy(mlake).to(dev)
        self.outlet_cell = torch.from_numpy(outlet_cell).to(dev)
        self.params = {k: torch.from_numpy(v.copy()).to(dev) for k, v in par.items()}
        self.volume = torch.zeros(nlake, dtype=torch.int64, device=dev)
        self.inflow = torch.zeros(nlake, dtype=torch.int64, device=dev)
        self._level = torch.zeros(nlake, dtype=torch.float64, device=dev)
        self._outflow = torch.zeros(nlake, dtype=torch.float32, device=dev)
        self.diag = torch.zeros(1, dtype=torch.int32, device=dev)
        self._blocks = {}
        self._dblocks = {}
        self.datum = None
        net.held = torch.from_numpy(held).to(dev)
        net._hold()
        if self.ch is not None and self.ch.conv is not None:
            self.ch.conv.masked_fill_(net.held, 0.0)
        torch.cuda.current_stream().synchronize()

    # ---- the hook
    def _after_launch(self, out_new, dt_sub, comm, stream):
        net = self.net
        if self.nlake == 0:
            return
        key = (out_new.data_ptr(), float(dt_sub), net.storage.data_ptr())
        b = self._blocks.get(key)
        if b is None:
            b = self._blocks[key] = (
                self.engine.lake_take_block(self.member_cell, self.member_lake, net.storage, self.inflow, self.quantum),
                self.engine.lake_release_block(self.volume, self.inflow, self.params, self.outlet_cell, out_new, self.quantum, dt_sub,
                                               level=self._level, outflow=self._outflow, diag=self.diag))
        self.engine.lake_take(b[0], stream=stream)
        if comm is not None:
            self.engine.stream_sync(stream)                              # the partial words are written before they are summed
            words = comm.reduce_sum_words(self.inflow)
            if words is not self.inflow:
                self.inflow.copy_(words)
            self.torch.cuda.current_stream().synchronize()               # ... and the sums have arrived before the release reads them
        self.engine.lake_release(b[1], stream=stream)
        if self.datum is not None and isinstance(self.ch, DiffusiveFlow) and self.ch.bed is not None:
            depth = self.ch.depth()                                      # net.cur has flipped: the plane this launch wrote
            key = (depth.data_ptr(), self.ch.bed.data_ptr())
            d = self._dblocks.get(key)
            if d is None:
                d = self._dblocks[key] = self.engine.lake_depth_block(self.member_cell, self.member_lake, self.volume, self.params["area"],
                                                                      self.datum, self.ch.bed, depth, self.quantum)
            self.engine.lake_depth(d, stream=stream)                     # the lake's stage is what the inflowing channels see next

    def attach(self):
        """Put the hook into net.after_launch: after every launch of FlowNetwork.step / ChannelFlow.step, before out travels."""
        if self.volume is None:
            raise ValueError("call set_lakes() first")
        if self._after_launch not in self.net.after_launch:
            self.net.after_launch.append(self._after_launch)

    def detach(self):
        """Take the hook out; the members go on holding what reaches them."""
        if self._after_launch in self.net.after_launch:
            self.net.after_launch.remove(self._after_launch)

    # ---- what the lakes hold
    def _wait(self):
        self.engine.stream_sync()
        self.torch.cuda.current_stream().synchronize()

    def level(self):
        """The level h [m above the datum] every lake's last release was made from (float64 device tensor)."""
        return self._level

    def outflow(self):
        """What every lake released in the last call [m3] (float32 device tensor)."""
        return self._outflow

    def volume_m3(self):
        """What every lake holds [m3]: words * quantum, float64 numpy.  One host wait."""
        self._wait()
        return self.volume.cpu().numpy().astype(np.float64) * self.quantum

    def set_volume_m3(self, v):
        """volume = floor(v / quantum) words per lake (a number or nlake values)."""
        self._wait()
        w = np.floor(np.broadcast_to(np.asarray(v, np.float64), (self.nlake,)) / self.quantum).astype(np.int64)
        self.volume.copy_(self.torch.from_numpy(w))
        self.torch.cuda.current_stream().synchronize()

    def emptied(self):
        """The number of (lake, call) pairs in which a lake released all it held.  One host wait."""
        self._wait()
        return int(self.diag.cpu().numpy().view(np.uint32)[0])

    def state_dict(self):
        """The restart words: volume (int64; with the network's own state_dict the whole restart state)."""
        self._wait()
        return dict(volume=self.volume.clone(), quantum=self.quantum)

    def load_state_dict(self, state):
        if float(state.get("quantum", self.quantum)) != self.quantum:
            raise ValueError("the restart words were made with another quantum")
        self._wait()
        self.volume.copy_(state["volume"])
        self.inflow.zero_()
        self.torch.cuda.current_stream().synchronize()
