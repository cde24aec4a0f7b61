"""ctypes mirrors of include/noahmp_hip.h, built from abi_spec.py.

Only plumbing lives here: structure definitions, the loader of the in-tree HIP
shared library, and helpers that pack numpy arrays / torch tensors into a
``noahmp_step_args`` block.  There is NO CPU fallback: if the HIP library is
missing, :func:`load_library` raises.
"""
import ctypes as C
import os

import numpy as np

from .abi_spec import STEP_FIELDS, TABLE_FIELDS, ERROR_CODES, NSNOW, WTABLE_FIELDS
from .abi_spec import HISTORY_OPS, HISTORY_FIN_FLAGS, HISTORY_ENTRY_FIELDS, HISTORY_PROBES_FIELDS
from .abi_spec import REGION_OPS, REGION_ENTRY_FIELDS
from .abi_spec import REGRID_MODES, REGRID_SOURCE_FIELDS, REGRID_ENTRY_FIELDS, REGRID_PLAN_PLANES, REGRID_MET_FIELDS
from .abi_spec import REGRID_CONSERVE_ENTRY_FIELDS, REGRID_CONSERVE_EDGES, REGRID_CONSERVE_MAX_ENTRIES
from .abi_spec import SHORTWAVE_MODES, SHORTWAVE_MAX_SAMPLES, SUN_TIME_FIELDS, SHORTWAVE_FIELDS
from .abi_spec import SHADOW_FIELDS, SHADOW_MAX_NSTEP
from .abi_spec import SKYVIEW_FIELDS, SKY_FIELDS, SKYVIEW_MAX_NDIR
from .abi_spec import WIND_TERRAIN_FIELDS, WIND_FIELDS, WIND_FLAGS
from .abi_spec import FLOW_NEIGHBOURS, FLOW_TERRAIN_FIELDS, ROUTE_FIELDS
from .abi_spec import FLOW_FILL_FIELDS, FLOW_FILL_FLAGS, FLOW_FILL_TILE, FLOW_FILL_MAX_SWEEPS
from .abi_spec import FLOW_BASIN_FIELDS, FLOW_BASIN_FLAGS, FLOW_BASIN_LABELS, FLOW_BASIN_MAX_SWEEPS
from .abi_spec import FLOW_UPSTREAM_FIELDS, FLOW_UPSTREAM_FLAGS
from .abi_spec import FLOW_CHANNEL_FIELDS, ROUTE_KINEMATIC_FIELDS
from .abi_spec import LAKE_TAKE_FIELDS, LAKE_RELEASE_FIELDS
from .abi_spec import FLOW_DROP_FIELDS, ROUTE_DIFFUSIVE_FIELDS, LAKE_DEPTH_FIELDS

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libnoahmp_hip.so")

MEM_HOST, MEM_DEVICE = 0, 1
SORT_VEG, SORT_SNOW, SORT_SNOW_FIRST, SORT_TAIR, SORT_COST = 1, 2, 4, 8, 16
HALO_TCP, HALO_RCCL, HALO_IPC = 0, 1, 2


def _step_ctype(kind):
    return {"i": C.c_int32, "f": C.c_float, "pf": C.c_void_p, "pi": C.c_void_p}[kind]


class StepArgs(C.Structure):
    """noahmp_step_args (include/noahmp_hip.h); mirrors the noahmplsm argument list, drv:11-44."""
    _fields_ = [(n, _step_ctype(k)) for n, k, lev, io, ln in STEP_FIELDS]


class WtableArgs(C.Structure):
    """noahmp_wtable_args; mirrors the WTABLE_mmf_noahmp argument list, gw:14-22."""
    _fields_ = [(n, _step_ctype(k)) for n, k, lev, io, ln in WTABLE_FIELDS]


WTABLE_INFO = {n: (k, lev, io) for n, k, lev, io, ln in WTABLE_FIELDS}
WTABLE_ARRAYS = [n for n, k, lev, io, ln in WTABLE_FIELDS if k in ("pf", "pi")]


FORCING_RECORD_FIELDS = ("t", "q", "u", "v", "p", "lw", "sw", "pcp", "fpar", "lai")


class ForcingRecord(C.Structure):
    """noahmp_forcing_record: one forcing file's planes as hrldas_input_read keeps them (netcdf_io:1228-1252)."""
    _fields_ = [(n, C.c_void_p) for n in FORCING_RECORD_FIELDS]


def _hist_ctype(kind):
    return {"i": C.c_int32, "l": C.c_int64, "f": C.c_float, "d": C.c_double, "pf": C.c_void_p, "pi": C.c_void_p, "pb": C.c_void_p, "pd": C.c_void_p,
            "pp": C.POINTER(C.c_void_p)}[kind]


class HistoryEntry(C.Structure):
    """noahmp_history_entry: one accumulator of noahmp_hip_history_step."""
    _fields_ = [(n, _hist_ctype(k)) for n, t, k, doc in HISTORY_ENTRY_FIELDS]


class HistoryProbes(C.Structure):
    """noahmp_history_probes: the point probes of noahmp_hip_history_step."""
    _fields_ = [(n, _hist_ctype(k)) for n, t, k, doc in HISTORY_PROBES_FIELDS]


HIST_OP = {nm.lower(): val for nm, val, doc in HISTORY_OPS}            # "sum", "sum_dt", "min", "max", "last"
HIST_FIN = {nm.lower(): val for nm, val, doc in HISTORY_FIN_FLAGS}     # "mean", "reset"


class RegionEntry(C.Structure):
    """noahmp_region_entry: one series of noahmp_hip_region_step."""
    _fields_ = [(n, _hist_ctype(k)) for n, t, k, doc in REGION_ENTRY_FIELDS]


REG_OP = {nm.lower(): val for nm, val, doc in REGION_OPS}              # "sum", "min", "max"


class RegridSource(C.Structure):
    """noahmp_regrid_source: the regular lat-lon grid a coarse forcing record lives on."""
    _fields_ = [(n, _hist_ctype(k)) for n, t, k, doc in REGRID_SOURCE_FIELDS]


class RegridEntry(C.Structure):
    """noahmp_regrid_entry: one plane of noahmp_hip_forcing_regrid."""
    _fields_ = [(n, _hist_ctype(k)) for n, t, k, doc in REGRID_ENTRY_FIELDS]


class RegridMet(C.Structure):
    """noahmp_regrid_met: the elevation-adjusted group (t, p, q, lw) of noahmp_hip_forcing_regrid_met."""
    _fields_ = [(n, _hist_ctype(k)) for n, t, k, doc in REGRID_MET_FIELDS]


class RegridConserveEntry(C.Structure):
    """noahmp_regrid_conserve_entry: one plane of noahmp_hip_forcing_regrid_conserve."""
    _fields_ = [(n, _hist_ctype(k)) for n, t, k, doc in REGRID_CONSERVE_ENTRY_FIELDS]


REGRID_EDGE = {nm.lower(): val for nm, val, doc in REGRID_CONSERVE_EDGES}     # "i_first", "i_last", "j_first", "j_last"
REGRID_CONSERVE_MAX = REGRID_CONSERVE_MAX_ENTRIES


class SunTime(C.Structure):
    """noahmp_sun_time: a time of the shortwave calls, as noahmp_hip_forcing_prep takes it."""
    _fields_ = [(n, _hist_ctype(k)) for n, t, k, doc in SUN_TIME_FIELDS]


class Shortwave(C.Structure):
    """noahmp_shortwave: the planes and parameters of noahmp_hip_forcing_shortwave."""
    _fields_ = [(n, _hist_ctype(k)) for n, t, k, doc in SHORTWAVE_FIELDS]


class Shadow(C.Structure):
    """noahmp_shadow: the window planes and parameters of noahmp_hip_forcing_shadow."""
    _fields_ = [(n, _hist_ctype(k)) for n, t, k, doc in SHADOW_FIELDS]


class Skyview(C.Structure):
    """noahmp_skyview: the window planes, parameters and directions of noahmp_hip_skyview."""
    _fields_ = [(n, _hist_ctype(k)) for n, t, k, doc in SKYVIEW_FIELDS]


class Sky(C.Structure):
    """noahmp_sky: the sky-view planes and parameters of noahmp_hip_forcing_radiation_sky."""
    _fields_ = [(n, _hist_ctype(k)) for n, t, k, doc in SKY_FIELDS]


class WindTerrain(C.Structure):
    """noahmp_wind_terrain: the window planes and parameters of noahmp_hip_wind_terrain."""
    _fields_ = [(n, _hist_ctype(k)) for n, t, k, doc in WIND_TERRAIN_FIELDS]


class Wind(C.Structure):
    """noahmp_wind: the planes and parameters of noahmp_hip_forcing_wind."""
    _fields_ = [(n, _hist_ctype(k)) for n, t, k, doc in WIND_FIELDS]


class FlowTerrain(C.Structure):
    """noahmp_flow_terrain: the window planes and parameters of noahmp_hip_flow_terrain."""
    _fields_ = [(n, _hist_ctype(k)) for n, t, k, doc in FLOW_TERRAIN_FIELDS]


class Route(C.Structure):
    """noahmp_route: the planes and parameters of noahmp_hip_route_runoff."""
    _fields_ = [(n, _hist_ctype(k)) for n, t, k, doc in ROUTE_FIELDS]


class FlowFill(C.Structure):
    """noahmp_flow_fill: the planes and parameters of noahmp_hip_flow_fill_init / noahmp_hip_flow_fill."""
    _fields_ = [(n, _hist_ctype(k)) for n, t, k, doc in FLOW_FILL_FIELDS]


class FlowBasin(C.Structure):
    """noahmp_flow_basin: the planes of noahmp_hip_flow_basin_init / _jump / _resolve."""
    _fields_ = [(n, _hist_ctype(k)) for n, t, k, doc in FLOW_BASIN_FIELDS]


class FlowUpstream(C.Structure):
    """noahmp_flow_upstream: the planes of noahmp_hip_flow_upstream_init / _pass."""
    _fields_ = [(n, _hist_ctype(k)) for n, t, k, doc in FLOW_UPSTREAM_FIELDS]


class FlowChannel(C.Structure):
    """noahmp_flow_channel: the window planes and parameters of noahmp_hip_flow_channel."""
    _fields_ = [(n, _hist_ctype(k)) for n, t, k, doc in FLOW_CHANNEL_FIELDS]


class RouteKinematic(C.Structure):
    """noahmp_route_kinematic: the planes and parameters of noahmp_hip_route_kinematic."""
    _fields_ = [(n, _hist_ctype(k)) for n, t, k, doc in ROUTE_KINEMATIC_FIELDS]


class LakeTake(C.Structure):
    """noahmp_lake_take: the member list and planes of noahmp_hip_lake_take."""
    _fields_ = [(n, _hist_ctype(k)) for n, t, k, doc in LAKE_TAKE_FIELDS]


class LakeRelease(C.Structure):
    """noahmp_lake_release: the words, parameter planes and outputs of noahmp_hip_lake_release."""
    _fields_ = [(n, _hist_ctype(k)) for n, t, k, doc in LAKE_RELEASE_FIELDS]


class FlowDrop(C.Structure):
    """noahmp_flow_drop: the window planes and parameters of noahmp_hip_flow_drop."""
    _fields_ = [(n, _hist_ctype(k)) for n, t, k, doc in FLOW_DROP_FIELDS]


class RouteDiffusive(C.Structure):
    """noahmp_route_diffusive: the planes and parameters of noahmp_hip_route_diffusive."""
    _fields_ = [(n, _hist_ctype(k)) for n, t, k, doc in ROUTE_DIFFUSIVE_FIELDS]


class LakeDepth(C.Structure):
    """noahmp_lake_depth: the member list and planes of noahmp_hip_lake_depth."""
    _fields_ = [(n, _hist_ctype(k)) for n, t, k, doc in LAKE_DEPTH_FIELDS]


BASIN_FLAG = {nm.lower(): val for nm, val, doc in FLOW_BASIN_FLAGS}    # "ring_w" .. "ring_n"
UPSTREAM_FLAG = {nm.lower(): val for nm, val, doc in FLOW_UPSTREAM_FLAGS}    # "ring_w" .. "ring_n"
BASIN_NONE, BASIN_PENDING, BASIN_CYCLE = (val for nm, val, doc in FLOW_BASIN_LABELS)
BASIN_MAX_SWEEPS = FLOW_BASIN_MAX_SWEEPS
FILL_FLAG = {nm.lower(): val for nm, val, doc in FLOW_FILL_FLAGS}      # "outlet_w" .. "ring_n"
FILL_TILE_I, FILL_TILE_J = FLOW_FILL_TILE
FILL_MAX_SWEEPS = FLOW_FILL_MAX_SWEEPS
FLOW_DI = tuple(di for k, di, dj, nm in FLOW_NEIGHBOURS)              # neighbour k = 1..8 at index k-1
FLOW_DJ = tuple(dj for k, di, dj, nm in FLOW_NEIGHBOURS)
WIND_FLAG = {nm.lower(): val for nm, val, doc in WIND_FLAGS}           # "turn"
SHADOW_MAX_STEPS = SHADOW_MAX_NSTEP
SKYVIEW_MAX_DIRS = SKYVIEW_MAX_NDIR
SW_MODE = {nm.lower(): val for nm, val, doc in SHORTWAVE_MODES}        # "linear", "zenith"
SW_MAX_SAMPLES = SHORTWAVE_MAX_SAMPLES
REGRID_MODE = {nm.lower(): val for nm, val, doc in REGRID_MODES}       # "bilinear", "nearest"
REGRID_PLANES = tuple(REGRID_PLAN_PLANES)                              # order of the planes of a plan workspace


def _tbl_ctype(kind, shape):
    t = C.c_int32 if kind == "i" else C.c_float
    for d in shape:           # Fortran (a,b) -> C [b][a]: wrap fastest dim first
        t = t * d
    return t


class Tables(C.Structure):
    """noahmp_tables: image of the reference's module tables (lsm:43-103, 215-259, 417-424)."""
    _fields_ = [(n, _tbl_ctype(k, s)) for n, k, s, src in TABLE_FIELDS]


class Status(C.Structure):
    _fields_ = [("code", C.c_int32), ("i", C.c_int32), ("j", C.c_int32),
                ("n_land", C.c_int32), ("n_glacier", C.c_int32), ("n_skipped", C.c_int32),
                ("kernel_ms", C.c_float)]


FIELD_INFO = {n: (k, lev, io) for n, k, lev, io, ln in STEP_FIELDS}
ARRAY_FIELDS = [n for n, k, lev, io, ln in STEP_FIELDS if k in ("pf", "pi")]


def nlev(lev, nsoil, nk_atm=2):
    return {None: 1, "atm": nk_atm, "soil": nsoil, "snow": NSNOW, "snso": NSNOW + nsoil}[lev]


def tables_to_dict(t):
    """Tables -> {name: numpy array in Fortran index order (e.g. saim[veg, month])}."""
    out = {}
    for n, k, s, src in TABLE_FIELDS:
        v = getattr(t, n)
        if s:
            a = np.ctypeslib.as_array(v).copy()
            out[n] = a.T.copy() if len(s) > 1 else a
        else:
            out[n] = v
    return out


def tables_from_dict(d):
    t = Tables()
    for n, k, s, src in TABLE_FIELDS:
        if s:
            dt = np.int32 if k == "i" else np.float32
            a = np.asarray(d[n], dtype=dt)
            assert a.shape == tuple(s), (n, a.shape, s)
            src_arr = np.ascontiguousarray(a.T) if len(s) > 1 else np.ascontiguousarray(a)
            C.memmove(C.addressof(getattr(t, n)), src_arr.ctypes.data, src_arr.nbytes)
        else:
            setattr(t, n, int(d[n]) if k == "i" else float(d[n]))
    return t


_lib = None


def load_library(path=None):
    """Load the in-tree HIP engine.  Fails loudly when it is missing (no CPU fallback)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise RuntimeError(
            "HIP engine %s not built. Run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback." % p)
    # PyTorch-ROCm wheels bundle their own libamdhip64.so.7; two HIP runtimes in one process
    # cannot both own the device.  Importing torch first makes the loader resolve this library's
    # libamdhip64.so.7 dependency to the copy torch already mapped (same SONAME).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(p)
    lib.noahmp_hip_abi_version.restype = C.c_int
    lib.noahmp_hip_nsoil.restype = C.c_int
    lib.noahmp_hip_nsoil.argtypes = []
    lib.noahmp_hip_sizeof_step_args.restype = C.c_size_t
    lib.noahmp_hip_sizeof_tables.restype = C.c_size_t
    lib.noahmp_hip_device_count.restype = C.c_int
    lib.noahmp_hip_set_device.argtypes = [C.c_int]
    lib.noahmp_hip_set_tables.argtypes = [C.POINTER(Tables)]
    lib.noahmp_hip_step.argtypes = [C.POINTER(StepArgs), C.c_int, C.c_void_p, C.POINTER(Status)]
    lib.noahmp_hip_fetch.argtypes = [C.POINTER(StepArgs)]
    lib.noahmp_hip_step_async.argtypes = [C.POINTER(StepArgs), C.c_void_p]
    lib.noahmp_hip_sync.argtypes = [C.POINTER(Status), C.POINTER(C.c_int)]
    lib.noahmp_hip_sync_timing.argtypes = [C.POINTER(C.c_float), C.c_int]
    lib.noahmp_hip_sync_step_timing.argtypes = [C.POINTER(C.c_float), C.c_int]
    lib.noahmp_hip_sync_counts.argtypes = [C.POINTER(C.c_int64), C.c_int]
    lib.noahmp_hip_fetch_cost.argtypes = [C.c_void_p, C.c_long, C.c_void_p]
    lib.noahmp_hip_fetch_cost.restype = C.c_long
    lib.noahmp_hip_init.argtypes = [C.POINTER(StepArgs), C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(Status)]
    lib.noahmp_hip_forcing_prep.argtypes = [C.POINTER(StepArgs), C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                            C.c_float, C.c_int, C.POINTER(C.c_float), C.c_int, C.c_void_p, C.POINTER(Status)]
    lib.noahmp_hip_forcing_interpolate.argtypes = [C.POINTER(StepArgs), C.POINTER(ForcingRecord), C.POINTER(ForcingRecord),
                                                   C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(Status)]
    lib.noahmp_hip_forcing_interpolate_prep.argtypes = [C.POINTER(StepArgs), C.POINTER(ForcingRecord), C.POINTER(ForcingRecord), C.c_int, C.c_int,
                                                        C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int,
                                                        C.POINTER(C.c_float), C.c_int, C.c_void_p, C.POINTER(Status)]
    lib.noahmp_hip_gather_fields.argtypes = [C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int),
                                             C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    lib.noahmp_hip_output_fields.argtypes = [C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int),
                                             C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_int, C.c_int, C.c_void_p]
    lib.noahmp_hip_history_step.argtypes = [C.c_int, C.POINTER(HistoryEntry), C.POINTER(HistoryProbes), C.POINTER(StepArgs), C.c_void_p,
                                            C.c_void_p]
    lib.noahmp_hip_history_finish.argtypes = [C.c_int, C.POINTER(HistoryEntry), C.POINTER(C.c_void_p), C.POINTER(C.c_uint32), C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_int, C.c_void_p]
    lib.noahmp_hip_region_plan_size.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64)]
    lib.noahmp_hip_region_plan.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    lib.noahmp_hip_region_plan_follow.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.noahmp_hip_region_scratch_size.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int64)]
    lib.noahmp_hip_region_step.argtypes = [C.c_void_p, C.c_int, C.POINTER(RegionEntry), C.POINTER(StepArgs), C.c_void_p, C.c_int, C.c_int,
                                           C.c_void_p, C.c_void_p, C.c_void_p]
    lib.noahmp_hip_regrid_plan_size.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int64)]
    lib.noahmp_hip_regrid_plan_latlon.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(RegridSource), C.c_void_p, C.c_int,
                                                  C.c_void_p, C.c_int64, C.POINTER(C.c_int32), C.c_void_p]
    lib.noahmp_hip_forcing_regrid.argtypes = [C.c_void_p, C.c_int64, C.POINTER(RegridSource), C.c_int, C.POINTER(RegridEntry), C.c_void_p]
    lib.noahmp_hip_forcing_regrid_met.argtypes = [C.c_void_p, C.c_int64, C.POINTER(RegridSource), C.POINTER(RegridMet), C.c_int,
                                                  C.POINTER(RegridEntry), C.c_void_p]
    lib.noahmp_hip_regrid_conserve_plan_size.argtypes = [C.c_int, C.c_int, C.POINTER(RegridSource), C.POINTER(C.c_int64)]
    lib.noahmp_hip_regrid_conserve_plan.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(RegridSource), C.c_void_p, C.c_void_p, C.c_int,
                                                    C.c_void_p, C.c_int64, C.POINTER(C.c_int32), C.c_void_p]
    lib.noahmp_hip_regrid_conserve_scratch_size.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int64)]
    lib.noahmp_hip_forcing_regrid_conserve.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(RegridSource), C.c_void_p, C.c_int64, C.c_int,
                                                       C.POINTER(RegridConserveEntry), C.c_void_p, C.c_void_p, C.c_void_p]
    lib.noahmp_hip_forcing_cosz_mean.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.POINTER(SunTime), C.c_void_p, C.c_void_p]
    lib.noahmp_hip_forcing_shortwave.argtypes = [C.POINTER(Shortwave), C.c_int64, C.POINTER(SunTime), C.c_void_p]
    lib.noahmp_hip_forcing_shadow.argtypes = [C.POINTER(Shadow), C.c_int64, C.POINTER(SunTime), C.c_void_p]
    lib.noahmp_hip_forcing_shortwave_lit.argtypes = [C.POINTER(Shortwave), C.c_void_p, C.c_int64, C.POINTER(SunTime), C.c_void_p]
    lib.noahmp_hip_skyview.argtypes = [C.POINTER(Skyview), C.c_int64, C.c_void_p]
    lib.noahmp_hip_forcing_radiation_sky.argtypes = [C.POINTER(Shortwave), C.POINTER(Sky), C.c_int64, C.POINTER(SunTime), C.c_void_p]
    lib.noahmp_hip_wind_terrain.argtypes = [C.POINTER(WindTerrain), C.c_int64, C.c_void_p]
    lib.noahmp_hip_forcing_wind.argtypes = [C.POINTER(Wind), C.c_int64, C.c_void_p]
    lib.noahmp_hip_flow_terrain.argtypes = [C.POINTER(FlowTerrain), C.c_void_p]
    lib.noahmp_hip_flow_inmask.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    lib.noahmp_hip_flow_accumulate.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    lib.noahmp_hip_route_runoff.argtypes = [C.POINTER(Route), C.c_int64, C.c_void_p]
    lib.noahmp_hip_flow_fill_init.argtypes = [C.POINTER(FlowFill), C.c_void_p]
    lib.noahmp_hip_flow_fill.argtypes = [C.POINTER(FlowFill), C.c_void_p]
    for fn in (lib.noahmp_hip_flow_basin_init, lib.noahmp_hip_flow_basin_jump, lib.noahmp_hip_flow_basin_resolve):
        fn.argtypes = [C.POINTER(FlowBasin), C.c_void_p]
    for fn in (lib.noahmp_hip_flow_upstream_init, lib.noahmp_hip_flow_upstream_pass):
        fn.argtypes = [C.POINTER(FlowUpstream), C.c_void_p]
    lib.noahmp_hip_flow_channel.argtypes = [C.POINTER(FlowChannel), C.c_void_p]
    lib.noahmp_hip_route_kinematic.argtypes = [C.POINTER(RouteKinematic), C.c_int64, C.c_void_p]
    lib.noahmp_hip_lake_take.argtypes = [C.POINTER(LakeTake), C.c_void_p]
    lib.noahmp_hip_lake_release.argtypes = [C.POINTER(LakeRelease), C.c_void_p]
    lib.noahmp_hip_flow_drop.argtypes = [C.POINTER(FlowDrop), C.c_void_p]
    lib.noahmp_hip_route_diffusive.argtypes = [C.POINTER(RouteDiffusive), C.c_int64, C.c_void_p]
    lib.noahmp_hip_lake_depth.argtypes = [C.POINTER(LakeDepth), C.c_void_p]
    lib.noahmp_hip_scatter_fields.argtypes = [C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int),
                                              C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    lib.noahmp_hip_sorted_exchange.argtypes = [C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_void_p, C.c_void_p,
                                               C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.noahmp_hip_sort_columns.argtypes = [C.POINTER(StepArgs), C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                            C.POINTER(C.c_int64), C.c_void_p]
    lib.noahmp_hip_sort_staleness.argtypes = [C.POINTER(StepArgs), C.c_int, C.c_void_p, C.POINTER(C.c_int64), C.c_void_p]
    lib.noahmp_hip_sort_staleness_async.argtypes = [C.POINTER(StepArgs), C.c_int, C.c_void_p, C.c_void_p]
    lib.noahmp_hip_sort_staleness_result.argtypes = [C.POINTER(C.c_int64), C.c_int]
    lib.noahmp_hip_sort_set_band.argtypes = [C.c_void_p]
    lib.noahmp_hip_sort_set_veg_order.argtypes = [C.POINTER(C.c_int32), C.c_int]
    lib.noahmp_hip_permute_step_arrays.argtypes = [C.POINTER(StepArgs), C.POINTER(StepArgs), C.c_void_p, C.c_void_p]
    lib.noahmp_hip_scatter_plan.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.noahmp_hip_stream_sync.argtypes = [C.c_void_p]
    lib.noahmp_hip_declination.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    lib.noahmp_hip_declination.restype = C.c_float
    lib.noahmp_hip_wtable_mmf.argtypes = [C.POINTER(WtableArgs), C.c_int, C.c_void_p, C.POINTER(Status)]
    lib.noahmp_hip_wtable_mmf_async.argtypes = [C.POINTER(WtableArgs), C.c_void_p]
    lib.noahmp_hip_wtable_lateral_async.argtypes = [C.POINTER(WtableArgs), C.c_void_p, C.c_void_p]
    lib.noahmp_hip_wtable_columns_async.argtypes = [C.POINTER(WtableArgs), C.c_void_p, C.c_void_p]
    lib.noahmp_hip_halo_init.argtypes = [C.c_int, C.c_int, C.c_char_p, C.c_int, C.c_int]
    lib.noahmp_hip_exchange_halo.argtypes = [C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.c_int, C.c_void_p]
    lib.noahmp_hip_groundwater_init.argtypes = [C.POINTER(WtableArgs), C.c_int, C.c_int, C.c_void_p, C.POINTER(Status)]
    lib.noahmp_hip_sizeof_wtable_args.restype = C.c_size_t
    lib.noahmp_hip_malloc.argtypes = [C.c_size_t]
    lib.noahmp_hip_malloc.restype = C.c_void_p
    lib.noahmp_hip_memcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    lib.noahmp_hip_free.argtypes = [C.c_void_p]
    lib.noahmp_hip_free.restype = None
    lib.noahmp_hip_jit_compile_check.argtypes = [C.POINTER(C.c_int32), C.c_char_p, C.c_size_t]
    lib.noahmp_hip_jit_cache_info.argtypes = [C.POINTER(C.c_int32)]
    lib.noahmp_hip_jit_cache_info.restype = C.c_char_p
    lib.noahmp_hip_jit_source_hash.restype = C.c_uint64
    lib.noahmp_hip_set_option.argtypes = [C.c_char_p, C.c_int]
    lib.noahmp_hip_debug_copy_stats.argtypes = [C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]
    lib.noahmp_hip_debug_copy_stats.restype = None
    lib.noahmp_hip_error_string.argtypes = [C.c_int]
    lib.noahmp_hip_error_string.restype = C.c_char_p
    lib.noahmp_hip_last_error.restype = C.c_char_p
    lib.noahmp_hip_finalize.restype = None
    if lib.noahmp_hip_sizeof_step_args() != C.sizeof(StepArgs):
        raise RuntimeError("ABI drift: sizeof(noahmp_step_args) %d != ctypes %d"
                           % (lib.noahmp_hip_sizeof_step_args(), C.sizeof(StepArgs)))
    if lib.noahmp_hip_sizeof_wtable_args() != C.sizeof(WtableArgs):
        raise RuntimeError("ABI drift: sizeof(noahmp_wtable_args)")
    if lib.noahmp_hip_sizeof_tables() != C.sizeof(Tables):
        raise RuntimeError("ABI drift: sizeof(noahmp_tables)")
    if path is None:
        _lib = lib
    return lib


EXPORTED_SYMBOLS = [
    "noahmp_hip_abi_version", "noahmp_hip_nsoil", "noahmp_hip_sizeof_step_args", "noahmp_hip_sizeof_tables",
    "noahmp_hip_device_count", "noahmp_hip_set_device", "noahmp_hip_set_tables",
    "noahmp_hip_step", "noahmp_hip_fetch", "noahmp_hip_step_async", "noahmp_hip_sync", "noahmp_hip_sync_timing", "noahmp_hip_sync_step_timing", "noahmp_hip_sync_counts", "noahmp_hip_fetch_cost", "noahmp_hip_init", "noahmp_hip_forcing_prep", "noahmp_hip_forcing_interpolate", "noahmp_hip_forcing_interpolate_prep", "noahmp_hip_declination", "noahmp_hip_gather_fields", "noahmp_hip_output_fields", "noahmp_hip_history_step", "noahmp_hip_history_finish", "noahmp_hip_region_plan_size", "noahmp_hip_region_plan", "noahmp_hip_region_plan_follow", "noahmp_hip_region_scratch_size", "noahmp_hip_region_step", "noahmp_hip_regrid_plan_size", "noahmp_hip_regrid_plan_latlon", "noahmp_hip_forcing_regrid", "noahmp_hip_forcing_regrid_met", "noahmp_hip_regrid_conserve_plan_size", "noahmp_hip_regrid_conserve_plan", "noahmp_hip_regrid_conserve_scratch_size", "noahmp_hip_forcing_regrid_conserve", "noahmp_hip_forcing_cosz_mean", "noahmp_hip_forcing_shortwave", "noahmp_hip_forcing_shadow", "noahmp_hip_forcing_shortwave_lit", "noahmp_hip_skyview", "noahmp_hip_forcing_radiation_sky", "noahmp_hip_wind_terrain", "noahmp_hip_forcing_wind", "noahmp_hip_flow_terrain", "noahmp_hip_flow_inmask", "noahmp_hip_flow_accumulate", "noahmp_hip_route_runoff", "noahmp_hip_flow_fill_init", "noahmp_hip_flow_fill", "noahmp_hip_flow_basin_init", "noahmp_hip_flow_basin_jump", "noahmp_hip_flow_basin_resolve", "noahmp_hip_flow_upstream_init", "noahmp_hip_flow_upstream_pass", "noahmp_hip_flow_channel", "noahmp_hip_route_kinematic", "noahmp_hip_lake_take", "noahmp_hip_lake_release", "noahmp_hip_flow_drop", "noahmp_hip_route_diffusive", "noahmp_hip_lake_depth", "noahmp_hip_scatter_fields", "noahmp_hip_scatter_chunk", "noahmp_hip_scatter_chunk_of", "noahmp_hip_index_width", "noahmp_hip_sorted_exchange", "noahmp_hip_sort_columns", "noahmp_hip_sort_set_band", "noahmp_hip_sort_set_veg_order", "noahmp_hip_sort_staleness", "noahmp_hip_sort_staleness_async", "noahmp_hip_sort_staleness_result", "noahmp_hip_permute_step_arrays", "noahmp_hip_scatter_plan", "noahmp_hip_stream_sync", "noahmp_hip_wtable_mmf", "noahmp_hip_wtable_mmf_async", "noahmp_hip_wtable_lateral_async", "noahmp_hip_wtable_columns_async", "noahmp_hip_groundwater_init", "noahmp_hip_halo_init", "noahmp_hip_exchange_halo", "noahmp_hip_halo_finalize", "noahmp_hip_halo_selftest_rccl", "noahmp_hip_sizeof_wtable_args", "noahmp_hip_malloc", "noahmp_hip_memcpy", "noahmp_hip_free", "noahmp_hip_jit_compile_check", "noahmp_hip_jit_cache_info", "noahmp_hip_jit_source_hash", "noahmp_hip_set_option", "noahmp_hip_debug_live_host_registrations", "noahmp_hip_debug_copy_stats", "noahmp_hip_error_string",
    "noahmp_hip_last_error", "noahmp_hip_finalize",
]


def error_name(code):
    return ERROR_CODES.get(code, ("unknown", ""))[0]
