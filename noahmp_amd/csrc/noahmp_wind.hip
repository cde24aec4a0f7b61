// Terrain-adjusted wind of the forcing (no reference counterpart; the contract is the text in include/noahmp_hip.h, the arithmetic is
// nmp_dev_wind.hpp): the MicroMet wind model with the two maxima given by the caller.
//
// noahmp_hip_wind_terrain: ONE launch per call, once per terrain.  One thread per window cell in row-major order: the lanes of a wave are
// neighbours along i, so each of the 13 heights a cell reads (the cell, its 4 neighbours at distance 1, its 8 at distance ncurv) is one
// row segment per wave, shifted by a constant -- coalesced, and shared with the neighbouring rows' workgroups through the L2: from memory
// the plane is read about once.  Three stores of 4 bytes per written cell.
// noahmp_hip_forcing_wind: ONE launch per call, one column per thread: 5 loads and 2 stores of 4 bytes, 28 bytes per column, and about 40
// float operations, three divisions (four with TURN), one square root and (with TURN) one sinf / cosf pair on an argument of about 0.25
// at most: 4.8 TB/s with the turn, 5.1 without at 7 077 888 columns, 0.89 / 0.94 of what noahmp_hip_forcing_radiation_sky reaches in the
// same run (profiles/wind_bench.md).
// Neither kernel uses LDS, a barrier, atomics or scratch.  Arguments go by value, nothing is allocated, nothing waits on the host.
#include <math.h>
#include <string.h>
#include <hip/hip_runtime.h>
#include "noahmp_hip.h"
#include "nmp_dev_wind.hpp"
#include "nmp_engine_host.hpp"

using namespace nmp;
using nmp_host::g, nmp_host::refuse, nmp_host::bad_count, nmp_host::bad_window, nmp_host::bad_spacing, nmp_host::stream_of, nmp_host::grid_1d;

namespace {

constexpr int kBlock = 256;

struct WindTerrainKArgs {
  const float* height; const float* cosalpha; const float* sinalpha;
  const int* dst_index;
  float* sx; float* sy; float* curv;
  long ncell, ndst;
  WindTerrainParams p;
};

__global__ void __launch_bounds__(kBlock) noahmp_wind_terrain_kernel(const WindTerrainKArgs k) {
  const long c = (long)blockIdx.x * kBlock + threadIdx.x;
  if (c >= k.ncell) return;
  const long d = k.dst_index ? (long)k.dst_index[c] : c;
  if (d < 0 || d >= k.ndst) return;                              // a margin cell: read by others and not written
  float ca = 1.f, sa = 0.f;
  if (k.p.has_rot) { ca = k.cosalpha[c]; sa = k.sinalpha[c]; }
  const int j = (int)(c / k.p.ni), i = (int)(c - (long)j * k.p.ni);
  const WindSlope s = wind_terrain_cell(k.p, k.height, ca, sa, i, j);
  k.sx[d] = s.sx;
  k.sy[d] = s.sy;
  k.curv[d] = s.curv;
}

struct WindKArgs {
  float* u; float* v;
  const float* sx; const float* sy; const float* curv;
  long ncell;
  WindParams p;
};

__global__ void __launch_bounds__(kBlock) noahmp_forcing_wind_kernel(const WindKArgs k) {
  const long c = (long)blockIdx.x * kBlock + threadIdx.x;
  if (c >= k.ncell) return;
  float u = k.u[c], v = k.v[c];
  if (!wind_column(k.p, k.sx[c], k.sy[c], k.curv[c], &u, &v)) return;      // the column keeps its bits: nothing is written
  k.u[c] = u;
  k.v[c] = v;
}

}  // namespace

extern "C" {

int noahmp_hip_wind_terrain(const noahmp_wind_terrain* wt, int64_t ndst, void* stream) {
  const char* me = "noahmp_hip_wind_terrain";
  if (!wt) return refuse(-105, "%s: the argument block is NULL", me);
  if (!wt->height || !wt->sx || !wt->sy || !wt->curv) return refuse(-105, "%s: height, sx, sy and curv are required", me);
  if ((wt->cosalpha != nullptr) != (wt->sinalpha != nullptr)) return refuse(-105, "%s: cosalpha and sinalpha go together: both or none", me);
  if (bad_window(wt->ni, wt->nj)) return refuse(-105, "%s: window: ni, nj >= 0 and ni*nj <= 2^31 - 1", me);
  if (wt->ncurv < 1 || wt->ncurv > NOAHMP_WIND_MAX_NCURV)
    return refuse(-105, "%s: ncurv %d (1 .. %d cells)", me, wt->ncurv, NOAHMP_WIND_MAX_NCURV);
  if (bad_spacing(wt->dx, wt->dy)) return refuse(-105, "%s: dx and dy must be finite and > 0", me);
  if (bad_count(ndst)) return refuse(-105, "%s: ndst: 0 .. 2^31 - 1", me);
  int rc = nmp_host::ensure_init();
  if (rc) return rc;
  const long ncell = (long)wt->ni * wt->nj;
  if (ndst == 0 || ncell == 0) return 0;
  hipStream_t s = stream_of(stream);
  WindTerrainKArgs k;
  memset(&k, 0, sizeof(k));
  k.height = wt->height; k.cosalpha = wt->cosalpha; k.sinalpha = wt->sinalpha; k.dst_index = wt->dst_index;
  k.sx = wt->sx; k.sy = wt->sy; k.curv = wt->curv; k.ncell = ncell; k.ndst = ndst;
  k.p = wind_terrain_params(wt->ni, wt->nj, wt->ncurv, wt->cosalpha ? 1 : 0, wt->dx, wt->dy);
  hipLaunchKernelGGL(noahmp_wind_terrain_kernel, grid_1d(ncell, kBlock), dim3(kBlock), 0, s, k);
  HIPCHK(hipGetLastError());
  return 0;
}

int noahmp_hip_forcing_wind(const noahmp_wind* w, int64_t ncell, void* stream) {
  const char* me = "noahmp_hip_forcing_wind";
  if (!w) return refuse(-105, "%s: the argument block is NULL", me);
  if (!w->u || !w->v || !w->sx || !w->sy || !w->curv) return refuse(-105, "%s: u, v, sx, sy and curv are required", me);
  if (!(isfinite(w->slope_max) && w->slope_max > 0.f)) return refuse(-105, "%s: slope_max must be finite and > 0", me);
  if (!(isfinite(w->curv_max) && w->curv_max > 0.f)) return refuse(-105, "%s: curv_max must be finite and > 0", me);
  if (bad_count(ncell)) return refuse(-105, "%s: ncell: 0 .. 2^31 - 1 columns", me);
  int rc = nmp_host::ensure_init();
  if (rc) return rc;
  if (ncell == 0) return 0;
  hipStream_t s = stream_of(stream);
  WindKArgs k;
  memset(&k, 0, sizeof(k));
  k.u = w->u; k.v = w->v; k.sx = w->sx; k.sy = w->sy; k.curv = w->curv; k.ncell = ncell;
  k.p.ds = w->slope_max + w->slope_max;
  k.p.dc = w->curv_max + w->curv_max;
  k.p.gamma_s = w->gamma_s; k.p.gamma_c = w->gamma_c;
  k.p.turn = (w->flags & NOAHMP_WIND_TURN) ? 1 : 0;
  hipLaunchKernelGGL(noahmp_forcing_wind_kernel, grid_1d(ncell, kBlock), dim3(kBlock), 0, s, k);
  HIPCHK(hipGetLastError());
  return 0;
}

}  // extern "C"
